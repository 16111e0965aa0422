"""ctypes binding of libsyzsig.so (the C ABI declared in include/syzsig.h).

The library is built in-tree (``make`` -> ``syzkaller_amd/libsyzsig.so``).
There is no fallback: if it is missing, importing the GPU API raises.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_int8, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SYZSIG_LIB") or os.path.join(_HERE, "libsyzsig.so")  # SYZSIG_LIB: an experiment build

SYZSIG_OK = 0
SYZSIG_EIO = -5
SYZSIG_ENOMEM = -12
SYZSIG_EINVAL = -22
SYZSIG_ERANGE = -34
SYZSIG_ECORRUPT = -74
SYZSIG_DEBUG_FIN_DEFER = 32
SYZSIG_DEBUG_MIN_ATOMIC = 64
SYZSIG_DEBUG_EXACT_CELLS = 128
SYZSIG_DEBUG_CAP_SPILL = 256
SYZSIG_DEBUG_RECS_GATE = 512
SYZSIG_DEBUG_EDGE_MARKALL = 1024
SYZSIG_DEBUG_EDGE_PASSES = 2048
SYZSIG_DEBUG_POLL_FAIL = 4096
SYZSIG_DEBUG_AGG_IDX64 = 8192
SYZSIG_COVER_DEDUP = 1
# the KCOV target of syzsig_edge_derive_target_dev / syzsig_edge_cover_target_dev (syzkaller_amd/targets.py)
SYZSIG_TARGET_PC32 = 1  # cover_t = uint32: the trace holds u32 PCs
SYZSIG_TARGET_CHECK_X86 = 2  # cover_check(uint64) = the x86 text range
SYZSIG_TARGET_LINUX_AMD64 = SYZSIG_TARGET_CHECK_X86  # what the entry points without `_target` run
SYZSIG_COVER_TILE = 4096  # include/syzsig.h: longer segments leave the one-workgroup LDS sort
SYZSIG_COMPS_TILE = 2048  # the same for the comparison hints' keys (comps.hip)
SYZSIG_CORPUS_TILE = 2048  # the same for a corpus key's entries in the NewInput batch (corpus.hip)
SYZSIG_ITEMS_TILE = 4096  # the same for a triage item's records (items.hip)
SYZSIG_POLLRES_TILE = 4096  # a poll reply's Serial past it leaves the one-workgroup LDS table (pollres.hip)
SYZSIG_SEG_MAXSIGNAL = 0  # syzsig_fuzzer_poll_res_dev: a reply's MaxSignal (fuzzer.go:344-347)
SYZSIG_SEG_INPUT = 1  # ... the Signal of one of its NewInputs (fuzzer.go:348-350)
SYZSIG_INPUT_PRESENT = 1  # a NewInput batch row that is the key's old corpus entry
SYZSIG_HINT_LIST = 1024  # the per-arg candidate list of syzsig_hint_mutants_dev in LDS (hints.hip)
SYZSIG_HINT_MAX_DATA = 100  # prog/hints.go:38 maxDataLength
SYZSIG_SIG_BYTES = 20  # hash.Sig, pkg/hash/hash.go:14
SYZSIG_HASH_MAX_MSG = 1 << 28  # syzsig_hash_dev: the longest message
SYZSIG_HASH_STAGE = 32768  # ... a wave's span up to this is staged in LDS (sigs.hip)
SYZSIG_HASH_LONG = 4096  # ... a message past this goes to the second launch
SYZSIG_SIGSET_TILE = 2048  # the sort tile of a batch of Sigs (sigs.hip)
SYZSIG_DB_END_EOF, SYZSIG_DB_END_BAD_HEADER, SYZSIG_DB_END_BAD_MAGIC, SYZSIG_DB_END_TRUNCATED = range(4)  # db_scan
(SYZSIG_INFLATE_OK, SYZSIG_INFLATE_TRUNCATED, SYZSIG_INFLATE_INVALID, SYZSIG_INFLATE_TRAILING,
 SYZSIG_INFLATE_TOO_LONG) = range(5)  # syzsig_inflate_dev's d_status
SYZSIG_INFLATE_MAX_OUT = SYZSIG_HASH_MAX_MSG  # ... the longest output of one stream
SYZSIG_INFLATE_LONG = 4096  # ... a stream of more compressed bytes goes to the second launch (db.hip)
SYZSIG_DEFLATE_LONG = 4096  # syzsig_deflate_dev: a value of more bytes goes to the second launch (db.hip)
SYZSIG_PRIO_MAX_CALLS = 16384  # syzsig_calc_prios_dev: len(target.Syscalls) at most (one LDS row, prio.hip)
SYZSIG_PRIO_SPLIT = 4096  # ... a call with more occurrences has its row counted in slices
SYZSIG_FILESET_TILE = 2048  # syzsig_file_set_dev: a file of more frames leaves the one-workgroup LDS sort (report.hip)
SYZSIG_PROGTEXT_DESERIALIZE, SYZSIG_PROGTEXT_CALLSET = 0, 1  # syzsig_prog_calls_dev's mode (csrc/calls.hip)
SYZSIG_PROGTEXT_MAX_LINE = 1 << 20  # ... a line of this many bytes or more fails its program (bufio.Scanner's buffer)
SYZSIG_PROGTEXT_TILE = 4096  # ... the bytes of text a workgroup stages
SYZSIG_PROGTEXT_WINDOW = 256  # ... and those behind them: a head that does not end there goes to the second launch
SYZSIG_PROGTEXT_SORT_TILE = 2048  # ... CallSet's dedup: a program of more known calls leaves the one-workgroup LDS sort
(SYZSIG_PT_OK, SYZSIG_PT_LINE_TOO_LONG, SYZSIG_PT_BAD_IDENT, SYZSIG_PT_BAD_HEAD, SYZSIG_PT_UNKNOWN_CALL,
 SYZSIG_PT_NO_BRACKET, SYZSIG_PT_EMPTY_NAME, SYZSIG_PT_NO_CALLS) = range(8)  # syzsig_prog_calls_dev's d_status
SYZSIG_ARCH_AMD64, SYZSIG_ARCH_386, SYZSIG_ARCH_ARM64, SYZSIG_ARCH_ARM, SYZSIG_ARCH_PPC64LE = range(5)  # report_pcs
SYZSIG_INGEST_OK = 0
SYZSIG_INGEST_ECOMPS = 8
SYZSIG_INGEST_ECOMPTYPE = 9


class SyzsigError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"syzsig error {code}: {msg}")
        self.code = code


class CorruptedSerial(SyzsigError):
    """panic("corrupted Serial") of pkg/signal/signal.go:60-62."""


class SynthCfg(ctypes.Structure):
    _fields_ = [("seed", c_uint64), ("nblocks_log2", c_uint32), ("region_log2", c_uint32),
                ("nsys", c_uint32), ("skew", c_uint32), ("restart_log2", c_uint32),
                ("errno_permille", c_uint32), ("any_permille", c_uint32), ("bad_pc_ppm", c_uint32),
                ("global_walk", c_uint32)]


class Batch(ctypes.Structure):
    _fields_ = [("sigs", c_void_p), ("call_start", c_void_p), ("call_len", c_void_p),
                ("call_prio", c_void_p), ("ncalls", c_uint64), ("nrec", c_uint64),
                ("new_bits", c_void_p), ("call_new", c_void_p), ("new_pairs", c_void_p),
                ("new_pairs_cap", c_uint64)]


class BatchStats(ctypes.Structure):
    _fields_ = [("records", c_uint64), ("survivors", c_uint64), ("candidates", c_uint64), ("changed", c_uint64),
                ("inserted", c_uint64), ("new_signal_len", c_uint64), ("retries", c_uint64),
                ("runs", c_uint64), ("parts", c_uint64), ("distinct", c_uint64), ("overflow_parts", c_uint64),
                ("new_pairs", c_uint64), ("part_ms", ctypes.c_double), ("probe_ms", ctypes.c_double), ("decide_ms", ctypes.c_double)]

    def as_dict(self):
        return {f[0]: (float if f[1] is ctypes.c_double else int)(getattr(self, f[0])) for f in self._fields_}


class StepStatus(ctypes.Structure):
    """syzsig_step_status: what syzsig_step_finish reports for one sharded step."""
    _fields_ = [("src_void", c_uint64), ("global_void", c_uint64), ("owners_void", c_uint64), ("records", c_uint64),
                ("distinct", c_uint64), ("sent", c_uint64), ("max_out", c_uint64), ("received", c_uint64),
                ("max_in", c_uint64), ("own_distinct", c_uint64), ("inserted", c_uint64), ("changed", c_uint64),
                ("new_pairs", c_uint64), ("own_parts", c_uint64), ("src_ms", ctypes.c_double),
                ("own_ms", ctypes.c_double), ("back_ms", ctypes.c_double)]

    def as_dict(self):
        return {f[0]: (float if f[1] is ctypes.c_double else int)(getattr(self, f[0])) for f in self._fields_}


STEP_HDR_VOID = 1 << 63
STEP_HDR_OVF = 1 << 62
STEP_HDR_COUNT = (1 << 40) - 1

_P = c_void_p
_PP = POINTER(c_void_p)

# name -> (restype, argtypes); must cover every function of include/syzsig.h
SIGNATURES = {
    "syzsig_abi_version": (c_int, []),
    "syzsig_last_error": (c_char_p, []),
    "syzsig_ctx_create": (c_int, [c_int, _PP]),
    "syzsig_ctx_destroy": (None, [_P]),
    "syzsig_ctx_set_stream": (c_int, [_P, _P]),
    "syzsig_ctx_stream": (_P, [_P]),
    "syzsig_ctx_set_timing": (c_int, [_P, c_int]),
    "syzsig_ctx_set_agg": (c_int, [_P, c_int, ctypes.c_uint32]),
    "syzsig_ctx_set_debug": (c_int, [_P, ctypes.c_uint32]),
    "syzsig_ctx_last_ms": (ctypes.c_double, [_P]),
    "syzsig_copy_bw_dev": (c_int, [_P, _P, _P, c_uint64, POINTER(ctypes.c_double)]),
    "syzsig_host_alloc": (c_int, [_P, c_uint64, POINTER(_P)]),
    "syzsig_host_free": (c_int, [_P, _P]),
    "syzsig_set_make": (c_int, [_P, c_uint64, _PP]),
    "syzsig_set_free": (None, [_P]),
    "syzsig_set_clone": (c_int, [_P, _P, _PP]),
    "syzsig_set_clear": (c_int, [_P, _P]),
    "syzsig_set_copy_from": (c_int, [_P, _P, _P]),
    "syzsig_set_restore_keys": (c_int, [_P, _P, _P, _P]),
    "syzsig_set_equal": (c_int, [_P, _P, _P, ctypes.POINTER(c_int)]),
    "syzsig_set_reserve": (c_int, [_P, _P, c_uint64]),
    "syzsig_len": (c_uint64, [_P]),
    "syzsig_empty": (c_int, [_P]),
    "syzsig_capacity": (c_uint64, [_P]),
    "syzsig_from_raw": (c_int, [_P, _P, c_uint64, c_uint8, _PP]),
    "syzsig_serialize": (c_int, [_P, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    "syzsig_serialize_batch": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P]),
    "syzsig_deserialize": (c_int, [_P, _P, c_uint64, _P, c_uint64, _PP]),
    "syzsig_deserialize_dev": (c_int, [_P, _P, _P, c_uint64, _PP]),
    "syzsig_diff": (c_int, [_P, _P, _P, _PP]),
    "syzsig_diff_raw": (c_int, [_P, _P, _P, c_uint64, c_uint8, _PP]),
    "syzsig_intersection": (c_int, [_P, _P, _P, _PP]),
    "syzsig_merge": (c_int, [_P, _PP, _P]),
    "syzsig_manager_poll_batch": (c_int, [_P, _PP, _P, c_uint32, _P, _P, _P, _P, c_uint32, _P]),
    "syzsig_manager_new_input_batch": (c_int, [_P, _PP, _PP, c_uint32, c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                               _P, _P, _P, c_uint64, _P, _P, c_uint64]),
    "syzsig_new_input_stats": (c_int, [_P, _P]),
    "syzsig_cover_merge": (c_int, [_P, _PP, _P, c_uint64]),
    "syzsig_cover_merge_dev": (c_int, [_P, _PP, _P, c_uint64]),
    "syzsig_triage_runs_dev": (c_int, [_P, _P, c_uint64, _P, _P, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _P]),
    "syzsig_minimize_pred_dev": (c_int, [_P, _P, c_uint64, _P, _P, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _P]),
    "syzsig_minimize": (c_int, [_P, _P, _P, _P, c_uint64, c_uint64, _P, POINTER(c_uint64)]),
    "syzsig_minimize_dev": (c_int, [_P, _P, _P, _P, c_uint64, c_uint64, _P, POINTER(c_uint64)]),
    "syzsig_minimize_shard_dev": (c_int, [_P, _P, _P, _P, c_uint64, c_uint32, c_uint32, c_uint64, _P, POINTER(c_uint64)]),
    "syzsig_minimize_split_dev": (c_int, [_P, _P, _P, _P, c_uint64, c_uint32, c_uint32, c_uint32, c_uint64, _P,
                                          c_uint64, _P]),
    "syzsig_minimize_resolve_dev": (c_int, [_P, _P, c_uint64, _P, c_uint64, _P, POINTER(c_uint64)]),
    "syzsig_check_new_signal": (c_int, [_P, _PP, _PP, _P, c_uint64, _P, _P, _P, c_uint32, _P,
                                        POINTER(c_uint32), _P]),
    "syzsig_triage_batch": (c_int, [_P, _P, _PP, POINTER(Batch), POINTER(BatchStats)]),
    "syzsig_edge_derive_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint64, _P, _P, _P]),
    "syzsig_edge_cover_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint64, _P, c_uint32, _P, _P]),
    "syzsig_edge_derive_target_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint64, c_uint32, _P, _P, _P]),
    "syzsig_edge_cover_target_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint64, _P, c_uint32, c_uint32, _P,
                                             _P]),
    "syzsig_triage_cover_dev": (c_int, [_P, c_uint64, c_uint32, _P, _P, _P, _P, _P, _P, c_uint64, _P, _P, _P, _P,
                                        c_uint64, POINTER(c_uint64)]),
    "syzsig_triage_items_dev": (c_int, [_P, _P, c_uint64, _P, _P, _P, c_uint64, _P, _P, _P, _P, c_uint64, _P, _P, c_uint64,
                                        _P, _P, _P, c_uint64, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    "syzsig_triage_items_stats": (c_int, [_P, _P]),
    "syzsig_corpus_add_inputs_dev": (c_int, [_P, _P, _P, c_uint64, _P, c_uint64, _P, _PP, _PP]),
    "syzsig_fuzzer_poll_res_dev": (c_int, [_P, _P, _P, c_uint64, _P, _P, c_uint64, _PP, _PP]),
    "syzsig_poll_res_stats": (c_int, [_P, _P]),
    "syzsig_exec_comps_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, c_uint64, _P, _P, _P]),
    "syzsig_comp_map_dev": (c_int, [_P, _P, c_uint64, _P, _P, _P, c_uint64, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    "syzsig_shrink_expand_dev": (c_int, [_P, _P, _P, c_uint64, c_uint64, _P, _P, c_uint64, _P, c_uint32, _P, _P,
                                         c_uint64, POINTER(c_uint64)]),
    "syzsig_hint_mutants_dev": (c_int, [_P, _P, _P, c_uint64, c_uint64, _P, _P, _P, _P, _P, c_uint64, c_uint64, _P,
                                        c_uint32, _P, _P, _P, _P, c_uint64, POINTER(c_uint64)]),
    "syzsig_hint_mutants_stats": (c_int, [_P, _P]),
    "syzsig_hash_dev": (c_int, [_P, _P, _P, c_uint64, c_uint64, _P]),
    "syzsig_hash_stats": (c_int, [_P, _P]),
    "syzsig_sigset_make": (c_int, [_P, _PP]),
    "syzsig_sigset_free": (None, [_P]),
    "syzsig_sigset_len": (c_uint64, [_P]),
    "syzsig_sigset_add_dev": (c_int, [_P, _PP, _P, c_uint64, _P]),
    "syzsig_sigset_contains_dev": (c_int, [_P, _P, _P, c_uint64, _P]),
    "syzsig_sigset_export_dev": (c_int, [_P, _P, _P, c_uint64, POINTER(c_uint64)]),
    "syzsig_number_sigs_dev": (c_int, [_P, _P, _P, c_uint64, _P, _P, _P, POINTER(c_uint64)]),
    "syzsig_hub_sync_dev": (c_int, [_P, _PP, _P, c_uint64, _P, _P, c_uint64, POINTER(c_uint64)]),
    "syzsig_db_scan": (c_int, [_P, c_uint64, c_uint64, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint32), _P, _P, _P,
                               _P, _P]),
    "syzsig_inflate_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint64, _P, _P, POINTER(c_uint64)]),
    "syzsig_inflate_stats": (c_int, [_P, _P]),
    "syzsig_db_live_dev": (c_int, [_P, _P, _P, c_uint64, c_uint64, _P, POINTER(c_uint64), POINTER(c_uint64)]),
    "syzsig_deflate_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P, c_uint64, _P, POINTER(c_uint64)]),
    "syzsig_deflate_stats": (c_int, [_P, _P]),
    "syzsig_deflate_host": (c_int, [_P, c_uint64, _P, c_uint64, POINTER(c_uint64)]),
    "syzsig_db_records_dev": (c_int, [_P, _P, _P, c_uint64, _P, c_uint64, _P, _P, c_uint64, _P, POINTER(c_uint64)]),
    "syzsig_db_apply_dev": (c_int, [_P, _P, _P, c_uint64, _P, c_uint64, _P, _P, _P, c_uint64, _P, c_uint64, _P, _P, _P, _P,
                                    POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    "syzsig_calltab_make":(c_int, [_P, _P, _P, c_uint64, _PP]),
    "syzsig_calltab_free": (None, [_P]),
    "syzsig_calltab_len": (c_uint64, [_P]),
    "syzsig_prog_calls_dev": (c_int, [_P, _P, _P, c_uint64, _P, c_uint64, c_uint32, _P, _P, _P, c_uint64, _P, _P, _P,
                                      POINTER(c_uint64)]),
    "syzsig_prog_calls_stats": (c_int, [_P, _P]),
    "syzsig_calc_prios_dev": (c_int, [_P, _P, _P, c_uint64, c_uint64, c_uint64, c_uint64, _P, _P]),
    "syzsig_static_prio_finish_dev": (c_int, [_P, _P, c_uint64]),
    "syzsig_choice_table_dev": (c_int, [_P, _P, _P, c_uint64, _P]),
    "syzsig_choice_lookup_dev": (c_int, [_P, _P, c_uint64, _P, _P, c_uint64, _P]),
    "syzsig_prio_stats": (c_int, [_P, _P]),
    "syzsig_call_cover_dev": (c_int, [_P, _P, _P, c_uint64, c_uint64, _P, _P, c_uint64, _P, _P, _P, _P, c_uint64, _P,
                                      POINTER(c_uint64)]),
    "syzsig_report_pcs_dev": (c_int, [_P, _P, c_uint64, c_uint32, c_uint32, _P, _P]),
    "syzsig_uncovered_pcs_dev": (c_int, [_P, _P, _P, c_uint64, _P, c_uint64, _P, c_uint64, _P, POINTER(c_uint64)]),
    "syzsig_report_stats": (c_int, [_P, _P]),
    "syzsig_file_set_dev": (c_int, [_P, _P, _P, _P, c_uint64, _P, _P, _P, c_uint64, c_uint64, c_uint64, _P, _P, _P, _P,
                                    c_uint64, _P, _P]),
    "syzsig_file_set_stats": (c_int, [_P, _P]),
    "syzsig_ingest_exec_output_dev": (c_int, [_P, _P, c_uint64, _P, c_uint64, _P, c_uint64, _P, _P, _P, _P, _P, _P,
                                              _P, _P, _P, POINTER(c_uint64)]),
    "syzsig_triage_records_dev": (c_int, [_P, _P, _PP, _P, c_uint64, _P, c_uint32, _P,
                                          POINTER(BatchStats)]),
    "syzsig_step_send_dev": (c_int, [_P, POINTER(Batch), c_uint64, _P, c_uint32, c_uint32, c_uint64, _P, c_int]),
    "syzsig_step_own_dev": (c_int, [_P, _P, _P, _P, c_uint32, c_uint64, _P, c_uint32, _P, c_int]),
    "syzsig_step_back_dev": (c_int, [_P, POINTER(Batch), c_uint64, _P, c_uint32, c_uint64, _P]),
    "syzsig_step_finish": (c_int, [_P, POINTER(StepStatus)]),
    "syzsig_synth_default": (None, [POINTER(SynthCfg)]),
    "syzsig_synth_traces_host": (c_int, [POINTER(SynthCfg), c_uint64, c_uint64, c_uint32, _P, _P, _P, _P]),
    "syzsig_synth_traces_dev": (c_int, [_P, POINTER(SynthCfg), c_uint64, c_uint64, c_uint32, _P, _P, _P, _P]),
    "syzsig_synth_m0_host": (c_int, [POINTER(SynthCfg), c_uint64, c_uint64, _P, _P]),
    "syzsig_synth_m0_dev": (c_int, [_P, POINTER(SynthCfg), c_uint64, c_uint64, _P, _P]),
    "syzsig_synth_m0_shard_dev": (c_int, [_P, POINTER(SynthCfg), c_uint64, c_uint64, c_uint32, c_uint32, _P, _P,
                                          c_uint64, POINTER(c_uint64)]),
}

_lib = None


def lib():
    """Load libsyzsig.so (raises if it was not built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != SYZSIG_OK:
        msg = lib().syzsig_last_error().decode(errors="replace")
        if rc == SYZSIG_ECORRUPT:
            raise CorruptedSerial(rc, msg)
        raise SyzsigError(rc, msg)
    return rc


def synth_default(**over):
    c = SynthCfg()
    lib().syzsig_synth_default(ctypes.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c
