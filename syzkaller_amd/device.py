"""Batch (device-resident) API of the engine over torch tensors.

torch is plumbing here: it owns HBM buffers and the stream; every computation
runs in libsyzsig's HIP kernels.  All tensors must live on this Device's GPU.
"""
import ctypes

import torch

from . import _lib
from ._lib import Batch, BatchStats, StepStatus, check
from .signal import Signal, engine

__all__ = ["Device", "call_layout"]


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if (t is not None and t.numel()) else 0)


def call_layout(call_len, device=None):
    """Exclusive prefix sum of per-call lengths -> call_start (u64 as int64)."""
    call_len = torch.as_tensor(call_len, device=device)
    start = torch.zeros(call_len.numel(), dtype=torch.int64, device=call_len.device)
    if call_len.numel() > 1:
        start[1:] = torch.cumsum(call_len[:-1].to(torch.int64), 0)
    return start


class Device:
    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise RuntimeError("syzkaller_amd.device needs a ROCm GPU (no CPU fallback)")
        self.index = int(device)
        self.dev = torch.device("cuda", self.index)
        self.eng = engine(self.index)
        self.sync_stream()

    def sync_stream(self):
        """Run library work on torch's current stream of this device.  torch's
        default stream is HIP's null stream (handle 0); the library's own
        stream (selected by 0) is a blocking stream, ordered against the null
        stream both ways, so inputs torch (or a synchronous RCCL collective)
        produced there are complete when a library kernel reads them."""
        self.eng.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)

    @property
    def L(self):
        return self.eng.L

    def _check_dev(self, *ts):
        for t in ts:
            if t is not None and t.device != self.dev:
                raise ValueError(f"tensor on {t.device}, expected {self.dev}")
            if t is not None and not t.is_contiguous():
                raise ValueError("tensors must be contiguous")

    def copy_bw(self, dst, src, nbytes):
        """Device time (ms) of a plain 16-B-per-lane copy of nbytes from src to
        dst (syzsig_copy_bw_dev): the achievable-bandwidth companion of the
        bench's rooflines."""
        self._check_dev(dst, src)
        if nbytes > min(dst.numel() * dst.element_size(), src.numel() * src.element_size()):
            raise ValueError("copy_bw: nbytes exceeds a buffer")
        ms = ctypes.c_double()
        check(self.L.syzsig_copy_bw_dev(self.eng.h, _p(dst), _p(src), int(nbytes), ctypes.byref(ms)))
        return ms.value

    # ---------------------------------------------------------------- sets
    def new_set(self, hint=0):
        return Signal.make(hint, self.eng)

    def deserialize(self, elems, prios):
        self._check_dev(elems, prios)
        assert elems.dtype == torch.int32 or elems.dtype == torch.uint32
        h = ctypes.c_void_p()
        check(self.L.syzsig_deserialize_dev(self.eng.h, _p(elems), _p(prios), elems.numel(), ctypes.byref(h)))
        return Signal(h, self.eng)

    # ---------------------------------------------------------------- K3
    def batch(self, sigs, call_start, call_len, call_prio, new_bits=None, call_new=None, new_pairs=None,
              want_bits=True):
        """A syzsig_batch over device tensors.  new_bits is allocated when
        want_bits (else NULL: not computed); new_pairs (int64) is optional."""
        self._check_dev(sigs, call_start, call_len, call_prio, new_bits, call_new, new_pairs)
        nrec, ncalls = sigs.numel(), call_len.numel()
        if new_bits is None and want_bits:
            new_bits = torch.empty((nrec + 31) // 32, dtype=torch.int32, device=self.dev)
        if call_new is None:
            call_new = torch.empty(ncalls, dtype=torch.uint8, device=self.dev)
        b = Batch(sigs=_p(sigs).value, call_start=_p(call_start).value, call_len=_p(call_len).value,
                  call_prio=_p(call_prio).value, ncalls=ncalls, nrec=nrec, new_bits=_p(new_bits).value,
                  call_new=_p(call_new).value, new_pairs=_p(new_pairs).value,
                  new_pairs_cap=0 if new_pairs is None else new_pairs.numel())
        return b, new_bits, call_new

    def triage(self, max_signal, new_signal, sigs, call_start, call_len, call_prio, new_bits=None, call_new=None,
               new_pairs=None, want_bits=True):
        """checkNewSignal over a whole batch (syz-fuzzer/fuzzer.go:494-511).
        Returns (new_bits int32[ceil(nrec/32)] or None, call_new uint8[ncalls], stats);
        stats["new_pairs"] = number of (call << 32 | elem) DiffRaw entries, the
        first min(that, new_pairs.numel()) of which are written to new_pairs."""
        b, new_bits, call_new = self.batch(sigs, call_start, call_len, call_prio, new_bits, call_new, new_pairs,
                                           want_bits)
        return new_bits, call_new, self.triage_b(max_signal, new_signal, b)

    def triage_b(self, max_signal, new_signal, b):
        """syzsig_triage_batch on a prepared Batch; returns the stats dict."""
        st = BatchStats()
        nh = ctypes.c_void_p(new_signal.handle.value or 0)
        check(self.L.syzsig_triage_batch(self.eng.h, max_signal.handle, ctypes.byref(nh), ctypes.byref(b),
                                         ctypes.byref(st)))
        if nh.value and new_signal.is_nil():
            new_signal._h = nh
        return st.as_dict()

    # ---------------------------------------------------------------- K1+K2
    def _trace_target(self, pcs, target, who):
        """The target word of a trace call and the dtype check that goes with it
        (None: the entry point without a target, int64 PCs under the x86 check)."""
        t = _lib.SYZSIG_TARGET_LINUX_AMD64 if target is None else int(target)
        want = {0: torch.int64, _lib.SYZSIG_TARGET_CHECK_X86: torch.int64, _lib.SYZSIG_TARGET_PC32: torch.int32}.get(t)
        # (any other target word: the library rejects it; no target: today's call, unchecked as ever)
        if target is not None and want is not None and pcs.dtype != want:
            raise ValueError(f"{who}: pcs is {pcs.dtype}, target {t} takes {want}")
        return t

    def edge_derive(self, pcs, call_start, call_len, prog_call, sigs=None, sig_cnt=None, completed=None, target=None):
        """executor write_coverage_signal for every program of a batch.  target
        (syzkaller_amd.targets; None = linux/amd64, today's call): pcs is int32
        for a PC32 target and int64 otherwise."""
        self._check_dev(pcs, call_start, call_len, prog_call, sigs, sig_cnt, completed)
        t = self._trace_target(pcs, target, "edge_derive")
        nprog = prog_call.numel() - 1
        if sigs is None:
            sigs = torch.empty(pcs.numel(), dtype=torch.int32, device=self.dev)
        if sig_cnt is None:
            sig_cnt = torch.empty(call_len.numel(), dtype=torch.int32, device=self.dev)
        if completed is None:
            completed = torch.empty(max(nprog, 0), dtype=torch.int32, device=self.dev)
        if target is None:
            check(self.L.syzsig_edge_derive_dev(self.eng.h, _p(pcs), pcs.numel(), _p(call_start), _p(call_len),
                                                call_len.numel(), _p(prog_call), max(nprog, 0), _p(sigs), _p(sig_cnt),
                                                _p(completed)))
        else:
            check(self.L.syzsig_edge_derive_target_dev(self.eng.h, _p(pcs), pcs.numel(), _p(call_start), _p(call_len),
                                                       call_len.numel(), _p(prog_call), max(nprog, 0), t, _p(sigs),
                                                       _p(sig_cnt), _p(completed)))
        return sigs, sig_cnt, completed

    def edge_cover(self, pcs, call_start, call_len, prog_call, completed, dedup=True, cover=None, cover_cnt=None,
                   target=None):
        """executor.h:514-527 for every call of a batch (syzsig_edge_cover_dev):
        the cover output of the traces edge_derive took, `completed` as it
        returned it.  dedup = flag_dedup_cover.  target as in edge_derive: with
        dedup, target 0 sorts and uniques the u64 PCs before truncating, so its
        output follows the u64 order and may repeat a low word.  Returns (cover
        int32[npc], call c's at cover[call_start[c] : +cover_cnt[c]], cover_cnt
        int32[ncalls])."""
        self._check_dev(pcs, call_start, call_len, prog_call, completed, cover, cover_cnt)
        t = self._trace_target(pcs, target, "edge_cover")
        nprog = prog_call.numel() - 1
        if cover is None:
            cover = torch.empty(pcs.numel(), dtype=torch.int32, device=self.dev)
        if cover_cnt is None:
            cover_cnt = torch.empty(call_len.numel(), dtype=torch.int32, device=self.dev)
        flags = _lib.SYZSIG_COVER_DEDUP if dedup else 0
        if target is None:
            check(self.L.syzsig_edge_cover_dev(self.eng.h, _p(pcs), pcs.numel(), _p(call_start), _p(call_len),
                                               call_len.numel(), _p(prog_call), max(nprog, 0), _p(completed), flags,
                                               _p(cover), _p(cover_cnt)))
        else:
            check(self.L.syzsig_edge_cover_target_dev(self.eng.h, _p(pcs), pcs.numel(), _p(call_start), _p(call_len),
                                                      call_len.numel(), _p(prog_call), max(nprog, 0), _p(completed),
                                                      flags, t, _p(cover), _p(cover_cnt)))
        return cover, cover_cnt

    # ---------------------------------------------------------------- comparison hints
    def _check_cap(self, rc, n):
        """check(rc); a SYZSIG_ERANGE carries the needed total as .needed"""
        try:
            check(rc)
        except _lib.SyzsigError as e:
            e.needed = int(n.value)
            raise

    def exec_comps(self, comps, call_start, call_len, out_start, out=None, out_words=None, comps_cnt=None):
        """executor.h:576-593 with flag_collect_comps for every call of a batch
        (syzsig_exec_comps_dev).  comps: int64[ncmp, 4] records (type, arg1,
        arg2, pc); out_start = the executor's output_data address.  Returns (out
        int32[5 * ncmp], call c's words at out[5 * call_start[c] : +out_words[c]],
        out_words int32[ncalls], comps_cnt int32[ncalls] = the records' comps_size)."""
        self._check_dev(comps, call_start, call_len, out, out_words, comps_cnt)
        if comps.numel() % 4:
            raise ValueError("comps holds records of four words")
        ncmp, ncalls = comps.numel() // 4, call_len.numel()
        if out is None:
            out = torch.empty(5 * ncmp, dtype=torch.int32, device=self.dev)
        if out.numel() < 5 * ncmp:
            raise ValueError("out needs 5 words per record")
        if out_words is None:
            out_words = torch.empty(ncalls, dtype=torch.int32, device=self.dev)
        if comps_cnt is None:
            comps_cnt = torch.empty(ncalls, dtype=torch.int32, device=self.dev)
        check(self.L.syzsig_exec_comps_dev(self.eng.h, _p(comps), ncmp, _p(call_start), _p(call_len), ncalls,
                                           int(out_start), _p(out), _p(out_words), _p(comps_cnt)))
        return out, out_words, comps_cnt

    def comp_map(self, words, comps_start, comps_cnt, comps_end=None, pairs=None):
        """ipc.go:420-465 per call (syzsig_comp_map_dev): comps_cnt[c] records
        from words[comps_start[c]] on, inside words[:comps_end[c]] (None: the
        whole buffer).  Returns (status int32[ncalls], map_off int64[ncalls + 1],
        pairs int64[n, 2]): call c's CompMap as its distinct (key, value) pairs,
        sorted, at pairs[map_off[c]:map_off[c + 1]].  A given `pairs` that is too
        small raises SyzsigError(SYZSIG_ERANGE) with the needed pairs in .needed."""
        self._check_dev(words, comps_start, comps_cnt, comps_end, pairs)
        ncalls = comps_cnt.numel()
        if comps_start.numel() != ncalls or (comps_end is not None and comps_end.numel() != ncalls):
            raise ValueError("comps_start / comps_end need one entry per call")
        status = torch.empty(ncalls, dtype=torch.int32, device=self.dev)
        off = torch.empty(ncalls + 1, dtype=torch.int64, device=self.dev)
        n = ctypes.c_uint64()
        if pairs is None:  # a record adds two pairs at most
            pairs = torch.empty((2 * int(comps_cnt.to(torch.int64).sum().item()), 2), dtype=torch.int64,
                                device=self.dev)
        self._check_cap(self.L.syzsig_comp_map_dev(self.eng.h, _p(words), words.numel(), _p(comps_start),
                                                   _p(comps_cnt), _p(comps_end), ncalls, _p(status), _p(off),
                                                   _p(pairs), pairs.numel() // 2, ctypes.byref(n)), n)
        return status, off, pairs.view(-1, 2)[: n.value]

    def shrink_expand(self, map_off, pairs, calls, values, special_ints=(), rep=None):
        """prog/hints.go:164-218 for queries (calls[q], values[q]) against the
        maps of comp_map (syzsig_shrink_expand_dev).  calls int32[nq], values
        int64[nq]; special_ints: prog/rand.go's list.  Returns (rep_off
        int64[nq + 1], rep int64[total]): query q's distinct replacers, sorted
        as unsigned, at rep[rep_off[q]:rep_off[q + 1]]."""
        self._check_dev(map_off, pairs, calls, values, rep)
        nq = calls.numel()
        if values.numel() != nq:
            raise ValueError("calls and values need one entry per query")
        sp = [int(x) & 0xFFFFFFFFFFFFFFFF for x in special_ints]
        csp = (ctypes.c_uint64 * max(len(sp), 1))(*sp)
        off = torch.empty(nq + 1, dtype=torch.int64, device=self.dev)
        n = ctypes.c_uint64()

        def run(r):
            return self.L.syzsig_shrink_expand_dev(self.eng.h, _p(map_off), _p(pairs), map_off.numel() - 1,
                                                   pairs.numel() // 2, _p(calls), _p(values), nq, csp, len(sp),
                                                   _p(off), _p(r), 0 if r is None else r.numel(), ctypes.byref(n))
        rc = run(rep)
        if rep is None and rc == _lib.SYZSIG_ERANGE:
            rep = torch.empty(n.value, dtype=torch.int64, device=self.dev)
            rc = run(rep)
        self._check_cap(rc, n)
        if rep is None:
            rep = torch.empty(0, dtype=torch.int64, device=self.dev)
        return off, rep[: n.value]

    def hint_mutants(self, map_off, pairs, arg_call, arg_kind, arg_val, arg_off, data, special_ints=(), out=None):
        """prog/hints.go:105-132 for a batch of args against the maps of
        comp_map (syzsig_hint_mutants_dev).  arg_call int32[narg], arg_kind
        uint8[narg] (0 = ConstArg, 1 = DataArg), arg_val int64[narg], arg_off
        int64[narg + 1] into data uint8[nbytes].  Returns (mut_off
        int64[narg + 1], at int32[total], nb uint8[total], rep int64[total]):
        arg a's mutants at [mut_off[a], mut_off[a + 1]), windows ascending,
        replacers ascending as unsigned.  out = (at, nb, rep) tensors to write
        into; too small raises SyzsigError(SYZSIG_ERANGE) with .needed."""
        at, nb, rep = out if out is not None else (None, None, None)
        self._check_dev(map_off, pairs, arg_call, arg_kind, arg_val, arg_off, data, at, nb, rep)
        narg = arg_call.numel()
        if arg_kind.numel() != narg or arg_val.numel() != narg or arg_off.numel() != narg + 1:
            raise ValueError("arg_call, arg_kind, arg_val need one entry per arg, arg_off one more")
        if arg_kind.dtype != torch.uint8 or data.dtype != torch.uint8:
            raise ValueError("arg_kind and data are uint8")
        sp = [int(x) & 0xFFFFFFFFFFFFFFFF for x in special_ints]
        csp = (ctypes.c_uint64 * max(len(sp), 1))(*sp)
        off = torch.empty(narg + 1, dtype=torch.int64, device=self.dev)
        n = ctypes.c_uint64()

        def run(at, nb, rep):
            cap = 0 if at is None else min(at.numel(), nb.numel(), rep.numel())
            return self.L.syzsig_hint_mutants_dev(self.eng.h, _p(map_off), _p(pairs), map_off.numel() - 1,
                                                  pairs.numel() // 2, _p(arg_call), _p(arg_kind), _p(arg_val),
                                                  _p(arg_off), _p(data), narg, data.numel(), csp, len(sp), _p(off),
                                                  _p(at), _p(nb), _p(rep), cap, ctypes.byref(n))
        rc = run(at, nb, rep)
        if out is None:
            if rc == _lib.SYZSIG_ERANGE:
                at = torch.empty(n.value, dtype=torch.int32, device=self.dev)
                nb = torch.empty(n.value, dtype=torch.uint8, device=self.dev)
                rep = torch.empty(n.value, dtype=torch.int64, device=self.dev)
                rc = run(at, nb, rep)
            elif rc == _lib.SYZSIG_OK:
                at = torch.empty(0, dtype=torch.int32, device=self.dev)
                nb = torch.empty(0, dtype=torch.uint8, device=self.dev)
                rep = torch.empty(0, dtype=torch.int64, device=self.dev)
        self._check_cap(rc, n)
        return off, at[: n.value], nb[: n.value], rep[: n.value]

    def hint_mutants_stats(self):
        """(args resolved in LDS, args that took the fallback, windows
        examined, accepted candidates before the dedup) of the last
        hint_mutants call (syzsig_hint_mutants_stats)."""
        out = (ctypes.c_uint64 * 4)()
        check(self.L.syzsig_hint_mutants_stats(self.eng.h, out))
        return tuple(int(x) for x in out)

    # ---------------------------------------------------------------- call priorities and the choice table
    def calculate_priorities(self, corpus_ids, ncalls, static=None, split=0, out=None):
        """target.CalculatePriorities(corpus), prog/prio.go:27-36, over the
        calls' ids of every corpus program: float32[N, N] on the device
        (syzkaller_amd.prio.calculate_priorities)."""
        from . import prio
        return prio.calculate_priorities(self, corpus_ids, ncalls, static, split, out)

    def prio_stats(self):
        """(rows counted whole, rows split, slices, pair increments) of the
        last calculate_priorities (syzsig_prio_stats)."""
        from . import prio
        return prio.prio_stats(self)

    def static_finish(self, mat):
        """The tail of calcStaticPriorities, prog/prio.go:118-129
        (syzkaller_amd.prio.static_finish)."""
        from . import prio
        return prio.static_finish(self, mat)

    def choice_table(self, prios, enabled, ncalls):
        """target.BuildChoiceTable(prios, enabled), prog/prio.go:198-228: a
        syzkaller_amd.prio.ChoiceTable."""
        from . import prio
        return prio.ChoiceTable.build(self, prios, enabled, ncalls)

    # ---------------------------------------------------------------- the manager's coverage pages
    def report_corpus(self, inputs, calls=()):
        """mgr.corpus as the report kernels read it (syzkaller_amd.report.Corpus):
        inputs = {sig: (call name, cover u32[])}."""
        from . import report
        return report.Corpus(self, inputs, calls)

    def syscall_info(self, corpus):
        """collectSyscallInfo, syz-manager/html.go:135-149: {call: (count,
        len(cov))} (syzkaller_amd.report.syscall_info)."""
        from . import report
        return report.syscall_info(corpus)

    def cover_for(self, corpus, call=None, input=None):
        """httpCover's cov, syz-manager/html.go:202-212, as a Cover
        (syzkaller_amd.report.cover_for)."""
        from . import report
        return report.cover_for(corpus, call, input)

    def report_pcs(self, pcs, base, arch):
        """RestorePC + previousInstructionPC per PC, in input order and sorted
        (syzkaller_amd.report.report_pcs)."""
        from . import report
        return report.report_pcs(self, pcs, base, arch)

    def uncovered_pcs(self, sym_start, sym_end, all_cover, pcs):
        """uncoveredPcsInFuncs, syz-manager/cover.go:254-304, for pcs in the
        order given (syzkaller_amd.report.uncovered_pcs)."""
        from . import report
        return report.uncovered_pcs(self, sym_start, sym_end, all_cover, pcs)

    def report_stats(self):
        """The paths of the last report call (syzsig_report_stats)."""
        from . import report
        return report.report_stats(self)

    def report_frames(self, covered, uncovered, files=(), funcs=()):
        """Symbolized frames as the file_set kernels read them
        (syzkaller_amd.report.Frames): File and Func interned to dense ids."""
        from . import report
        return report.Frames(self, covered, uncovered, files, funcs)

    def file_set(self, frames, nlines=None, cap=None):
        """fileSet and the line walk's Coverage, syz-manager/cover.go:129-193, as
        CSR over the files (syzkaller_amd.report.file_set)."""
        from . import report
        return report.file_set(frames, nlines, cap)

    def file_set_stats(self):
        """The paths of the last file_set call (syzsig_file_set_stats)."""
        from . import report
        return report.file_set_stats(self)

    # ---------------------------------------------------------------- executor output ingest
    def ingest_exec_output(self, out, prog_off, prog_call, call_any, call_num=None, want_cover=False):
        """pkg/ipc/ipc.go:328-468 readOutCoverage over a batch of executor output
        regions (program p's at out[prog_off[p]:prog_off[p+1]]).  Returns a dict of
        device tensors call_start (int64), call_len (int32), call_prio (uint8),
        call_errno (int32), prog_status (int32), cover_start/cover_len (if
        want_cover), and n_failed.  call_start/len index `out`, so
        triage(max, new, out, call_start, call_len, call_prio) runs checkNewSignal
        on the batch without copying the signal."""
        self._check_dev(out, prog_off, prog_call, call_any, call_num)
        nprog, ncalls = prog_off.numel() - 1, call_any.numel()
        if prog_call.numel() != prog_off.numel():
            raise ValueError("prog_call and prog_off need nprog + 1 entries")
        if call_num is not None and call_num.numel() != ncalls:
            raise ValueError("call_num needs one entry per call")
        r = {"call_start": torch.empty(ncalls, dtype=torch.int64, device=self.dev),
             "call_len": torch.empty(ncalls, dtype=torch.int32, device=self.dev),
             "call_prio": torch.empty(ncalls, dtype=torch.uint8, device=self.dev),
             "call_errno": torch.empty(ncalls, dtype=torch.int32, device=self.dev),
             "prog_status": torch.empty(max(nprog, 0), dtype=torch.int32, device=self.dev)}
        if want_cover:
            r["cover_start"] = torch.empty(ncalls, dtype=torch.int64, device=self.dev)
            r["cover_len"] = torch.empty(ncalls, dtype=torch.int32, device=self.dev)
        nf = ctypes.c_uint64()
        check(self.L.syzsig_ingest_exec_output_dev(
            self.eng.h, _p(out), out.numel(), _p(prog_off), max(nprog, 0), _p(prog_call), ncalls, _p(call_num),
            _p(call_any), _p(r["call_start"]), _p(r["call_len"]), _p(r["call_prio"]), _p(r["call_errno"]),
            _p(r.get("cover_start")), _p(r.get("cover_len")), _p(r["prog_status"]), ctypes.byref(nf)))
        r["n_failed"] = int(nf.value)
        return r

    # ---------------------------------------------------------------- triageInput re-runs
    def triage_runs(self, item_off, elems, prios, item_flags, runs, run_off, run_sigs, run_prio, run_errno,
                    run_exec, cover=None):
        """syz-fuzzer/proc.go:107-140 over a batch of triage items (see
        include/syzsig.h syzsig_triage_runs_dev).  Returns (item_keep, elem_keep)
        as uint8 device tensors.  With cover = (cover, run_cover_start,
        run_cover_len) -- the runs' cover lists, see triage_cover -- it also
        returns the items' inputCover (proc.go:139) as a list: entry i is the
        slice of sorted PCs for RPCInput.Cover (:173) of a kept item, None for
        a dropped one."""
        self._check_dev(item_off, elems, prios, item_flags, run_off, run_sigs, run_prio, run_errno, run_exec)
        nitems = item_off.numel() - 1
        if run_off.numel() != nitems * runs + 1 and nitems > 0:
            raise ValueError("run_off needs nitems * runs + 1 entries")
        item_keep = torch.empty(max(nitems, 0), dtype=torch.uint8, device=self.dev)
        elem_keep = torch.empty(elems.numel(), dtype=torch.uint8, device=self.dev)
        check(self.L.syzsig_triage_runs_dev(self.eng.h, _p(item_off), max(nitems, 0), _p(elems), _p(prios),
                                            _p(item_flags), int(runs), _p(run_off), _p(run_sigs), _p(run_prio),
                                            _p(run_errno), _p(run_exec), _p(item_keep), _p(elem_keep)))
        if cover is None:
            return item_keep, elem_keep
        off, item_cover = self.triage_cover(item_flags, item_keep, runs, run_off, run_errno, run_exec, *cover)
        o, k = off.cpu().tolist(), item_keep.cpu().tolist()
        return item_keep, elem_keep, [item_cover[o[i]:o[i + 1]] if k[i] else None for i in range(max(nitems, 0))]

    def triage_cover(self, item_flags, item_keep, runs, run_off, run_errno, run_exec, cover, run_cover_start,
                     run_cover_len, item_cover=None):
        """triageInput's inputCover (proc.go:139, :173) per item, over the layout
        of triage_runs (syzsig_triage_cover_dev): run r's cover list is
        cover[run_cover_start[r] : +run_cover_len[r]] (int64 / int32 tensors of
        nitems * runs entries; `cover` is an edge_cover output or the executor
        regions the ingest indexed).  Returns (item_cover_off int64[nitems + 1],
        item_cover int32[total]): item i's PCs, sorted, at
        item_cover[off[i]:off[i + 1]], empty for a dropped item.  A given
        item_cover that is too small raises SyzsigError(SYZSIG_ERANGE)."""
        self._check_dev(item_flags, item_keep, run_off, run_errno, run_exec, cover, run_cover_start, run_cover_len,
                        item_cover)
        nitems = item_keep.numel()
        if run_cover_start.numel() != nitems * runs or run_cover_len.numel() != nitems * runs:
            raise ValueError("run_cover_start / run_cover_len need nitems * runs entries")
        if nitems and runs and run_off.numel() != nitems * runs + 1:
            raise ValueError("run_off needs nitems * runs + 1 entries")
        if item_cover is None:  # the union is no longer than the lists together
            item_cover = torch.empty(int(run_cover_len.to(torch.int64).sum().item()), dtype=torch.int32,
                                     device=self.dev)
        off = torch.empty(nitems + 1, dtype=torch.int64, device=self.dev)
        n = ctypes.c_uint64()
        check(self.L.syzsig_triage_cover_dev(self.eng.h, nitems, int(runs), _p(item_flags), _p(item_keep), _p(run_off),
                                             _p(run_errno), _p(run_exec), _p(cover), cover.numel(),
                                             _p(run_cover_start), _p(run_cover_len), _p(off), _p(item_cover),
                                             item_cover.numel(), ctypes.byref(n)))
        return off, item_cover[: n.value]

    # ---------------------------------------------------------------- triage items
    def triage_items(self, sigs, call_start, call_len, call_prio, call_new, corpus_signal=None, caps=None):
        """proc.go:232-245 and :107-111 over a batch (syzsig_triage_items_dev):
        the calls triage flagged in call_new become items, in call order, each
        with its inputSignal = FromRaw(call's signal, prio) and its newSignal =
        corpusSignal.Diff(inputSignal) (corpus_signal: a Signal, None = nil).
        Returns a dict of device tensors: item_call int32[n], item_prio int8[n],
        input_off int64[n + 1], input_elems int32[] (RPCInput.Signal: item i's
        elements, ascending, all with item_prio[i]), and item_off int64[n + 1],
        elems int32[], prios int8[] -- the CSR triage_runs reads.  caps =
        (items, input entries, new entries) sizes the outputs; None starts from
        the flagged calls' records being unknown: one call to learn the totals,
        one to write.  Given caps that are too small raise
        SyzsigError(SYZSIG_ERANGE) with the three totals in .needed."""
        self._check_dev(sigs, call_start, call_len, call_prio, call_new)
        ncalls = call_len.numel()
        if call_start.numel() != ncalls or call_prio.numel() != ncalls or call_new.numel() != ncalls:
            raise ValueError("call_start / call_len / call_prio / call_new need one entry per call")
        cs = corpus_signal.handle if corpus_signal is not None else ctypes.c_void_p(0)
        n = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()]

        def run(ci, cn, cw):
            r = {"item_call": torch.empty(ci, dtype=torch.int32, device=self.dev),
                 "item_prio": torch.empty(ci, dtype=torch.int8, device=self.dev),
                 "input_off": torch.empty(ci + 1, dtype=torch.int64, device=self.dev),
                 "input_elems": torch.empty(cn, dtype=torch.int32, device=self.dev),
                 "item_off": torch.empty(ci + 1, dtype=torch.int64, device=self.dev),
                 "elems": torch.empty(cw, dtype=torch.int32, device=self.dev),
                 "prios": torch.empty(cw, dtype=torch.int8, device=self.dev)}
            rc = self.L.syzsig_triage_items_dev(
                self.eng.h, _p(sigs), sigs.numel(), _p(call_start), _p(call_len), _p(call_prio), ncalls, _p(call_new),
                cs, _p(r["item_call"]), _p(r["item_prio"]), ci, _p(r["input_off"]), _p(r["input_elems"]), cn,
                _p(r["item_off"]), _p(r["elems"]), _p(r["prios"]), cw, ctypes.byref(n[0]), ctypes.byref(n[1]),
                ctypes.byref(n[2]))
            return rc, r

        rc, r = run(*(caps if caps is not None else (0, 0, 0)))
        if caps is None and rc == _lib.SYZSIG_ERANGE and n[0].value:
            rc, r = run(n[0].value, n[1].value, n[2].value)
        try:
            check(rc)
        except _lib.SyzsigError as e:
            e.needed = tuple(int(x.value) for x in n)
            raise
        ni, nin, nnew = (int(x.value) for x in n)
        return {"item_call": r["item_call"][:ni], "item_prio": r["item_prio"][:ni], "input_off": r["input_off"][:ni + 1],
                "input_elems": r["input_elems"][:nin], "item_off": r["item_off"][:ni + 1], "elems": r["elems"][:nnew],
                "prios": r["prios"][:nnew]}

    def triage_items_stats(self):
        """(items, items past SYZSIG_ITEMS_TILE, rank-merge passes, corpusSignal
        probes) of the last triage_items call (syzsig_triage_items_stats)."""
        out = (ctypes.c_uint64 * 4)()
        check(self.L.syzsig_triage_items_stats(self.eng.h, out))
        return tuple(int(x) for x in out)

    def corpus_add_inputs(self, input_off, input_elems, item_prio, corpus_signal, max_signal, item_keep=None):
        """addInputToCorpus (fuzzer.go:446-460) over the items triageInput kept
        (syzsig_corpus_add_inputs_dev): every item with item_keep != 0 (None =
        all) and a non-empty inputSignal is max-merged into corpus_signal and
        max_signal (Signal objects; a nil one is allocated when something is
        merged).  input_off / input_elems / item_prio as triage_items returned them."""
        self._check_dev(input_off, input_elems, item_prio, item_keep)
        nitems = item_prio.numel()
        if input_off.numel() != nitems + 1 or (item_keep is not None and item_keep.numel() != nitems):
            raise ValueError("input_off needs nitems + 1 entries, item_keep nitems")
        ch = ctypes.c_void_p(corpus_signal.handle.value or 0)
        mh = ctypes.c_void_p(max_signal.handle.value or 0)
        check(self.L.syzsig_corpus_add_inputs_dev(self.eng.h, _p(input_off), _p(input_elems), input_elems.numel(),
                                                  _p(item_prio), nitems, _p(item_keep), ctypes.byref(ch),
                                                  ctypes.byref(mh)))
        if ch.value and corpus_signal.is_nil():
            corpus_signal._h = ch
        if mh.value and max_signal.is_nil():
            max_signal._h = mh

    def poll_res(self, seg_off, seg_kind, elems, prios, corpus_signal, max_signal):
        """The reply to a fuzzer's poll (fuzzer.go:344-350) over a batch of
        Serials (syzsig_fuzzer_poll_res_dev): segment s is elems / prios
        [seg_off[s] : seg_off[s + 1]] (seg_off int64[nseg + 1]) and seg_kind[s]
        (uint8) is SYZSIG_SEG_MAXSIGNAL (addMaxSignal, :468-475: merged into
        max_signal) or SYZSIG_SEG_INPUT (addInputFromAnotherFuzzer, :433-460:
        merged into corpus_signal and max_signal).  Each segment is
        deserialized first: the last entry of an element gives its prio.
        corpus_signal / max_signal are Signal objects; a nil one is allocated
        when a non-empty segment reaches it."""
        self._check_dev(seg_off, seg_kind, elems, prios)
        nseg = seg_kind.numel()
        if seg_off.numel() != nseg + 1 or prios.numel() != elems.numel():
            raise ValueError("seg_off needs nseg + 1 entries, prios one per element")
        ch = ctypes.c_void_p(corpus_signal.handle.value or 0)
        mh = ctypes.c_void_p(max_signal.handle.value or 0)
        check(self.L.syzsig_fuzzer_poll_res_dev(self.eng.h, _p(seg_off), _p(seg_kind), nseg, _p(elems), _p(prios),
                                                elems.numel(), ctypes.byref(ch), ctypes.byref(mh)))
        if ch.value and corpus_signal.is_nil():
            corpus_signal._h = ch
        if mh.value and max_signal.is_nil():
            max_signal._h = mh

    def poll_res_stats(self):
        """(segments resolved in LDS, segments resolved through a scratch
        table, entries that lost to a later entry of their element, scratch
        bytes) of the last poll_res call (syzsig_poll_res_stats)."""
        out = (ctypes.c_uint64 * 4)()
        check(self.L.syzsig_poll_res_stats(self.eng.h, out))
        return tuple(int(x) for x in out)

    def minimize_pred(self, item_off, elems, prios, item_flags, attempts, run_off, run_sigs, run_prio, run_errno,
                      run_exec):
        """triageInput's minimize predicate (proc.go:141-160) per item; uint8 tensor."""
        self._check_dev(item_off, elems, prios, item_flags, run_off, run_sigs, run_prio, run_errno, run_exec)
        nitems = item_off.numel() - 1
        if run_off.numel() != nitems * attempts + 1 and nitems > 0:
            raise ValueError("run_off needs nitems * attempts + 1 entries")
        pred = torch.empty(max(nitems, 0), dtype=torch.uint8, device=self.dev)
        check(self.L.syzsig_minimize_pred_dev(self.eng.h, _p(item_off), max(nitems, 0), _p(elems), _p(prios),
                                              _p(item_flags), int(attempts), _p(run_off), _p(run_sigs),
                                              _p(run_prio), _p(run_errno), _p(run_exec), _p(pred)))
        return pred

    # ---------------------------------------------------------------- K5
    def minimize(self, ctx_off, elems, prios, hint_distinct=0):
        self._check_dev(ctx_off, elems, prios)
        n = ctx_off.numel() - 1
        keep = torch.empty(max(n, 0), dtype=torch.uint8, device=self.dev)
        cnt = ctypes.c_uint64()
        check(self.L.syzsig_minimize_dev(self.eng.h, _p(ctx_off), _p(elems), _p(prios), max(n, 0),
                                         int(hint_distinct), _p(keep), ctypes.byref(cnt)))
        return keep, int(cnt.value)

    def minimize_shard(self, ctx_off, elems, prios, nshards, shard, hint_distinct=0):
        """Minimize over the elements this shard owns (owner_of); OR the keep
        arrays of all shards for the corpus result (see dist.sharded_minimize)."""
        self._check_dev(ctx_off, elems, prios)
        n = ctx_off.numel() - 1
        keep = torch.empty(max(n, 0), dtype=torch.uint8, device=self.dev)
        cnt = ctypes.c_uint64()
        check(self.L.syzsig_minimize_shard_dev(self.eng.h, _p(ctx_off), _p(elems), _p(prios), max(n, 0),
                                               int(nshards), int(shard), int(hint_distinct), _p(keep),
                                               ctypes.byref(cnt)))
        return keep, int(cnt.value)

    def minimize_split(self, ctx_off, elems, prios, nparts, part, nshards, hint_distinct=0, send=None):
        """Data-split Minimize, source side (syzsig_minimize_split_dev): this
        part's contexts aggregated, one winner record per distinct element,
        grouped by owner.  -> (send int64[sum(counts)], counts)."""
        self._check_dev(ctx_off, elems, prios, send)
        n = ctx_off.numel() - 1
        if send is None:
            send = torch.empty(max(elems.numel(), 1), dtype=torch.int64, device=self.dev)
        counts = (ctypes.c_uint64 * nshards)()
        check(self.L.syzsig_minimize_split_dev(self.eng.h, _p(ctx_off), _p(elems), _p(prios), max(n, 0), int(nparts),
                                               int(part), int(nshards), int(hint_distinct), _p(send), send.numel(),
                                               counts))
        counts = [int(c) for c in counts]
        return send[: sum(counts)], counts

    def minimize_resolve(self, ctx_off, recs):
        """Data-split Minimize, owner side (syzsig_minimize_resolve_dev): the
        winner records sent to this owner -> keep uint8[nctx]."""
        self._check_dev(ctx_off, recs)
        n = ctx_off.numel() - 1
        keep = torch.empty(max(n, 0), dtype=torch.uint8, device=self.dev)
        cnt = ctypes.c_uint64()
        check(self.L.syzsig_minimize_resolve_dev(self.eng.h, _p(ctx_off), max(n, 0), _p(recs), recs.numel(),
                                                 _p(keep), ctypes.byref(cnt)))
        return keep, int(cnt.value)

    # ---------------------------------------------------------------- sharding (records mode: the owner side)
    def triage_records(self, shard, new_signal, recs, levels, new_flags):
        self._check_dev(recs, new_flags)
        lv = (ctypes.c_int8 * len(levels))(*levels)
        st = BatchStats()
        nh = ctypes.c_void_p(new_signal.handle.value or 0)
        check(self.L.syzsig_triage_records_dev(self.eng.h, shard.handle, ctypes.byref(nh), _p(recs), recs.numel(),
                                               lv, len(levels), _p(new_flags), ctypes.byref(st)))
        if nh.value and new_signal.is_nil():
            new_signal._h = nh
        return st.as_dict()

    # ---------------------------------------------------------------- the stream-ordered sharded step
    def step_send(self, b, serial_base, levels, nshards, cap, send, exact=False):
        """Source side (syzsig_step_send_dev): b's staircase records into
        nshards buckets of cap + 1 words (send, int64).  Enqueues only."""
        self._check_dev(send)
        if send.numel() < nshards * (cap + 1):
            raise ValueError("send needs nshards * (cap + 1) words")
        lv = (ctypes.c_int8 * len(levels))(*levels)
        check(self.L.syzsig_step_send_dev(self.eng.h, ctypes.byref(b), int(serial_base), lv, len(levels), int(nshards),
                                          int(cap), _p(send), int(bool(exact))))

    def step_own(self, shard, new_signal, recv, nshards, cap, levels, flags, exact=False):
        """Owner side (syzsig_step_own_dev): the received buckets against this
        owner's shard; flags (uint8, nshards * (cap + 1)).  Enqueues only
        (exact: the per-record path, synchronous)."""
        self._check_dev(recv, flags)
        if recv.numel() < nshards * (cap + 1) or flags.numel() < nshards * (cap + 1):
            raise ValueError("recv / flags need nshards * (cap + 1) entries")
        if new_signal.is_nil():
            raise ValueError("step_own needs a non-nil newSignal shard (make(Signal, hint))")
        lv = (ctypes.c_int8 * len(levels))(*levels)
        check(self.L.syzsig_step_own_dev(self.eng.h, shard.handle, new_signal.handle, _p(recv), int(nshards),
                                         int(cap), lv, len(levels), _p(flags), int(bool(exact))))

    def step_back(self, b, serial_base, send, nshards, cap, back):
        """Source side again (syzsig_step_back_dev): the owners' flags -> b's
        call_new / new_pairs (/ new_bits).  Enqueues only unless bits are wanted."""
        self._check_dev(send, back)
        check(self.L.syzsig_step_back_dev(self.eng.h, ctypes.byref(b), int(serial_base), _p(send), int(nshards),
                                          int(cap), _p(back)))

    def step_finish(self):
        """The step's one host synchronisation -> the status dict."""
        st = StepStatus()
        check(self.L.syzsig_step_finish(self.eng.h, ctypes.byref(st)))
        return st.as_dict()

    # ---------------------------------------------------------------- synthetic data
    def synth_traces(self, cfg, prog_base, nprog, calls_per_prog, call_len):
        """-> (pcs int64[sum], call_start int64[n], call_prio uint8[n]) for nprog programs."""
        call_len = call_len.to(self.dev, torch.int32).contiguous()
        call_start = call_layout(call_len)
        total = int(call_len.to(torch.int64).sum().item())
        pcs = torch.empty(total, dtype=torch.int64, device=self.dev)
        prio = torch.empty(call_len.numel(), dtype=torch.uint8, device=self.dev)
        check(self.L.syzsig_synth_traces_dev(self.eng.h, ctypes.byref(cfg), int(prog_base), int(nprog),
                                             int(calls_per_prog), _p(call_start), _p(call_len), _p(pcs), _p(prio)))
        return pcs, call_start, call_len, prio

    def synth_m0_shard(self, cfg, known_sys, n, nshards, shard):
        """This shard's elements of synth_m0(cfg, known_sys, n), in index order
        (owner_of), without materialising the whole M0."""
        cap = n // nshards + 8 * int(n ** 0.5) + 1024 if nshards > 1 else n
        for _ in range(2):
            elems = torch.empty(max(cap, 1), dtype=torch.int32, device=self.dev)
            prios = torch.empty(max(cap, 1), dtype=torch.int8, device=self.dev)
            got = ctypes.c_uint64()
            rc = self.L.syzsig_synth_m0_shard_dev(self.eng.h, ctypes.byref(cfg), int(known_sys), int(n), int(nshards),
                                                  int(shard), _p(elems), _p(prios), cap, ctypes.byref(got))
            if rc == _lib.SYZSIG_ERANGE and got.value > cap:
                cap = got.value
                continue
            check(rc)
            return elems[: got.value], prios[: got.value]
        raise RuntimeError("synth_m0_shard: size changed between calls")

    def synth_m0(self, cfg, known_sys, n):
        elems = torch.empty(n, dtype=torch.int32, device=self.dev)
        prios = torch.empty(n, dtype=torch.int8, device=self.dev)
        check(self.L.syzsig_synth_m0_dev(self.eng.h, ctypes.byref(cfg), int(known_sys), int(n), _p(elems),
                                         _p(prios)))
        return elems, prios
