"""The calls of a batch of programs from their text, on device: the step between
db.open_db's (data, off) and prio.calculate_priorities' (off, ids).

In the reference this is the one per-program host loop left on the manager's
start-up and Connect paths: loadCorpus (syz-manager/manager.go:209-240) runs
Deserialize on every record to split the corpus into broken, "contains a
disabled syscall" and candidates, and Connect (:888-896) runs it on every input
again only to hand p.Calls[*].Meta.ID to CalculatePriorities.  Neither needs the
arguments; both need only the head of each line (prog/encoding.go:159-180 over
the parser of :740-828).  prog.CallSet (:836-869) is the reference's own "very
conservative" reader of the same thing.

What this is not: it does not parse arguments, it does not run validate(), and
it does not run SanitizeCall.  A program whose heads are well-formed but whose
arguments are broken is reported OK here.  The caller keeps Deserialize for
programs that arrive from outside (NewInput, the hub).

Everything is computed by libsyzsig's kernels (csrc/calls.hip); torch owns the
buffers."""
import ctypes

import numpy as np
import torch

from . import _lib, hashing
from ._lib import check

__all__ = ["CallTable", "prog_calls", "call_set", "load_corpus", "stats", "STATUS", "DESERIALIZE", "CALLSET", "WINDOW",
           "TILE", "SORT_TILE", "MAX_LINE"]

DESERIALIZE, CALLSET = _lib.SYZSIG_PROGTEXT_DESERIALIZE, _lib.SYZSIG_PROGTEXT_CALLSET
WINDOW, TILE, SORT_TILE = _lib.SYZSIG_PROGTEXT_WINDOW, _lib.SYZSIG_PROGTEXT_TILE, _lib.SYZSIG_PROGTEXT_SORT_TILE
MAX_LINE = _lib.SYZSIG_PROGTEXT_MAX_LINE
STATUS = {_lib.SYZSIG_PT_OK: "ok", _lib.SYZSIG_PT_LINE_TOO_LONG: "line_too_long", _lib.SYZSIG_PT_BAD_IDENT: "bad_ident",
          _lib.SYZSIG_PT_BAD_HEAD: "bad_head", _lib.SYZSIG_PT_UNKNOWN_CALL: "unknown_call",
          _lib.SYZSIG_PT_NO_BRACKET: "no_bracket", _lib.SYZSIG_PT_EMPTY_NAME: "empty_name",
          _lib.SYZSIG_PT_NO_CALLS: "no_calls"}


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if (t is not None and t.numel()) else 0)


class CallTable:
    """The target's call names as a device object (syzsig_calltab): names[i] is
    the name of call id i (target.Syscalls[i].Name).  Built once per target.
    Empty or duplicate names raise SyzsigError(SYZSIG_EINVAL)."""

    def __init__(self, dev, names):
        names = [bytes(n, "ascii") if isinstance(n, str) else bytes(n) for n in names]
        blob = b"".join(names)
        off = np.zeros(len(names) + 1, np.uint64)
        np.cumsum([len(n) for n in names], out=off[1:])
        buf = ctypes.create_string_buffer(blob, max(len(blob), 1))
        h = ctypes.c_void_p()
        self.dev, self.h, self.n = dev, None, len(names)
        check(dev.L.syzsig_calltab_make(dev.eng.h, buf, off.ctypes.data, len(names), ctypes.byref(h)))
        self.h = h

    def __len__(self):
        return int(self.dev.L.syzsig_calltab_len(self.h)) if self.h else 0

    def free(self):
        if self.h:
            self.dev.L.syzsig_calltab_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _vals(dev, vals):
    """(data uint8[nbytes], off int64[n + 1]) on the device, from such a pair
    (db.open_db's vals) or from a list of byte strings."""
    if isinstance(vals, tuple) and len(vals) == 2 and (torch.is_tensor(vals[1]) or isinstance(vals[1], np.ndarray)):
        data = hashing._bytes_tensor(dev, vals[0])
        off = torch.as_tensor(vals[1]).to(torch.int64).to(dev.dev).contiguous()
    else:
        progs = [bytes(p) for p in vals]
        off_np = np.zeros(len(progs) + 1, np.int64)
        np.cumsum([len(p) for p in progs], out=off_np[1:])
        data = hashing._bytes_tensor(dev, b"".join(progs))
        off = torch.from_numpy(off_np).to(dev.dev)
    if data.numel() and data.data_ptr() % 16:
        data = data.clone()  # (a view into a larger buffer: the kernels load 16 aligned bytes per lane)
    return data, off


def _enabled(dev, tab, enabled):
    if enabled is None:
        return None
    e = torch.as_tensor(np.asarray(enabled.cpu() if torch.is_tensor(enabled) else enabled).astype(bool).astype(np.uint8))
    if e.numel() < tab.n:
        raise ValueError("enabled has one flag per call of the table")
    return e.to(dev.dev).contiguous()


def _run(dev, tab, vals, mode, enabled, ids=None, sizing=False):
    if tab is None or tab.h is None:
        raise ValueError("a CallTable is needed")
    data, off = _vals(dev, vals)
    en = _enabled(dev, tab, enabled)
    n = max(off.numel() - 1, 0)
    coff = torch.empty(n + 1, dtype=torch.int64, device=dev.dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev.dev)
    err_line = torch.empty(n, dtype=torch.int32, device=dev.dev)
    flag = torch.empty(n, dtype=torch.uint8, device=dev.dev)
    total = ctypes.c_uint64()
    dev.sync_stream()

    def call(o):
        try:
            check(dev.L.syzsig_prog_calls_dev(dev.eng.h, tab.h, _p(data), data.numel(), _p(off), n, mode, _p(en), _p(coff),
                                              _p(o), o.numel() if o is not None else 0, _p(status), _p(err_line),
                                              _p(flag), ctypes.byref(total)))
        except _lib.SyzsigError as e:
            e.needed = int(total.value)
            raise

    if ids is None:
        call(None)  # the sizing call
        if sizing:
            return coff, None, status, err_line, flag
        ids = torch.empty(int(total.value), dtype=torch.int32, device=dev.dev)
    elif ids.device != dev.dev or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError("ids is a contiguous int32 tensor on the device")
    if ids.numel() or n:
        call(ids)
    return coff, ids[: total.value], status, err_line, flag


def prog_calls(dev, tab, vals, enabled=None, ids=None, sizing=False):
    """The calls Deserialize would give each program, from the heads of its
    lines alone (syzsig_prog_calls_dev, SYZSIG_PROGTEXT_DESERIALIZE).  vals:
    (data, off) on the device, or a list of byte strings.  Returns (off
    int64[n + 1], ids int32[total], status uint8[n], err_line int32[n], disabled
    uint8[n]) on the device; (off, ids) goes straight into
    prio.calculate_priorities.  A program that is not OK (STATUS) has an empty
    range; err_line is its first failing line, 1-based, skipped lines counted;
    disabled[i] = 1 when a call of an OK program has enabled[id] == 0.  It does
    not parse arguments, it does not run validate(), and it does not run
    SanitizeCall: a program whose heads are well-formed but whose arguments are
    broken is reported OK here.  A given `ids` that is too small raises
    SyzsigError(SYZSIG_ERANGE) with the needed count in .needed; sizing=True
    stops after everything but the ids."""
    return _run(dev, tab, vals, DESERIALIZE, enabled, ids, sizing)


def call_set(dev, tab, vals, enabled=None, ids=None, sizing=False):
    """prog.CallSet of each program (SYZSIG_PROGTEXT_CALLSET): (off, ids, status,
    err_line, supported uint8[n], has_unknown uint8[n]); ids = the distinct names
    found in the table, ascending; has_unknown: some name is not in the table;
    supported = not has_unknown and every id enabled (managerSupportsAllCalls)."""
    off, i, status, err_line, flag = _run(dev, tab, vals, CALLSET, enabled, ids, sizing)
    return off, i, status, err_line, flag & 1, flag >> 1


def load_corpus(dev, tab, db, enabled):
    """loadCorpus's split (syz-manager/manager.go:209-240) without the shuffle:
    (broken, disabled, candidates), the index arrays (int64, on the device) of
    db's records in db's order -- broken: the heads do not parse; disabled: a
    call is not enabled (the caller remembers their keys in disabledHashes);
    candidates: the rest.  db: a db.DB or a (data, off) pair."""
    vals = db.vals if hasattr(db, "vals") else db
    _, _, status, _, dis = prog_calls(dev, tab, vals, enabled, sizing=True)
    bad = status != 0
    return (torch.nonzero(bad).flatten(), torch.nonzero(~bad & (dis != 0)).flatten(),
            torch.nonzero(~bad & (dis == 0)).flatten())


def stats(dev):
    """(lines seen, lines skipped, heads parsed in the window, heads on the long
    list) of the last prog_calls / call_set (syzsig_prog_calls_stats)."""
    out = (ctypes.c_uint64 * 4)()
    check(dev.L.syzsig_prog_calls_stats(dev.eng.h, out))
    return tuple(int(x) for x in out)
