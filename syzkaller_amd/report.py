"""The corpus-wide loops behind the manager's coverage pages on device: the
numeric part of syz-manager/html.go and syz-manager/cover.go --
collectSyscallInfo (html.go:135-149), httpCover's selection (html.go:202-212),
RestorePC / previousInstructionPC / httpRawCover's sort (html.go:319-331,
cover.go:99-104, :394-411), uncoveredPcsInFuncs (cover.go:254-304), fileSet
(cover.go:162-193) and the line walk's Coverage count (cover.go:129-148).

The text tools stay with the caller: objdump, nm, readelf, addr2line, the
source files and the HTML template.  Call names are interned to dense ids by
Corpus, file and function names by Frames; PCs are numpy / torch integers.  Everything is computed by libsyzsig's
kernels (csrc/report.hip); torch owns the buffers.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check
from .signal import Cover

__all__ = ["ARCH", "Corpus", "call_cover", "syscall_info", "cover_for", "report_pcs", "raw_cover_text",
           "all_cover_pcs", "sort_symbols", "uncovered_pcs", "report_stats", "Frames", "file_set", "file_set_dict",
           "file_set_stats", "parse_file_nlines", "file_order", "cover_files"]

ARCH = {"amd64": _lib.SYZSIG_ARCH_AMD64, "386": _lib.SYZSIG_ARCH_386, "arm64": _lib.SYZSIG_ARCH_ARM64,
        "arm": _lib.SYZSIG_ARCH_ARM, "ppc64le": _lib.SYZSIG_ARCH_PPC64LE}


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if (t is not None and t.numel()) else 0)


def _u64(dev, a):
    """u64 values as an int64 tensor on the device (torch has no uint64 arithmetic; the bits are what travels)."""
    if torch.is_tensor(a):
        if a.dtype != torch.int64:
            raise ValueError("a tensor of u64 values is int64 (the same bits)")
        return a.reshape(-1).to(dev.dev).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64)).to(dev.dev)


def _host_u64(t):
    return t.cpu().numpy().view(np.uint64)


class Corpus:
    """mgr.corpus (map[string]rpctype.RPCInput) as the report kernels read it:
    the inputs' covers as CSR on the device and their calls as dense ids.
    inputs: {sig: (call name, cover u32[])}, or an iterable of (sig, call,
    cover).  .calls lists the interned names (id = index), in first-seen order;
    extra names (calls without inputs) may be given up front."""

    def __init__(self, dev, inputs, calls=()):
        rows = [(k, v[0], v[1]) for k, v in inputs.items()] if isinstance(inputs, dict) else [tuple(r) for r in inputs]
        self.dev = dev
        self.calls = list(calls)
        self.call_id = {c: i for i, c in enumerate(self.calls)}
        self.sigs = [r[0] for r in rows]
        self.index = {s: i for i, s in enumerate(self.sigs)}
        if len(self.index) != len(self.sigs):
            raise ValueError("corpus keys are distinct (it is a map)")
        ids = np.empty(len(rows), np.uint32)
        for i, (_, call, _) in enumerate(rows):
            if call not in self.call_id:
                self.call_id[call] = len(self.calls)
                self.calls.append(call)
            ids[i] = self.call_id[call]
        covs = [np.ascontiguousarray(r[2], dtype=np.uint32).reshape(-1) for r in rows]
        off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([c.size for c in covs], out=off[1:])
        cov = np.concatenate(covs) if covs else np.empty(0, np.uint32)
        self.host_call = ids
        self.off = torch.from_numpy(off).to(dev.dev)
        self.cov = torch.from_numpy(cov.view(np.int32)).to(dev.dev)
        self.call = torch.from_numpy(ids.view(np.int32)).to(dev.dev)

    @property
    def ninputs(self):
        return len(self.sigs)

    @property
    def ncalls(self):
        return len(self.calls)

    @property
    def total(self):
        return self.cov.numel()


def call_cover(corpus, select=None, want_all=False, cover_cap=None):
    """syzsig_call_cover_dev over the corpus (select: None = every input, else
    ninputs flags).  Returns (count int32[ncalls], cover_len int32[ncalls], off
    int64[ncalls + 1], cov int32[...], all): the per-call unions as CSR on the
    device, PCs ascending (u32 bits), and with want_all the union over all
    selected inputs (else None)."""
    dev = corpus.dev
    n, nc = corpus.ninputs, corpus.ncalls
    if select is not None:
        select = torch.as_tensor(np.asarray(select.cpu() if torch.is_tensor(select) else select).astype(bool)
                                 .astype(np.uint8)).to(dev.dev).contiguous()
        if select.numel() != n:
            raise ValueError("select has one flag per input")
    cap = corpus.total if cover_cap is None else int(cover_cap)
    count = torch.zeros(nc, dtype=torch.int32, device=dev.dev)
    cover_len = torch.zeros(nc, dtype=torch.int32, device=dev.dev)
    off = torch.zeros(nc + 1, dtype=torch.int64, device=dev.dev)
    cov = torch.empty(cap, dtype=torch.int32, device=dev.dev)
    allc = torch.empty(max(cap, 1), dtype=torch.int32, device=dev.dev) if want_all else None  # (never NULL)
    n_all = ctypes.c_uint64(0)
    dev.sync_stream()
    check(dev.L.syzsig_call_cover_dev(dev.eng.h, _p(corpus.off), _p(corpus.cov), n, corpus.total, _p(corpus.call),
                                      _p(select), nc, _p(count), _p(cover_len), ctypes.c_void_p(off.data_ptr()), _p(cov),
                                      cap, ctypes.c_void_p(allc.data_ptr()) if want_all else None,
                                      ctypes.byref(n_all) if want_all else None))
    return count, cover_len, off, cov, (allc[:n_all.value] if want_all else None)


def syscall_info(corpus):
    """collectSyscallInfo (html.go:135-149): {call: (count, len(cov))} for the
    calls that have an input -- the Go map has no other keys; an input with an
    empty cover still counts."""
    count, cover_len, _, _, _ = call_cover(corpus)
    count, cover_len = count.cpu().numpy(), cover_len.cpu().numpy()
    return {corpus.calls[c]: (int(count[c]), int(cover_len[c])) for c in np.flatnonzero(count).tolist()}


def cover_for(corpus, call=None, input=None):
    """httpCover's cov (html.go:202-212) as a Cover: one input's cover
    (KeyError when the corpus has no such input: Go dereferences nil there),
    the union over one call's inputs, or over all inputs.  A selection without
    inputs leaves the Cover nil, as Go's loop does; an empty result is the
    caller's "No coverage data available"."""
    if input is not None and input != "":
        sel = np.zeros(corpus.ninputs, np.uint8)
        sel[corpus.index[input]] = 1
    elif call is None or call == "":
        sel = None
    else:
        cid = corpus.call_id.get(call, -1)
        sel = (corpus.host_call == cid).astype(np.uint8) if corpus.ninputs else np.zeros(0, np.uint8)
    c = Cover(corpus.dev.eng)
    if corpus.ninputs == 0 or (sel is not None and not sel.any()):
        return c
    allc = call_cover(corpus, sel, want_all=True)[4]
    c.merge_dev(allc.contiguous())
    return c


def _arch(arch):
    if isinstance(arch, str):
        return ARCH.get(arch, 0xFFFFFFFF)  # an unknown name: the library's SYZSIG_EINVAL (Go panics)
    return int(arch) & 0xFFFFFFFF


def report_pcs(dev, pcs, base, arch):
    """syzsig_report_pcs_dev: (order, sorted) int64 tensors (u64 bits) on the
    device -- previousInstructionPC(arch, RestorePC(pc, base)) per PC in input
    order (generateCoverHTML, cover.go:99-104) and ascending (httpRawCover,
    html.go:323-331).  pcs: u32 values (numpy) or a 32-bit device tensor."""
    if torch.is_tensor(pcs):
        if pcs.element_size() != 4:
            raise ValueError("pcs is a 32-bit tensor")
        pcs = pcs.reshape(-1).to(dev.dev).contiguous()
    else:
        pcs = torch.from_numpy(np.ascontiguousarray(pcs, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev.dev)
    n = pcs.numel()
    order = torch.empty(n, dtype=torch.int64, device=dev.dev)
    srt = torch.empty(n, dtype=torch.int64, device=dev.dev)
    dev.sync_stream()
    check(dev.L.syzsig_report_pcs_dev(dev.eng.h, _p(pcs), n, int(base) & 0xFFFFFFFF, _arch(arch), _p(order), _p(srt)))
    return order, srt


def raw_cover_text(cover, base, arch, dev=None):
    """httpRawCover's body (html.go:323-338) for a Cover: "0x%x\\n" per
    previous-instruction PC, ascending; the formatting runs on the host."""
    if dev is None:
        from .device import Device
        dev = Device(cover._s._e.device)
    _, srt = report_pcs(dev, cover.Serialize(), base, arch)
    return "".join("0x%x\n" % int(pc) for pc in _host_u64(srt).tolist())


def all_cover_pcs(pcs):
    """allCoverPCs (cover.go:306-363's list) as syzsig_uncovered_pcs_dev wants
    it: ascending without repeats (host u64).  The result is a map's keys, so
    dropping repeats cannot change it."""
    return np.unique(np.asarray(pcs, dtype=np.uint64).reshape(-1))


def sort_symbols(symbols):
    """symbols: (start, end) pairs with end = Addr + Size.  Sorted by start as
    sort.Sort(symbols) leaves them (cover.go:265); equal starts keep the
    caller's order.  Returns (start u64[], end u64[])."""
    a = np.asarray(list(symbols), dtype=np.uint64).reshape(-1, 2)
    o = np.argsort(a[:, 0], kind="stable")
    return np.ascontiguousarray(a[o, 0]), np.ascontiguousarray(a[o, 1])


def uncovered_pcs(dev, sym_start, sym_end, all_cover, pcs):
    """uncoveredPcsInFuncs (cover.go:254-304) for `pcs` in the order the loop
    sees them (syzsig_uncovered_pcs_dev): the keys of `uncovered`, ascending,
    as an int64 tensor (u64 bits) on the device.  sym_start / sym_end as
    sort_symbols gives them, all_cover as all_cover_pcs gives it."""
    ss, se, ac, pc = _u64(dev, sym_start), _u64(dev, sym_end), _u64(dev, all_cover), _u64(dev, pcs)
    if ss.numel() != se.numel():
        raise ValueError("one end per symbol start")
    out = torch.empty(ac.numel(), dtype=torch.int64, device=dev.dev)
    n = ctypes.c_uint64(0)
    dev.sync_stream()
    check(dev.L.syzsig_uncovered_pcs_dev(dev.eng.h, _p(ss), _p(se), ss.numel(), _p(ac), ac.numel(), _p(pc), pc.numel(),
                                         _p(out), ctypes.byref(n)))
    return out[:n.value]


def report_stats(dev):
    """(call segments past SYZSIG_COVER_TILE, merge passes, functions handled,
    functions whose sites a workgroup walked) of the last report call
    (syzsig_report_stats)."""
    out = (ctypes.c_uint64 * 4)()
    check(dev.L.syzsig_report_stats(dev.eng.h, out))
    return tuple(int(x) for x in out)


# ---- fileSet and the per-file Coverage (cover.go:129-193) ----

def _ids(dev, a, what):
    """dense ids or lines as an int32 tensor on the device (u32 ids travel as the same bits)"""
    if torch.is_tensor(a):
        if a.element_size() != 4 or a.is_floating_point():
            raise ValueError(f"{what} is a 32-bit integer tensor")
        return a.reshape(-1).to(dev.dev).contiguous().view(torch.int32)
    a = np.asarray(a)
    if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 32)):
        raise ValueError(f"{what} does not fit 32 bits")
    a = np.ascontiguousarray(a.astype(np.int64).astype(np.uint32).reshape(-1))
    return torch.from_numpy(a.view(np.int32)).to(dev.dev)


def _is_interned(x):
    return isinstance(x, tuple) and len(x) == 3 and all(hasattr(a, "dtype") for a in x)


class Frames:
    """coveredFrames and uncoveredFrames ([]symbolizer.Frame) as the file_set
    kernels read them: per list three parallel arrays on the device -- dense
    file ids, lines (int32) and dense function ids.  A list is an iterable of
    (File, Line, Func) tuples, whose names are interned here as Corpus interns
    call names (first-seen order over covered, then uncovered; names may be
    given up front), or a tuple (file_ids, lines, func_ids) of arrays / tensors
    that the caller interned, and then files / funcs give the names, or just
    their counts.  funcs is keyed by the name alone, as the Go map is: one name
    is one id whatever its file."""

    def __init__(self, dev, covered, uncovered, files=(), funcs=()):
        self.dev = dev
        self.files, self.nfiles = (None, int(files)) if isinstance(files, int) else (list(files), None)
        self.funcs, self.nfuncs = (None, int(funcs)) if isinstance(funcs, int) else (list(funcs), None)
        self.file_id = {f: i for i, f in enumerate(self.files or ())}
        self.func_id = {f: i for i, f in enumerate(self.funcs or ())}
        self.cov = self._list(covered)
        self.unc = self._list(uncovered)
        if self.nfiles is None:
            self.nfiles = len(self.files)
        if self.nfuncs is None:
            self.nfuncs = len(self.funcs)

    def _intern(self, names, ids, name, what):
        if names is None:
            raise ValueError(f"frames with {what} names need the names' list, not a count")
        i = ids.get(name)
        if i is None:
            i = ids[name] = len(names)
            names.append(name)
        return i

    def _list(self, frames):
        if _is_interned(frames):
            t = (_ids(self.dev, frames[0], "file ids"), _ids(self.dev, frames[1], "lines"),
                 _ids(self.dev, frames[2], "function ids"))
            if not t[0].numel() == t[1].numel() == t[2].numel():
                raise ValueError("a frame has a file, a line and a function")
            return t
        rows = [tuple(r) for r in frames]
        a = np.empty((3, len(rows)), np.int64)
        for i, (file, line, func) in enumerate(rows):
            a[0, i] = self._intern(self.files, self.file_id, file, "file")
            a[1, i] = int(line)
            a[2, i] = self._intern(self.funcs, self.func_id, func, "function")
        return _ids(self.dev, a[0], "file ids"), _ids(self.dev, a[1], "lines"), _ids(self.dev, a[2], "function ids")

    @property
    def ncov(self):
        return self.cov[0].numel()

    @property
    def nunc(self):
        return self.unc[0].numel()


def _nlines_tensor(frames, nlines):
    if isinstance(nlines, dict):
        if frames.files is None:
            raise ValueError("nlines by name needs the files' names")
        nlines = [nlines.get(f, 0) for f in frames.files]  # (a file without a count shows nothing)
    t = _ids(frames.dev, nlines, "nlines")
    if t.numel() != frames.nfiles:
        raise ValueError("nlines has one count per file")
    return t


def file_set(frames, nlines=None, cap=None):
    """syzsig_file_set_dev: fileSet(covered, uncovered) (cover.go:162-193) as
    CSR over the interned files, and with nlines the walk of cover.go:129-148.
    Returns device tensors (off int64[nfiles + 1], line int32[...], covered
    uint8[...], shown, coverage): file f's sorted (line, covered) list is
    line / covered[off[f]:off[f + 1]]; shown[f] = the entries the walk
    consumes, coverage[f] = templateFile.Coverage (both None without nlines).
    nlines: {file: len(parseFile(file))} or one count per file id."""
    dev = frames.dev
    nf = frames.nfiles
    cap = frames.ncov + frames.nunc if cap is None else int(cap)
    off = torch.zeros(nf + 1, dtype=torch.int64, device=dev.dev)
    line = torch.empty(cap, dtype=torch.int32, device=dev.dev)
    covered = torch.empty(cap, dtype=torch.uint8, device=dev.dev)
    nl = shown = coverage = None
    if nlines is not None and nf:  # (no files: nothing to walk, and nothing to point at)
        nl = _nlines_tensor(frames, nlines)
        shown = torch.zeros(nf, dtype=torch.int32, device=dev.dev)
        coverage = torch.zeros(nf, dtype=torch.int32, device=dev.dev)
    dev.sync_stream()
    check(dev.L.syzsig_file_set_dev(dev.eng.h, _p(frames.cov[0]), _p(frames.cov[1]), _p(frames.cov[2]), frames.ncov,
                                    _p(frames.unc[0]), _p(frames.unc[1]), _p(frames.unc[2]), frames.nunc, nf,
                                    frames.nfuncs, _p(nl), ctypes.c_void_p(off.data_ptr()), _p(line), _p(covered), cap,
                                    _p(shown), _p(coverage)))
    n = int(off[-1])
    if nlines is not None and not nf:
        shown = torch.zeros(0, dtype=torch.int32, device=dev.dev)
        coverage = torch.zeros(0, dtype=torch.int32, device=dev.dev)
    return off, line[:n], covered[:n], shown, coverage


def file_set_dict(frames, cap=None):
    """fileSet's Go map: {file: [(line, covered), ...]} with only the files that
    have entries (names, or ids when the frames came interned without names)."""
    off, line, covered, _, _ = file_set(frames, cap=cap)
    off, line, covered = off.cpu().numpy(), line.cpu().numpy().tolist(), covered.cpu().numpy().astype(bool).tolist()
    return {(frames.files[f] if frames.files is not None else f):
            list(zip(line[off[f]:off[f + 1]], covered[off[f]:off[f + 1]]))
            for f in np.flatnonzero(np.diff(off)).tolist()}


def file_set_stats(dev):
    """(uncovered frames kept by the funcs filter, files of more than
    SYZSIG_FILESET_TILE frames, merge passes, entries written) of the last
    file_set call (syzsig_file_set_stats)."""
    out = (ctypes.c_uint64 * 4)()
    check(dev.L.syzsig_file_set_stats(dev.eng.h, out))
    return tuple(int(x) for x in out)


def parse_file_nlines(data):
    """len(parseFile(f)) for a file's bytes (cover.go:195-214): one line per
    '\n', and one more when bytes follow the last '\n'."""
    data = bytes(data)
    return data.count(b"\n") + (1 if data and not data.endswith(b"\n") else 0)


def file_order(names):
    """The names as sort.Sort(templateFileArray) leaves them (cover.go:427-440):
    names that start with '.' -- include files -- go below the others, each
    group ascending; the empty name compares as a plain string."""
    return sorted(names, key=lambda n: (n[:1] == ".", n))


def cover_files(dev, cover_pcs, base, arch, sym_start, sym_end, all_cover, symbolize, nlines, files=(), funcs=()):
    """generateCoverHTML's numeric path (cover.go:99-158), one device call per
    step: report_pcs -> uncovered_pcs -> symbolize(covered PCs),
    symbolize(uncovered PCs) -> file_set with the walk.  symbolize(pcs) takes
    an int64 device tensor (u64 bits) and returns the frames of those PCs as
    Frames takes a list -- (File, Line, Func) tuples, or three arrays interned
    against files / funcs; File is the name the page shows (the common prefix
    is text and stays with the caller).  Returns the page's files in
    templateFileArray's order: dicts with ID (hash.String(Name), from the
    batch hash), Name, Coverage, shown, and line / covered numpy arrays of the
    file's sorted list.  No covered frames: ValueError, as Go's "does not have
    debug info"."""
    from . import hashing

    order, _ = report_pcs(dev, cover_pcs, base, arch)
    unc = uncovered_pcs(dev, sym_start, sym_end, all_cover, order)
    frames = Frames(dev, symbolize(order), symbolize(unc), files, funcs)
    if frames.ncov == 0:
        raise ValueError("no covered frames: the kernel object does not have debug info")
    if frames.files is None:
        raise ValueError("cover_files needs the files' names")
    off, line, covered, shown, coverage = file_set(frames, nlines)
    off, line, covered = off.cpu().numpy(), line.cpu().numpy(), covered.cpu().numpy().astype(bool)
    shown, coverage = shown.cpu().numpy(), coverage.cpu().numpy()
    have = np.flatnonzero(np.diff(off)).tolist()
    names = [frames.files[f].encode() for f in have]
    noff = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(n) for n in names], out=noff[1:])
    sigs = hashing.hash_batch(dev, b"".join(names), noff).cpu().numpy()
    by_name = {frames.files[f]: {"ID": hashing.to_string(sigs[k]), "Name": frames.files[f], "Coverage": int(coverage[f]),
                                 "shown": int(shown[f]), "line": line[off[f]:off[f + 1]],
                                 "covered": covered[off[f]:off[f + 1]]} for k, f in enumerate(have)}
    return [by_name[n] for n in file_order(list(by_name))]
