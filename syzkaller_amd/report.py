"""The corpus-wide loops behind the manager's coverage pages on device: the
numeric part of syz-manager/html.go and syz-manager/cover.go --
collectSyscallInfo (html.go:135-149), httpCover's selection (html.go:202-212),
RestorePC / previousInstructionPC / httpRawCover's sort (html.go:319-331,
cover.go:99-104, :394-411) and uncoveredPcsInFuncs (cover.go:254-304).

The text tools stay with the caller: objdump, nm, readelf, addr2line, the
source files and the HTML template.  Call names are interned to dense ids by
Corpus; PCs are numpy / torch integers.  Everything is computed by libsyzsig's
kernels (csrc/report.hip); torch owns the buffers.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check
from .signal import Cover

__all__ = ["ARCH", "Corpus", "call_cover", "syscall_info", "cover_for", "report_pcs", "raw_cover_text",
           "all_cover_pcs", "sort_symbols", "uncovered_pcs", "report_stats"]

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
