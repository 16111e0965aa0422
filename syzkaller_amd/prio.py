"""Call-to-call priorities over the whole corpus and the ChoiceTable on device:
the numeric part of prog/prio.go -- CalculatePriorities (prio.go:27-36, :133-187;
syz-manager/manager.go:896 on Connect), the tail of calcStaticPriorities
(:118-129), BuildChoiceTable (:198-228; syz-fuzzer/fuzzer.go:173) and Choose's
lookup (:230-245; prog/rand.go:398).

A corpus is the calls' Meta.IDs per program; deserialising program text into
ids stays with the caller.  Matrices are float32[N, N] tensors on the device,
bit for bit what the reference computes on amd64.  Everything is computed by
libsyzsig's kernels (csrc/prio.hip); torch owns the buffers.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check

__all__ = ["MAX_CALLS", "SPLIT", "corpus_csr", "calculate_priorities", "prio_stats", "static_finish", "ChoiceTable"]

MAX_CALLS = _lib.SYZSIG_PRIO_MAX_CALLS
SPLIT = _lib.SYZSIG_PRIO_SPLIT


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if (t is not None and t.numel()) else 0)


def corpus_csr(dev, corpus_ids):
    """A corpus as (off int64[nprog + 1], ids int32[total]) on the device: from a
    list of id lists, or from such a pair of tensors / arrays (the ids' 32 bits
    are Meta.ID as u32)."""
    if isinstance(corpus_ids, tuple) and len(corpus_ids) == 2 and (torch.is_tensor(corpus_ids[0])
                                                                   or isinstance(corpus_ids[0], np.ndarray)):
        off, ids = corpus_ids
        off = torch.as_tensor(off).to(torch.int64)
        ids = torch.as_tensor(ids)
        if ids.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16):
            raise ValueError("ids are integers")
        if ids.dtype != torch.int32:
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= 1 << 32):
                raise ValueError("a call id is a u32")
            ids = torch.from_numpy(ids.cpu().numpy().astype(np.uint32).view(np.int32))
    else:
        progs = [np.asarray(p, np.int64).reshape(-1) for p in corpus_ids]
        off_np = np.zeros(len(progs) + 1, np.int64)
        np.cumsum([p.size for p in progs], out=off_np[1:])
        flat = np.concatenate(progs) if progs else np.empty(0, np.int64)
        if flat.size and (flat.min() < 0 or flat.max() >= 1 << 32):
            raise ValueError("a call id is a u32")
        off, ids = torch.from_numpy(off_np), torch.from_numpy(flat.astype(np.uint32).view(np.int32))
    return off.to(dev.dev).contiguous(), ids.to(dev.dev).contiguous()


def _matrix(dev, m, ncalls, what):
    m = torch.as_tensor(m)
    if m.dtype != torch.float32 or m.numel() != ncalls * ncalls:
        raise ValueError(f"{what} is float32[N, N]")
    return m.to(dev.dev).contiguous()


def calculate_priorities(dev, corpus_ids, ncalls, static=None, split=0, out=None):
    """target.CalculatePriorities(corpus) (syzsig_calc_prios_dev): the
    normalised pair counts of calcDynamicPrio, times `static` (float32[N, N],
    calcStaticPriorities' result) when given.  corpus_ids: a list of id lists or
    (off, ids).  split: a call with more occurrences has its row counted in
    slices (0 = the default); the result does not depend on it.  Returns
    float32[N, N] on the device (`out` if given)."""
    off, ids = corpus_csr(dev, corpus_ids)
    nprog = max(off.numel() - 1, 0)
    if static is not None:
        static = _matrix(dev, static, ncalls, "static")
    if out is None:
        out = torch.empty((ncalls, ncalls), dtype=torch.float32, device=dev.dev)
    if out.device != dev.dev or out.dtype != torch.float32 or out.numel() < ncalls * ncalls or not out.is_contiguous():
        raise ValueError("out is a contiguous float32[N, N] on the device")
    dev.sync_stream()
    check(dev.L.syzsig_calc_prios_dev(dev.eng.h, _p(off), _p(ids), nprog, ids.numel(), ncalls, split, _p(static),
                                      ctypes.c_void_p(out.data_ptr())))
    return out


def prio_stats(dev):
    """(rows counted whole, rows split, slices, pair increments = sum of len^2)
    of the last calculate_priorities (syzsig_prio_stats)."""
    out = (ctypes.c_uint64 * 4)()
    check(dev.L.syzsig_prio_stats(dev.eng.h, out))
    return tuple(int(x) for x in out)


def static_finish(dev, mat):
    """The tail of calcStaticPriorities (prio.go:118-129) on the summed matrix
    (syzsig_static_prio_finish_dev): the diagonal takes each row's max, then
    normalizePrio.  Returns a new float32[N, N] on the device."""
    mat = torch.as_tensor(mat)
    if mat.dtype != torch.float32 or mat.dim() != 2 or mat.shape[0] != mat.shape[1]:
        raise ValueError("mat is float32[N, N]")
    m = mat.to(dev.dev).contiguous().clone()
    dev.sync_stream()
    check(dev.L.syzsig_static_prio_finish_dev(dev.eng.h, ctypes.c_void_p(m.data_ptr()), m.shape[0]))
    return m


class ChoiceTable:
    """prog.ChoiceTable: .run is int32[N, N] on the device, row i the running
    sums of BuildChoiceTable (zeros for a disabled row, nil in Go)."""

    def __init__(self, dev, run, enabled, ncalls):
        self.dev, self.run, self.ncalls = dev, run, ncalls
        self.enabled = enabled  # uint8[N] on the device, or None: every call
        self._enabled_calls = None

    @classmethod
    def build(cls, dev, prios, enabled, ncalls, out=None):
        """target.BuildChoiceTable(prios, enabled) (syzsig_choice_table_dev).
        prios: float32[N, N] or None (Go's nil: every weight 1); enabled: N
        flags or None (every call).  A weight that Go's int() does not define
        raises SyzsigError(SYZSIG_EINVAL) naming the first such row."""
        if prios is not None:
            prios = _matrix(dev, prios, ncalls, "prios")
        if enabled is not None:
            enabled = torch.as_tensor(np.asarray(enabled.cpu() if torch.is_tensor(enabled) else enabled).astype(bool)
                                      .astype(np.uint8)).to(dev.dev).contiguous()
            if enabled.numel() != ncalls:
                raise ValueError("enabled has N flags")
        if out is None:
            out = torch.empty((ncalls, ncalls), dtype=torch.int32, device=dev.dev)
        if out.device != dev.dev or out.dtype != torch.int32 or out.numel() < ncalls * ncalls or not out.is_contiguous():
            raise ValueError("out is a contiguous int32[N, N] on the device")
        dev.sync_stream()
        check(dev.L.syzsig_choice_table_dev(dev.eng.h, _p(prios), _p(enabled), ncalls,
                                            ctypes.c_void_p(out.data_ptr())))
        return cls(dev, out, enabled, ncalls)

    def lookup(self, call, x, out=None):
        """sort.SearchInts(run[call], x) for arrays of queries
        (syzsig_choice_lookup_dev): int32[n] on the device, N (the sentinel:
        "uniform over enabledCalls") where call < 0 or the row is disabled."""
        dev = self.dev
        call = torch.as_tensor(call, dtype=torch.int32).reshape(-1).to(dev.dev).contiguous()
        x = torch.as_tensor(x, dtype=torch.int32).reshape(-1).to(dev.dev).contiguous()
        if call.numel() != x.numel():
            raise ValueError("one x per call")
        n = call.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=dev.dev)
        if out.device != dev.dev or out.dtype != torch.int32 or out.numel() < n or not out.is_contiguous():
            raise ValueError("out is a contiguous int32[n] on the device")
        dev.sync_stream()
        check(dev.L.syzsig_choice_lookup_dev(dev.eng.h, _p(self.run), self.ncalls, _p(call), _p(x), n, _p(out)))
        return out

    def totals(self):
        """run[i][N - 1] per row (host int64[N]): what Choose draws x below."""
        return self.run.view(self.ncalls, self.ncalls)[:, -1].cpu().numpy().astype(np.int64)

    def choose(self, rng, call):
        """ChoiceTable.Choose(r, call) for one call or an array of them, with
        rng a numpy Generator: x = r.Intn(total) + 1 drawn here, the lookup on
        the device, and the sentinel resolved as the reference does: a uniform
        draw over enabledCalls (in ascending id order; Go's order is its map's).
        Returns int64[n] on the host (an int for a scalar call)."""
        scalar = np.isscalar(call)
        calls = np.atleast_1d(np.asarray(call, np.int64))
        if calls.size and calls.max() >= self.ncalls:
            raise ValueError("call is below N")
        tot = self.totals()
        t = np.where(calls >= 0, tot[np.clip(calls, 0, None)], 0)
        x = np.where(t > 0, rng.integers(1, np.maximum(t, 1) + 1), 1).astype(np.int32)
        got = self.lookup(calls.astype(np.int32), x).cpu().numpy().astype(np.int64)
        uni = got == self.ncalls
        if uni.any():
            if self._enabled_calls is None:
                self._enabled_calls = (np.arange(self.ncalls) if self.enabled is None
                                       else np.flatnonzero(self.enabled.cpu().numpy()))
            if self._enabled_calls.size == 0:
                raise ValueError("no enabled calls")
            got[uni] = self._enabled_calls[rng.integers(0, self._enabled_calls.size, int(uni.sum()))]
        return int(got[0]) if scalar else got
