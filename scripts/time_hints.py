#!/usr/bin/env python3
"""Device time of syzsig_hint_mutants_dev (checkConstArg / checkDataArg over a
batch of args, prog/hints.go:105-132) beside the same result composed from
windows built in torch and syzsig_shrink_expand_dev, in the same process.

    python scripts/time_hints.py            # 4096 calls x 1024 comparisons, 4 args per call

Per call: two const args (keys of its map) and two data args of 64 and 256
bytes drawn from its operand pool (keys little-endian back to back).  Times are
HIP events on the library's stream around each route -- for the composition
the window building included -- the median of --reps runs after one warm-up;
ms_library is the span the library itself times (syzsig_ctx_last_ms).  The
algorithmic traffic of the new call is the args' heads (at most 107 bytes per
data arg), 16 B per accepted candidate and 13 B per mutant, plus the offsets;
beside the achievable bandwidth of a plain device copy.  Prints one JSON line.
Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from syzkaller_amd import _lib, synth  # noqa: E402
from syzkaller_amd.device import Device  # noqa: E402
from syzkaller_amd.hints import SPECIAL_INTS, CompMap  # noqa: E402
from time_comps import OUT_START, achievable_bw  # noqa: E402

MAXD = _lib.SYZSIG_HINT_MAX_DATA


def timed(dev, reps, fn):
    outer, lib, r = [], [], None
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        outer.append(e0.elapsed_time(e1))
        lib.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
    return float(np.median(outer[1:])), float(np.median(lib[1:])), r


def build_args(rng, hoff, hpairs, ncalls, lens=(64, 256)):
    call, kind, val, off, data = [], [], [], [0], bytearray()
    for c in range(ncalls):
        keys = hpairs[int(hoff[c]):int(hoff[c + 1]), 0]
        if keys.size == 0:
            keys = np.array([0x1234], np.uint64)
        for _ in range(2):
            call.append(c), kind.append(0), val.append(keys[rng.integers(0, keys.size)]), off.append(len(data))
        for n in lens:
            data += keys[rng.integers(0, keys.size, n // 8)].astype("<u8").tobytes()
            call.append(c), kind.append(1), val.append(0), off.append(len(data))
    return (np.array(call, np.int32), np.array(kind, np.uint8), np.array(val, np.uint64), np.array(off, np.int64),
            bytes(data))


def windows_torch(kind, val, off, data):
    """every arg's windows as shrink_expand queries, on the device: (the
    query's arg, its window, its value)"""
    n = off[1:] - off[:-1]
    nwin = torch.where(kind == 0, torch.ones_like(n), n.clamp(max=MAXD))
    arg = torch.repeat_interleave(torch.arange(n.numel(), device=n.device), nwin)
    first = torch.cumsum(nwin, 0) - nwin
    win = torch.arange(arg.numel(), device=n.device) - first[arg]
    j = torch.arange(8, device=n.device)
    pos = (off[:-1][arg] + win)[:, None] + j[None, :]
    live = (win[:, None] + j[None, :]) < n[arg][:, None]
    padded = torch.cat([data, torch.zeros(8, dtype=torch.uint8, device=data.device)])
    b = torch.where(live, padded[pos.clamp(max=padded.numel() - 1)].to(torch.int64), torch.zeros((), dtype=torch.int64,
                                                                                                  device=n.device))
    v = (b << (8 * j)[None, :]).sum(1)
    return arg, win, torch.where(kind[arg] == 0, val[arg], v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--comps", type=int, default=1024)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    bw = achievable_bw(dev)
    lens = np.full(a.calls, a.comps, np.uint32)
    comps, starts = synth.comparisons(1, lens, OUT_START, pool=a.pool)
    t = lambda x, dt: torch.from_numpy(x.view(dt)).to(dev.dev)
    dstart = t(starts, np.int64)
    words, nw, cnt = dev.exec_comps(t(comps, np.int64), dstart, t(lens, np.int32), OUT_START)
    m = CompMap.from_exec_output(dev, words, dstart, nw, cnt)
    hoff, hpairs = m.off.cpu().numpy(), m.pairs.cpu().numpy().view(np.uint64).reshape(-1, 2)
    call, kind, val, off, data = build_args(np.random.default_rng(3), hoff, hpairs, a.calls)
    dcall, dkind, dval, doff = t(call, np.int32), torch.from_numpy(kind).to(dev.dev), t(val, np.int64), t(off, np.int64)
    ddata = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev.dev)
    r0 = dev.hint_mutants(m.off, m.pairs, dcall, dkind, dval, doff, ddata, SPECIAL_INTS)
    nmut = r0[1].numel()
    outs = (torch.empty(max(nmut, 1), dtype=torch.int32, device=dev.dev),
            torch.empty(max(nmut, 1), dtype=torch.uint8, device=dev.dev),
            torch.empty(max(nmut, 1), dtype=torch.int64, device=dev.dev))
    ms_new, ms_new_lib, r = timed(dev, a.reps, lambda: dev.hint_mutants(m.off, m.pairs, dcall, dkind, dval, doff, ddata,
                                                                       SPECIAL_INTS, out=outs))
    fast, fallback, windows, cands = dev.hint_mutants_stats()
    rep_buf = torch.empty(max(nmut, 1), dtype=torch.int64, device=dev.dev)

    def composed():
        arg, win, v = windows_torch(dkind, dval, doff, ddata)
        ro, rep = dev.shrink_expand(m.off, m.pairs, dcall[arg].contiguous(), v.contiguous(), SPECIAL_INTS, rep=rep_buf)
        return arg, win, ro, rep
    ms_comp, ms_se_lib, (arg, win, ro, rep) = timed(dev, a.reps, composed)
    # the two routes agree
    per_q = ro[1:] - ro[:-1]
    assert rep.numel() == nmut and torch.equal(rep, r[3])
    assert torch.equal(torch.repeat_interleave(win, per_q).to(torch.int32), r[1])
    head = int(np.minimum(off[1:] - off[:-1], MAXD + 7).sum())
    nbytes = head + 16 * cands + 13 * nmut + 8 * (call.size + 1) + 13 * call.size
    res = {"shape": [a.calls, a.comps], "pool": a.pool, "reps": a.reps, "args": int(call.size), "list": _lib.SYZSIG_HINT_LIST,
           "achievable_bw_GBps": round(bw, 1),
           "hint_mutants": {"ms": round(ms_new, 4), "ms_library": round(ms_new_lib, 4), "windows": windows,
                            "candidates": cands, "mutants": nmut, "fast_args": fast, "fallback_args": fallback,
                            "windows_per_s": round(windows / (ms_new * 1e-3), 1), "algorithmic_bytes": nbytes,
                            "achieved_GBps": round(nbytes / (ms_new * 1e-3) / 1e9, 3),
                            "fraction_of_copy_bw": round(nbytes / (ms_new * 1e-3) / 1e9 / bw, 5)},
           "composition": {"ms": round(ms_comp, 4), "shrink_expand_ms_library": round(ms_se_lib, 4),
                           "queries": int(arg.numel())},
           "composition_over_hint_mutants": round(ms_comp / ms_new, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
