#!/usr/bin/env python3
"""Device time of the three comparison-hints entry points
(syzsig_exec_comps_dev, syzsig_comp_map_dev, syzsig_shrink_expand_dev) on
synthetic comparisons, beside syzsig_edge_cover_dev over as many 8-byte inputs
in the same process.

    python scripts/time_comps.py                              # 4096 calls x 1024: the one-tile path
    python scripts/time_comps.py --calls 64 --comps 65535     # the long path (tiles + merge passes)

Times come from the library's HIP events (syzsig_ctx_set_timing /
syzsig_ctx_last_ms; they span an entry's kernels and the host round trips
between them): the median of --reps runs after one warm-up.  keys are the
records in (exec_comps), the distinct pairs out (comp_map) and the candidate
values under the 12 mutants of every query (shrink_expand).  The bandwidth is
the algorithmic traffic -- 32 B per record in plus the words out; the words in
plus 16 B per pair; 16 B per candidate -- over that time, beside the
achievable bandwidth of a plain device copy (syzsig_copy_bw_dev).  Prints one
JSON line.  Needs the GPU.
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

OUT_START = 0x7f1200000000
M64 = (1 << 64) - 1


def achievable_bw(dev, nbytes=1 << 30, reps=5):
    src = torch.ones(nbytes // 8, dtype=torch.int64, device=dev.dev)
    dst = torch.empty_like(src)
    ms = [dev.copy_bw(dst, src, nbytes) for _ in range(reps + 1)][1:]
    return 2 * nbytes / (float(np.median(ms)) * 1e-3) / 1e9


def timed(dev, reps, fn):
    ms, r = [], None
    for _ in range(reps + 1):
        r = fn()
        ms.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
    return float(np.median(ms[1:])), r


def count_candidates(off, pairs, calls, vals):
    """the values under the 12 mutants (hints.go:165-191) of every query"""
    keys, total = pairs[:, 0], 0
    for c in np.unique(calls):
        k = keys[int(off[c]):int(off[c + 1])]
        v = vals[calls == c]
        for width, expand, be in [(8, 0, 0), (4, 0, 0), (2, 0, 0), (1, 0, 0), (4, 1, 0), (2, 1, 0), (1, 1, 0),
                                  (8, 0, 1), (4, 0, 1), (2, 0, 1), (4, 1, 1), (2, 1, 1)]:
            mask = np.uint64(M64 if width == 8 else (1 << (8 * width)) - 1)
            m = (v | ~mask) if expand else (v & mask)
            if be:
                m = (m & mask).astype({2: np.uint16, 4: np.uint32, 8: np.uint64}[width]).byteswap().astype(np.uint64)
            total += int((np.searchsorted(k, m, "right") - np.searchsorted(k, m, "left")).sum())
    return total


def entry(ms, keys, nbytes, bw, yard):
    return {"ms": round(ms, 4), "keys": keys, "keys_per_s": round(keys / (ms * 1e-3), 1),
            "algorithmic_bytes": nbytes, "achieved_GBps": round(nbytes / (ms * 1e-3) / 1e9, 2),
            "fraction_of_copy_bw": round(nbytes / (ms * 1e-3) / 1e9 / bw, 4), "over_edge_cover": round(ms / yard, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--comps", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=1 << 16)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    bw = achievable_bw(dev)
    lens = np.full(a.calls, a.comps, np.uint32)
    comps, starts = synth.comparisons(1, lens, OUT_START, pool=a.pool)
    nrec = comps.shape[0]
    dcomps = torch.from_numpy(comps.view(np.int64)).to(dev.dev)
    dstart = torch.from_numpy(starts.view(np.int64)).to(dev.dev)
    dlen = torch.from_numpy(lens.view(np.int32)).to(dev.dev)
    # the yardstick: edge_cover over nrec PCs in the same call layout
    cfg = synth.synth_default(global_walk=1)
    pcs, cs, dcl, _ = dev.synth_traces(cfg, 0, a.calls, 1, torch.from_numpy(lens.view(np.int32)))
    pidx = torch.from_numpy(synth.prog_call_index(a.calls, 1).view(np.int32)).to(dev.dev)
    _, _, comp = dev.edge_derive(pcs, cs, dcl, pidx)
    cover = torch.empty(pcs.numel(), dtype=torch.int32, device=dev.dev)
    yard, _ = timed(dev, a.reps, lambda: dev.edge_cover(pcs, cs, dcl, pidx, comp, cover=cover))
    del pcs, cover
    # entry 1
    out = torch.empty(5 * nrec, dtype=torch.int32, device=dev.dev)
    ms1, (words, nw, cnt) = timed(dev, a.reps, lambda: dev.exec_comps(dcomps, dstart, dlen, OUT_START, out=out))
    wout = int(nw.to(torch.int64).sum().item())
    # entry 2
    wstart = (5 * dstart).contiguous()
    wend = (wstart + nw.to(torch.int64)).contiguous()
    pairs_buf = torch.empty((2 * int(cnt.to(torch.int64).sum().item()), 2), dtype=torch.int64, device=dev.dev)
    ms2, (st, off, pairs) = timed(dev, a.reps, lambda: dev.comp_map(words, wstart, cnt, wend, pairs=pairs_buf))
    npairs = pairs.shape[0]
    # entry 3: values from the maps' keys, a third of them under other upper bytes
    rng = np.random.default_rng(2)
    hoff, hpairs = off.cpu().numpy(), pairs.cpu().numpy().view(np.uint64)
    calls = rng.integers(0, a.calls, a.queries).astype(np.int32)
    pick = hoff[calls] + (rng.integers(0, 1 << 62, a.queries) % np.maximum(hoff[calls + 1] - hoff[calls], 1))
    vals = hpairs[np.minimum(pick, max(npairs - 1, 0)), 0].copy()
    up = rng.integers(0, 3, a.queries) == 0
    vals[up] = (vals[up] & np.uint64(0xffff)) | (rng.integers(1, 1 << 40, int(up.sum())).astype(np.uint64) << np.uint64(16))
    m = CompMap(dev, st, off, pairs)
    dcalls = torch.from_numpy(calls).to(dev.dev)
    dvals = torch.from_numpy(vals.view(np.int64)).to(dev.dev)
    _, rep0 = m.shrink_expand(dcalls, dvals)
    rep_buf = torch.empty(max(rep0.numel(), 1), dtype=torch.int64, device=dev.dev)
    ms3, (_, rep) = timed(dev, a.reps,
                          lambda: dev.shrink_expand(off, pairs, dcalls, dvals, SPECIAL_INTS, rep=rep_buf))
    ncand = count_candidates(hoff, hpairs, calls, vals)
    res = {"shape": [a.calls, a.comps], "tile": _lib.SYZSIG_COMPS_TILE, "long_segment_path": a.comps > _lib.SYZSIG_COMPS_TILE,
           "pool": a.pool, "reps": a.reps, "achievable_bw_GBps": round(bw, 1), "edge_cover_ms": round(yard, 4),
           "exec_comps": dict(entry(ms1, nrec, 32 * nrec + 4 * wout, bw, yard), words_out=wout,
                              comps_out=int(cnt.to(torch.int64).sum().item())),
           "comp_map": dict(entry(ms2, npairs, 4 * wout + 16 * npairs, bw, yard), words_in=wout),
           "shrink_expand": dict(entry(ms3, ncand, 16 * ncand, bw, yard), queries=a.queries,
                                 replacers=int(rep.numel()))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
