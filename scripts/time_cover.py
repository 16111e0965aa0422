#!/usr/bin/env python3
"""Device time of syzsig_edge_cover_dev (dedup on) beside syzsig_edge_derive_dev
(K1+K2) on the same synthetic traces, in one process.

    python scripts/time_cover.py                       # BASELINE config 2: 4096 x 64 x 4096, both walks
    python scripts/time_cover.py --programs 2 --calls 32 --pcs 262143   # the long-segment path alone

Times come from the library's HIP events (syzsig_ctx_set_timing /
syzsig_ctx_last_ms; for edge_cover they span its kernels and the one host
round trip between them): the median of --reps runs after one warm-up.  The
bandwidth is the algorithmic traffic, 8 B per PC in plus 4 B per surviving PC
out, over that time, beside the achievable bandwidth of a plain device copy
(syzsig_copy_bw_dev).  Prints one JSON line.  Needs the GPU.
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


def achievable_bw(dev, nbytes=1 << 30, reps=5):
    src = torch.ones(nbytes // 8, dtype=torch.int64, device=dev.dev)
    dst = torch.empty_like(src)
    ms = [dev.copy_bw(dst, src, nbytes) for _ in range(reps + 1)][1:]
    return 2 * nbytes / (float(np.median(ms)) * 1e-3) / 1e9


def time_walk(dev, walk, nprog, cpp, npcs, reps):
    cfg = synth.synth_default(global_walk=1 if walk == "global" else 0)
    cl = torch.full((nprog * cpp,), npcs, dtype=torch.int32)
    pcs, cs, dcl, _ = dev.synth_traces(cfg, 0, nprog, cpp, cl)
    pidx = torch.from_numpy(synth.prog_call_index(nprog, cpp).view(np.int32)).to(dev.dev)
    sigs = torch.empty(pcs.numel(), dtype=torch.int32, device=dev.dev)
    cover = torch.empty(pcs.numel(), dtype=torch.int32, device=dev.dev)
    edge_ms, cover_ms = [], []
    for _ in range(reps + 1):
        _, _, comp = dev.edge_derive(pcs, cs, dcl, pidx, sigs=sigs)
        edge_ms.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
        _, cnt = dev.edge_cover(pcs, cs, dcl, pidx, comp, cover=cover)
        cover_ms.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
    e, c = float(np.median(edge_ms[1:])), float(np.median(cover_ms[1:]))
    surv = int(cnt.to(torch.int64).sum().item())
    nbytes = 8 * pcs.numel() + 4 * surv
    return {"edge_derive_ms": round(e, 4), "edge_cover_ms": round(c, 4), "cover_over_derive": round(c / e, 4),
            "pcs": pcs.numel(), "surviving_pcs": surv, "algorithmic_bytes": nbytes,
            "achieved_GBps": round(nbytes / (c * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--pcs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--walks", default="global,region")
    ap.add_argument("--tile", type=int, default=_lib.SYZSIG_COVER_TILE,
                    help="label only: the tile of an experiment build selected with SYZSIG_LIB")
    a = ap.parse_args()
    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    res = {"shape": [a.programs, a.calls, a.pcs], "tile": a.tile,
           "long_segment_path": a.pcs > a.tile, "reps": a.reps,
           "lib": os.path.basename(_lib.LIB_PATH)}
    for walk in a.walks.split(","):
        res[walk] = time_walk(dev, walk, a.programs, a.calls, a.pcs, a.reps)
    res["achievable_bw_GBps"] = round(achievable_bw(dev), 1)
    for walk in a.walks.split(","):
        res[walk]["fraction_of_achievable"] = round(res[walk]["achieved_GBps"] / res["achievable_bw_GBps"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
