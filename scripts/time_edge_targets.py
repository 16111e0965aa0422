#!/usr/bin/env python3
"""Device time of edge_derive (K1+K2) and edge_cover (dedup on) under the three
KCOV targets, on one synthetic batch in one process:

    x86    today's path: u64 PCs, the x86 cover_check (SYZSIG_TARGET_CHECK_X86)
    pc32   the same PCs' low words as a u32 trace (SYZSIG_TARGET_PC32): half the
           input bytes of K1, the u32 cover sort fed 4 B per key
    u64    the same u64 PCs unchecked (target 0): K1 without the abort test, the
           cover sort on full u64 keys

    python scripts/time_edge_targets.py                  # BASELINE config 2: 4096 x 64 x 4096, global walk
    python scripts/time_edge_targets.py --programs 256   # a smaller batch

Times come from the library's HIP events (syzsig_ctx_set_timing /
syzsig_ctx_last_ms).  After one warm-up round of every variant, --reps rounds run
the variants alternately (x86, pc32, u64, x86, ...), so that drift of the machine
falls on all three alike; per variant the median and the min-max spread.  The
signals and counts of the three must be equal (the low-word identity), which is
checked before any time is reported.  Prints one JSON line.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from syzkaller_amd import _lib, synth, targets  # noqa: E402
from syzkaller_amd.device import Device  # noqa: E402


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--pcs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--walk", default="global", choices=["global", "region"])
    a = ap.parse_args()
    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    cfg = synth.synth_default(global_walk=1 if a.walk == "global" else 0)
    cl = torch.full((a.programs * a.calls,), a.pcs, dtype=torch.int32)
    pcs, cs, dcl, _ = dev.synth_traces(cfg, 0, a.programs, a.calls, cl)
    pidx = torch.from_numpy(synth.prog_call_index(a.programs, a.calls).view(np.int32)).to(dev.dev)
    variants = {"x86": (pcs, targets.CHECK_X86), "pc32": (pcs.to(torch.int32), targets.PC32), "u64": (pcs, 0)}
    n = pcs.numel()
    sigs = {k: torch.empty(n, dtype=torch.int32, device=dev.dev) for k in variants}
    cover = torch.empty(n, dtype=torch.int32, device=dev.dev)
    derive = {k: [] for k in variants}
    cov = {k: [] for k in variants}
    cnts, ccnts = {}, {}
    for rep in range(a.reps + 1):
        for k, (p, t) in variants.items():
            _, cnt, comp = dev.edge_derive(p, cs, dcl, pidx, sigs=sigs[k], target=t)
            d = dev.L.syzsig_ctx_last_ms(dev.eng.h)
            _, ccnt = dev.edge_cover(p, cs, dcl, pidx, comp, cover=cover, target=t)
            c = dev.L.syzsig_ctx_last_ms(dev.eng.h)
            if rep == 0:  # the warm-up round: its results are the equality check's
                cnts[k], ccnts[k] = cnt.clone(), ccnt.clone()
            else:
                derive[k].append(d)
                cov[k].append(c)
    for k in ("pc32", "u64"):
        assert torch.equal(cnts[k], cnts["x86"]) and torch.equal(ccnts[k], ccnts["x86"]), k
        # (inside a call's count the signals agree; past it the words are unspecified)
        for s, m in zip(cs[:64].tolist(), cnts["x86"][:64].tolist()):
            assert torch.equal(sigs[k][s:s + m], sigs["x86"][s:s + m]), k
    res = {"shape": [a.programs, a.calls, a.pcs], "walk": a.walk, "reps": a.reps, "pcs": n,
           "cover_tile": _lib.SYZSIG_COVER_TILE, "lib": os.path.basename(_lib.LIB_PATH),
           "signals": int(cnts["x86"].to(torch.int64).sum().item()),
           "cover_survivors": int(ccnts["x86"].to(torch.int64).sum().item())}
    for k in variants:
        res[k] = {"edge_derive": summary(derive[k]), "edge_cover_dedup": summary(cov[k])}
    for k in ("pc32", "u64"):
        for what in ("edge_derive", "edge_cover_dedup"):
            res[k][what]["over_x86"] = round(res[k][what]["median_ms"] / res["x86"][what]["median_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
