#!/usr/bin/env python3
"""Time of the coverage-report calls -- syzsig_call_cover_dev,
syzsig_report_pcs_dev, syzsig_uncovered_pcs_dev (syz-manager/html.go and
cover.go's corpus-wide loops) -- beside a host version of the same work, in
the same process.

    python scripts/time_report.py                      # 10^5 inputs, 3500 calls, 10^6 PCs, 2*10^5 symbols
    python scripts/time_report.py --scales 0.001 0.01  # smaller corpora, to see where the host wins

The corpus is synthetic: --inputs inputs of about --cover PCs each drawn from
--pcs distinct PCs, calls Zipf-distributed over --ncalls ids (one call owns
most of the corpus, as mmap does); --syms abutting functions with --sites call
sites spread over them.  The host version is numpy where the work vectorises
(np.unique over call << 32 | pc; the map and np.sort) and tests/report_ref.py,
the line-by-line restatement, for uncoveredPcsInFuncs, over the first
--host-pcs PCs of the cover (the device is timed on the same PCs, and on all).
Device times are the spans the library times itself (syzsig_ctx_last_ms),
medians of --reps runs after one warm-up.  Results are compared exactly.
Prints one JSON line.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(reps, fn, lib_ms):
    t = []
    for _ in range(reps + 1):
        fn()
        t.append(lib_ms())
    return round(float(np.median(t[1:])), 4)


def host_ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return round((time.perf_counter() - t0) * 1e3, 3), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=100000)
    ap.add_argument("--ncalls", type=int, default=3500)
    ap.add_argument("--pcs", type=int, default=1000000)
    ap.add_argument("--cover", type=int, default=50)
    ap.add_argument("--syms", type=int, default=200000)
    ap.add_argument("--sites", type=int, default=2000000)
    ap.add_argument("--host-pcs", type=int, default=100000)
    ap.add_argument("--scales", type=float, nargs="*", default=[0.001, 0.01, 0.1, 1.0])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from syzkaller_amd import report
    from syzkaller_amd.device import Device
    from tests import report_ref as R

    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    lib_ms = lambda: dev.L.syzsig_ctx_last_ms(dev.eng.h)  # noqa: E731
    base, rows = 0xFFFFFFFF, []
    for sc in a.scales:
        rng = np.random.default_rng(1)
        n, npcs = max(int(a.inputs * sc), 1), max(int(a.pcs * sc), 16)
        nsym, nsites = max(int(a.syms * sc), 1), max(int(a.sites * sc), 4)
        # sites 8 bytes apart from 0x81000000 on; PC universe = a subset of the sites' return addresses
        site = 0x81000000 + 8 * np.arange(nsites, dtype=np.uint64)
        universe = (site[rng.choice(nsites, size=min(npcs, nsites), replace=False)] + 5).astype(np.uint32)
        lens = rng.integers(0, 2 * a.cover + 1, n)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        cov = universe[rng.integers(0, universe.size, int(off[-1]))]
        call = (np.minimum(rng.zipf(1.3, n), a.ncalls) - 1).astype(np.uint32)
        corpus = report.Corpus.__new__(report.Corpus)
        corpus.dev, corpus.calls, corpus.sigs = dev, [str(c) for c in range(a.ncalls)], list(range(n))
        corpus.host_call = call
        corpus.off = torch.from_numpy(off).to(dev.dev)
        corpus.cov = torch.from_numpy(cov.view(np.int32)).to(dev.dev)
        corpus.call = torch.from_numpy(call.view(np.int32)).to(dev.dev)
        row = {"scale": sc, "inputs": n, "total_pcs": int(off[-1]), "symbols": nsym, "sites": nsites}

        # 1: per-call unions and the whole union
        res = {}
        row["call_cover_ms"] = med(a.reps, lambda: res.update(r=report.call_cover(corpus, want_all=True)), lib_ms)
        row["call_cover_stats"] = report.report_stats(dev)[:2]

        def host_cc():
            key = np.unique((np.repeat(call.astype(np.uint64), lens) << np.uint64(32)) | cov)
            return np.bincount(call, minlength=a.ncalls), key, np.unique(cov)
        row["call_cover_host_ms"], (cnt, key, union) = host_ms(host_cc)
        count, _, d_off, d_cov, d_all = res["r"]
        assert np.array_equal(count.cpu().numpy(), cnt) and int(d_off[-1]) == key.size
        assert np.array_equal(d_cov[: key.size].cpu().numpy().view(np.uint32), key.astype(np.uint32))
        assert np.array_equal(d_all.cpu().numpy().view(np.uint32), union)

        # 2: RestorePC, previousInstructionPC, sort
        perm = rng.permutation(union.size)  # a map's iteration order
        d_pcs = torch.from_numpy(union[perm].view(np.int32)).to(dev.dev)
        row["report_pcs_n"] = int(union.size)
        row["report_pcs_ms"] = med(a.reps, lambda: res.update(p=report.report_pcs(dev, d_pcs, base, "amd64")), lib_ms)

        def host_rp():
            v = (np.uint64(base) << np.uint64(32)) + union[perm].astype(np.uint64) - np.uint64(5)
            return v, np.sort(v)
        row["report_pcs_host_ms"], (order, srt) = host_ms(host_rp)
        assert np.array_equal(res["p"][0].cpu().numpy().view(np.uint64), order)
        assert np.array_equal(res["p"][1].cpu().numpy().view(np.uint64), srt)

        # 3: uncoveredPcsInFuncs over abutting functions
        full = (np.uint64(base) << np.uint64(32)) + site
        cut = np.sort(rng.choice(np.arange(1, nsites), size=min(nsym, nsites) - 1, replace=False))
        start = np.concatenate([full[:1], full[cut]]) - np.uint64(3)
        end = np.concatenate([start[1:], full[-1:] + np.uint64(8)])
        ss, se, ac = (torch.from_numpy(x.view(np.int64)).to(dev.dev) for x in (start, end, full))
        order_t = res["p"][0]
        row["uncovered_npc"] = int(order_t.numel())
        row["uncovered_ms"] = med(a.reps, lambda: res.update(u=report.uncovered_pcs(dev, ss, se, ac, order_t)), lib_ms)
        row["uncovered_stats"] = report.report_stats(dev)[2:]
        k = min(a.host_pcs, order.size)
        sub = order_t[:k].contiguous()
        row["uncovered_sub_npc"] = k
        row["uncovered_sub_ms"] = med(a.reps, lambda: res.update(u=report.uncovered_pcs(dev, ss, se, ac, sub)), lib_ms)
        syms, allc, pcs = list(zip(start.tolist(), end.tolist())), full.tolist(), order[:k].tolist()
        row["uncovered_sub_host_ms"], want = host_ms(lambda: R.uncovered_pcs_in_funcs(syms, allc, pcs))
        assert res["u"].cpu().numpy().view(np.uint64).tolist() == want
        rows.append(row)
    print(json.dumps({"ncalls": a.ncalls, "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
