#!/usr/bin/env python3
"""Time of syzsig_calc_prios_dev plus syzsig_choice_table_dev
(target.CalculatePriorities and BuildChoiceTable, prog/prio.go) beside a
vectorised numpy host version (np.add.at over the enumerated pairs, then row
operations), in the same process.

    python scripts/time_prio.py                     # 10^5 programs over N = 3500
    python scripts/time_prio.py --splits 0 1024 -1  # thresholds to compare (-1: never split)

The corpus is synthetic: --n programs of 1 to --maxlen calls, the first call of
every program id 0 (the mmap of a real corpus), the others Zipf-distributed
over the remaining ids.  For the prefixes in --sizes and each threshold in
--splits: the wall time of the two calls (both end synchronised), the spans the
library times itself (syzsig_ctx_last_ms), and syzsig_prio_stats; once per
size the host version.  Medians of --reps runs after one warm-up (the host
version: --host-reps runs).  The device result is compared with the host's bit
for bit.  Prints one JSON line.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus(n, ncalls, maxlen, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, maxlen + 1, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ids = (np.minimum(rng.zipf(1.2, int(off[-1])), ncalls - 1)).astype(np.int64)  # 1 .. N - 1
    ids[off[:-1]] = 0
    return off, ids


def host_counts(off, ids, ncalls):
    """count[a][b] over every ordered pair of positions of every program: the
    programs of one length as a matrix, its pairs enumerated by broadcasting."""
    cnt = np.zeros((ncalls, ncalls), np.int64)
    lens = np.diff(off)
    for ln in np.unique(lens):
        if ln == 0:
            continue
        m = ids[off[:-1][lens == ln][:, None] + np.arange(ln)[None, :]]
        a = np.broadcast_to(m[:, :, None], (m.shape[0], ln, ln)).ravel()
        b = np.broadcast_to(m[:, None, :], (m.shape[0], ln, ln)).ravel()
        np.add.at(cnt, (a, b), 1)
    return cnt


def wall(reps, fn, warm=1):
    t = []
    for _ in range(reps + warm):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[warm:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--ncalls", type=int, default=3500)
    ap.add_argument("--maxlen", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 100, 1000, 10000, 100000])
    ap.add_argument("--splits", type=int, nargs="*", default=[0, -1])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    import torch

    from syzkaller_amd import _lib, prio
    from syzkaller_amd.device import Device
    from tests import prio_ref as R

    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    N = a.ncalls
    off, ids = corpus(a.n, N, a.maxlen)
    out = torch.empty((N, N), dtype=torch.float32, device=dev.dev)
    run = torch.empty((N, N), dtype=torch.int32, device=dev.dev)
    rows = []
    for n in [s for s in a.sizes if s <= a.n]:
        o, i = off[: n + 1], ids[: off[n]]
        d_off = torch.from_numpy(o.copy()).to(dev.dev)
        d_ids = torch.from_numpy(i.astype(np.int32)).to(dev.dev)
        row = {"n": n, "calls": int(o[-1]), "pairs": int((np.diff(o) ** 2).sum()), "device": []}
        for split in a.splits:
            sp = 1 << 40 if split < 0 else split
            lib_p, lib_t = [], []

            def run_dev():
                prio.calculate_priorities(dev, (d_off, d_ids), N, split=sp, out=out)
                lib_p.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
                prio.ChoiceTable.build(dev, out, None, N, out=run)
                lib_t.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
            ms = wall(a.reps, run_dev)
            st = prio.prio_stats(dev)
            row["device"].append({"split": split if split else _lib.SYZSIG_PRIO_SPLIT, "wall_ms": round(ms, 4),
                                  "calc_prios_ms_library": round(float(np.median(lib_p[1:])), 4),
                                  "choice_table_ms_library": round(float(np.median(lib_t[1:])), 4),
                                  "rows_whole": st[0], "rows_split": st[1], "slices": st[2]})
        host = {}

        def run_host():
            host["p"] = R.normalize_prio(R.counts_to_f32(host_counts(o, i, N)))
            host["run"] = R.build_choice_table_fast(host["p"], None, N)
        row["host_ms"] = round(wall(a.host_reps, run_host, warm=0), 2)
        t0 = time.perf_counter()
        host_counts(o, i, N)
        row["host_counts_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        gp, hp = out.cpu().numpy(), host["p"]
        assert np.array_equal(np.isnan(gp), np.isnan(hp)) and \
            np.array_equal(gp.view(np.uint32)[~np.isnan(gp)], hp.view(np.uint32)[~np.isnan(hp)]), "prios differ"
        assert np.array_equal(run.cpu().numpy(), host["run"]), "choice tables differ"
        row["host_over_device"] = round(row["host_ms"] / row["device"][0]["wall_ms"], 2)
        rows.append(row)
    print(json.dumps({"ncalls": N, "maxlen": a.maxlen, "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
