#!/usr/bin/env python3
"""Time of one Manager.NewInput batch (syzsig_manager_new_input_batch) beside
the per-input way of doing its acceptance -- per input syzsig_deserialize +
syzsig_diff + syzsig_merge + syzsig_cover_merge, which has no per-key merge --
in one process.

    python scripts/time_new_input.py                  # the manager-like shape and the hot-element shape
    python scripts/time_new_input.py --shapes manager --inputs 512

Shapes: `manager` = --inputs rows x ~--entries signal entries x --pcs cover PCs
against a --corpus element corpusSignal, --keys keys; `hot` = 3000 rows of ~20
entries that all carry one element (acceptance takes the sequential fallback).
Times are HIP events around the call (the calls end synchronised, so they
span its host round trips), the median of --reps runs after one warm-up, each
run on fresh clones of the sets.  Algorithmic bytes: 5 B per entry + 8 B per
distinct element + 4 B per PC in and out, beside a plain device copy's
bandwidth (syzsig_copy_bw_dev).  Prints one JSON line per shape.  Needs the GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from syzkaller_amd import signal as S  # noqa: E402
from syzkaller_amd.device import Device  # noqa: E402


def achievable_bw(dev, nbytes=1 << 30, reps=5):
    src = torch.ones(nbytes // 8, dtype=torch.int64, device=dev.dev)
    dst = torch.empty_like(src)
    ms = [dev.copy_bw(dst, src, nbytes) for _ in range(reps + 1)][1:]
    return 2 * nbytes / (float(np.median(ms)) * 1e-3) / 1e9


def make_shape(name, a, rng):
    if name == "hot":
        K, n, c, U, nkeys, corpus = 3000, 20, 16, 1 << 20, 1000, 100_000
    else:
        K, n, c, U, nkeys, corpus = a.inputs, a.entries, a.pcs, 1 << 26, a.keys, a.corpus
    rows = []
    for _ in range(K):
        m = int(rng.integers(n * 3 // 4, n + 1))
        e = rng.integers(0, U, size=m).astype(np.uint32)
        if name == "hot":
            e[-1] = 7
        p = rng.integers(0, 4, size=m).astype(np.int8)
        rows.append((int(rng.integers(0, nkeys)), S.Serial(e, p), rng.integers(0, 1 << 24, size=c).astype(np.uint32)))
    ce = np.unique(rng.integers(0, U, size=corpus).astype(np.uint32))
    return rows, nkeys, S.Serial(ce, rng.integers(0, 4, size=ce.size).astype(np.int8))


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):
        prep = fn(None)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(prep)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms[1:])), out


def run_shape(dev, name, a, bw):
    rng = np.random.default_rng(1)
    rows, nkeys, corpus = make_shape(name, a, rng)
    eng = dev.eng
    cs0 = corpus.Deserialize(eng)

    def fresh():
        return cs0.clone(), S.Cover(eng)

    def batch(prep):
        if prep is None:
            return fresh()
        cs, cc = prep
        acc, new, entries = S.manager_new_input(cs, cc, rows, nkeys, eng)
        return int(acc.sum()), len(entries), sum(c.size for _, c in entries.values()), S.new_input_stats(eng)

    def loop(prep):
        if prep is None:
            return fresh()
        cs, cc = prep
        L, n_acc = eng.L, 0
        sh = ctypes.c_void_p(cs.handle.value)
        for _, ser, cov in rows:
            d, nw = ctypes.c_void_p(), ctypes.c_void_p()
            S.check(L.syzsig_deserialize(eng.h, S._ptr(ser.Elems), ser.Elems.size, S._ptr(ser.Prios), ser.Prios.size,
                                         ctypes.byref(d)))
            S.check(L.syzsig_diff(eng.h, sh, d, ctypes.byref(nw)))
            if not L.syzsig_empty(nw):
                S.check(L.syzsig_merge(eng.h, ctypes.byref(sh), d))
                cc.Merge(cov)
                n_acc += 1
            L.syzsig_set_free(d)
            L.syzsig_set_free(nw)
        return n_acc

    b_ms, (n_acc, n_touched, c_out, stats) = timed(batch, a.reps)
    l_ms, l_acc = timed(loop, a.reps)
    n = sum(r[1].Elems.size for r in rows)
    c_in = sum(r[2].size for r in rows)
    distinct = int(np.unique(np.concatenate([r[1].Elems for r in rows])).size)
    nbytes = 5 * n + 8 * distinct + 4 * (c_in + c_out)
    gbps = nbytes / (b_ms * 1e-3) / 1e9
    return {"shape": name, "inputs": len(rows), "keys": nkeys, "entries": n, "pcs": c_in, "corpus_signal": len(cs0),
            "accepted": n_acc, "loop_accepted": l_acc, "touched_keys": n_touched, "paths": stats, "reps": a.reps,
            "batch_ms": round(b_ms, 3), "per_input_loop_ms": round(l_ms, 3), "loop_over_batch": round(l_ms / b_ms, 2),
            "entries_per_s": round(n / (b_ms * 1e-3)), "algorithmic_bytes": nbytes, "achieved_GBps": round(gbps, 2),
            "copy_bw_GBps": round(bw, 1), "fraction_of_copy_bw": round(gbps / bw, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="manager,hot")
    ap.add_argument("--inputs", type=int, default=4096)
    ap.add_argument("--entries", type=int, default=2040)
    ap.add_argument("--pcs", type=int, default=4096)
    ap.add_argument("--keys", type=int, default=1024)
    ap.add_argument("--corpus", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = Device(0)
    bw = achievable_bw(dev)
    for name in a.shapes.split(","):
        print(json.dumps(run_shape(dev, name, a, bw)), flush=True)


if __name__ == "__main__":
    main()
