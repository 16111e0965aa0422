#!/usr/bin/env python3
"""Time of syzsig_hash_dev (pkg/hash over a batch) and syzsig_sigset_add_dev
(addInputToCorpus's corpusHashes check, fuzzer.go:447-452) beside a hashlib.sha1
loop and a Python set on one core, in the same process.

    python scripts/time_hash.py              # 10^5 programs, LDS staging on
    python scripts/time_hash.py --stage 0    # the same with every wave reading global memory directly

The corpus is synthetic: --n program-like byte strings (serialized syscalls,
printable text) whose lengths are lognormal with median 400 bytes and sigma
0.9, clipped to [16, 16384] -- a few calls to a few hundred, the shape of a
syzkaller corpus; a tenth of them repeat an earlier one.  For the prefixes in
--sizes: the device hash (wall time of the call, which ends synchronised, and
the span the library times itself, syzsig_ctx_last_ms), the hashlib loop, and
the same for the set insertion of the resulting Sigs into a set that already
holds the first half.  Medians of --reps runs after one warm-up.  The bytes of
the messages over the device time stand beside the achievable bandwidth of a
plain device copy.  Prints one JSON line.  Needs the GPU.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus(n, seed=1):
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.lognormal(np.log(400), 0.9, n), 16, 16384).astype(np.int64)
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789(){}&=$, _x\n", np.uint8)
    progs = [alphabet[rng.integers(0, alphabet.size, int(k))].tobytes() for k in lens]
    for i in rng.integers(1, n, n // 10):  # repeats of an earlier program
        progs[i] = progs[int(rng.integers(0, i))]
    return progs


def wall(reps, fn):
    t = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 1024, 16384, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage", type=int, default=1)
    a = ap.parse_args()
    os.environ["SYZSIG_HASH_STAGE"] = str(a.stage)  # read when the context is created
    import torch

    from syzkaller_amd import _lib, hashing
    from syzkaller_amd.device import Device
    from time_comps import achievable_bw

    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    bw = achievable_bw(dev)
    progs = corpus(a.n)
    rows = []
    for n in [s for s in a.sizes if s <= a.n]:
        p = progs[:n]
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(x) for x in p], out=off[1:])
        data = torch.from_numpy(np.frombuffer(b"".join(p), np.uint8).copy()).to(dev.dev)
        doff = torch.from_numpy(off).to(dev.dev)
        out = torch.empty((n, 20), dtype=torch.uint8, device=dev.dev)
        lib = []

        def run_hash():
            hashing.hash_batch(dev, data, doff, out=out)
            lib.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
        ms_dev = wall(a.reps, run_hash)
        stats = hashing.hash_stats(dev)
        ref = []
        ms_cpu = wall(a.reps, lambda: ref.__setitem__(slice(None), [hashlib.sha1(x).digest() for x in p]))
        assert out.cpu().numpy().tobytes() == b"".join(ref), "device and hashlib disagree"
        half = hashing._rows(out)[: n // 2].contiguous()
        lib_add = []

        def run_add():
            s = hashing.SigSet(dev)
            s.add(half)
            s.add(out)
            lib_add.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))  # the second add's span

        def cpu_add():
            s = set(ref[: n // 2])
            for x in ref:
                if x not in s:
                    s.add(x)
        ms_add, ms_add_cpu = wall(a.reps, run_add), wall(a.reps, cpu_add)
        nbytes = int(off[-1])
        rows.append({"n": n, "bytes": nbytes, "hash_ms": round(ms_dev, 4), "hash_ms_library": round(float(np.median(lib[1:])), 4),
                     "hashlib_ms": round(ms_cpu, 4), "hashlib_over_device": round(ms_cpu / ms_dev, 2),
                     "staged": stats[0], "direct": stats[1], "long": stats[2], "blocks": stats[3],
                     "hash_GBps": round(nbytes / (float(np.median(lib[1:])) * 1e-3) / 1e9, 3),
                     "two_adds_ms": round(ms_add, 4), "second_add_ms_library": round(float(np.median(lib_add[1:])), 4),
                     "python_set_ms": round(ms_add_cpu, 4)})
    print(json.dumps({"stage": a.stage, "stage_bytes": _lib.SYZSIG_HASH_STAGE, "long": _lib.SYZSIG_HASH_LONG,
                      "reps": a.reps, "achievable_bw_GBps": round(bw, 1), "rows": rows}))


if __name__ == "__main__":
    main()
