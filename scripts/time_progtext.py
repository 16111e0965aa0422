#!/usr/bin/env python3
"""Time of syzsig_prog_calls_dev (the heads of program-text lines, csrc/calls.hip)
beside the restated Python loop (tests/progtext_ref.py) and a numpy line
splitter (np.flatnonzero(data == 10)), in the same process.

    python scripts/time_progtext.py              # 10^5 programs of 5 to 30 calls
    python scripts/time_progtext.py --n 20000

The corpus is generated text in the shape Serialize writes,
`rN = name$variant(0x..., &(0x7f0000000000)=...)`, over --ncalls names.  For
each mode: the wall time of the sizing call and of the full call into a given
output (both end synchronised), the span the library times itself
(syzsig_ctx_last_ms), syzsig_prog_calls_stats, and the fraction of a plain
device copy's bandwidth (syzsig_copy_bw_dev) that one read of the text in the
library's span comes to.  The restated loop runs once over the first
--ref-n programs and is scaled; the device result is compared with it exactly
on that prefix.  Medians of --reps runs after one warm-up.  Prints one JSON
line.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus(n, names, seed=1):
    """n programs of 5 to 30 calls; the lines are drawn from a pool, so that building 10^6 lines stays quick"""
    rng = np.random.default_rng(seed)
    pool = []
    for k in range(20000):
        nm = names[int(rng.integers(0, len(names)))]
        head = (b"r%d = " % (k % 40) if k % 3 else b"") + nm
        pool.append(head + b"(0x%x, &(0x7f0000000000)={0x%x, 0x0, @void, {0x%x, 0x%x}}, 0x%x, &(0x7f0000001000)=\"%s\")\n"
                    % (int(rng.integers(0, 1 << 31)), int(rng.integers(0, 1 << 16)), k, k * 7, int(rng.integers(0, 4096)),
                       b"%02x" % (k % 256) * int(rng.integers(0, 24))))
    lens = rng.integers(5, 31, n)
    pick = rng.integers(0, len(pool), int(lens.sum()))
    progs, at = [], 0
    for ln in lens:
        progs.append(b"".join(pool[int(j)] for j in pick[at:at + ln]))
        at += ln
    return progs


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
    ap.add_argument("--ref-n", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from syzkaller_amd import progtext
    from syzkaller_amd.device import Device
    from tests import progtext_ref as R

    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    names = [b"sys%d$v%d" % (i // 7, i % 7) for i in range(a.ncalls)]
    tab = progtext.CallTable(dev, names)
    progs = corpus(a.n, names)
    blob = b"".join(progs)
    off = np.zeros(a.n + 1, np.int64)
    np.cumsum([len(p) for p in progs], out=off[1:])
    data = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev.dev)
    d_off = torch.from_numpy(off).to(dev.dev)
    enabled = np.ones(a.ncalls, np.uint8)
    enabled[::50] = 0
    res = {"programs": a.n, "bytes": len(blob), "modes": {}}
    src = torch.ones((1 << 30) // 8, dtype=torch.int64, device=dev.dev)
    dst = torch.empty_like(src)
    bw_ms = float(np.median([dev.copy_bw(dst, src, 1 << 30) for _ in range(a.reps + 1)][1:]))
    bw = 2 * (1 << 30) / (bw_ms * 1e-3) / 1e9  # GB/s of a plain device copy over 1 GiB
    del src, dst
    res["copy_GBps"] = round(bw, 1)
    for name, fn, mode in (("deserialize", progtext.prog_calls, 0), ("callset", progtext.call_set, 1)):
        out = fn(dev, tab, (data, d_off), enabled)
        ids = torch.empty(out[1].numel(), dtype=torch.int32, device=dev.dev)
        lib = []

        def full():
            fn(dev, tab, (data, d_off), enabled, ids=ids)
            lib.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
        full_ms = wall(a.reps, full)
        sizing_ms = wall(a.reps, lambda: fn(dev, tab, (data, d_off), enabled, sizing=True))
        st = progtext.stats(dev)
        lib_ms = float(np.median(lib[1:]))
        # the restated loop on a prefix, compared exactly
        m = min(a.ref_n, a.n)
        t0 = time.perf_counter()
        eoff, eids, est, eerr, eflag = R.batch(progs[:m], names, mode, enabled.tolist())
        ref_ms = (time.perf_counter() - t0) * 1e3
        assert out[0][: m + 1].cpu().tolist() == eoff and out[1][: eoff[-1]].cpu().tolist() == eids, name
        assert out[2][:m].cpu().tolist() == est, name
        res["modes"][name] = {
            "calls": int(out[1].numel()), "full_call_wall_ms": round(full_ms, 4), "sizing_call_wall_ms": round(sizing_ms, 4),
            "library_ms": round(lib_ms, 4), "lines": st[0], "skipped": st[1], "window": st[2], "long": st[3],
            "text_GBps_in_library_span": round(len(blob) / lib_ms / 1e6, 1),
            "fraction_of_copy_bw": round(len(blob) / lib_ms / 1e6 / bw, 4),
            "ref_loop_ms_scaled": round(ref_ms * a.n / m, 1), "ref_over_device": round(ref_ms * a.n / m / full_ms, 1)}
    h = np.frombuffer(blob, np.uint8)
    res["numpy_flatnonzero_ms"] = round(wall(3, lambda: np.flatnonzero(h == 10), warm=0), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
