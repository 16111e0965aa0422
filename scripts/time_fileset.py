#!/usr/bin/env python3
"""Time of syzsig_file_set_dev -- fileSet and the per-file Coverage of
syz-manager/cover.go:129-193 -- beside two host versions of the same work, in
the same process.

    python scripts/time_fileset.py                       # 10^3 .. 3*10^6 frames
    python scripts/time_fileset.py --frames 1000 100000  # chosen sizes

The frames are synthetic and stand in PC order, as symbolize returns them: a
third covered, two thirds uncovered; one function per --per-func frames and one
file per --per-file frames (2*10^5 functions and 2*10^4 files at 3*10^6 frames,
the kernel's own proportions); a function's frames are contiguous and lie in
its file, except one in ten, which is inlined from a header drawn from a Zipf
distribution; a fifth of the functions have no covered frame, so their
uncovered frames are dropped.  The numpy version packs (file, key) into one
word, takes np.unique and drops an uncovered entry behind its line's covered
one; the plain-Python version is tests/fileset_ref.py (up to --py-max frames:
it is an interpreter's loop).  Device times are the spans the library times
itself (syzsig_ctx_last_ms), medians of --reps runs after one warm-up; host
times are one run each.  Results are compared exactly.  Prints one JSON line.
Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return round((time.perf_counter() - t0) * 1e3, 3), r


def make_frames(rng, n, nfiles, nfuncs, pool):
    """n frames in PC order over the functions of `pool` (ascending ids)"""
    fn = np.sort(pool[rng.integers(0, pool.size, size=n)])
    fl = (fn.astype(np.int64) * nfiles // nfuncs).astype(np.uint32)  # a file holds neighbouring functions
    inl = rng.random(n) < 0.1
    fl[inl] = (np.minimum(rng.zipf(1.3, int(inl.sum())), nfiles) - 1).astype(np.uint32)
    ln = (fn.astype(np.int64) % 97 * 40 + rng.integers(1, 60, size=n)).astype(np.int32)
    ln[rng.random(n) < 0.0005] = 0  # addr2line's ?:0
    return fl, ln, fn.astype(np.uint32)


def numpy_file_set(cov, unc, nfiles, nfuncs, nlines):
    have = np.zeros(nfuncs, bool)
    have[cov[2]] = True
    keep = have[unc[2]]

    def keys(fl, ln, bit):
        return (fl.astype(np.uint64) << np.uint64(33)) | ((ln.view(np.uint32) ^ np.uint32(1 << 31)).astype(np.uint64)
                                                          << np.uint64(1)) | np.uint64(bit)
    k = np.unique(np.concatenate([keys(cov[0], cov[1], 0), keys(unc[0][keep], unc[1][keep], 1)]))
    first = np.ones(k.size, bool)
    first[1:] = (k[1:] >> np.uint64(1)) != (k[:-1] >> np.uint64(1))
    k = k[first]
    fl = (k >> np.uint64(33)).astype(np.int64)
    line = (((k >> np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ np.uint32(1 << 31)).view(np.int32)
    covered = (k & np.uint64(1)) == 0
    off = np.zeros(nfiles + 1, np.int64)
    np.cumsum(np.bincount(fl, minlength=nfiles), out=off[1:])
    within = line.astype(np.int64) <= nlines.astype(np.int64)[fl]
    head_ok = np.zeros(nfiles, bool)
    nz = np.flatnonzero(np.diff(off))
    head_ok[nz] = line[off[nz]] >= 1
    shown = np.bincount(fl, weights=within, minlength=nfiles).astype(np.int64) * head_ok
    coverage = np.bincount(fl, weights=within & covered, minlength=nfiles).astype(np.int64) * head_ok
    return int(keep.sum()), off, line, covered, shown, coverage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1000, 10000, 100000, 1000000, 3000000])
    ap.add_argument("--per-func", type=int, default=15)
    ap.add_argument("--per-file", type=int, default=150)
    ap.add_argument("--py-max", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from syzkaller_amd import report
    from syzkaller_amd.device import Device
    from tests import fileset_ref as R

    dev = Device(0)
    dev.L.syzsig_ctx_set_timing(dev.eng.h, 1)
    rows = []
    for n in a.frames:
        rng = np.random.default_rng(1)
        nfuncs, nfiles = max(n // a.per_func, 8), max(n // a.per_file, 4)
        covered_funcs = np.flatnonzero(rng.random(nfuncs) < 0.8)
        cov = make_frames(rng, n // 3, nfiles, nfuncs, covered_funcs)
        unc = make_frames(rng, n - n // 3, nfiles, nfuncs, np.arange(nfuncs))
        nlines = rng.integers(0, 97 * 40 + 60, size=nfiles).astype(np.uint32)
        fr = report.Frames(dev, tuple(torch.from_numpy(x.view(np.int32)) for x in cov),
                           tuple(torch.from_numpy(x.view(np.int32)) for x in unc), files=nfiles, funcs=nfuncs)
        nl = torch.from_numpy(nlines.view(np.int32)).to(dev.dev)
        t, res = [], None
        for _ in range(a.reps + 1):
            res = report.file_set(fr, nl)
            t.append(dev.L.syzsig_ctx_last_ms(dev.eng.h))
        st = report.file_set_stats(dev)
        row = {"frames": n, "ncov": int(cov[0].size), "nunc": int(unc[0].size), "files": nfiles, "funcs": nfuncs,
               "dev_ms": round(float(np.median(t[1:])), 4), "kept": st[0], "long_files": st[1], "merge_passes": st[2],
               "entries": st[3]}
        row["numpy_ms"], (kept, off, line, covered, shown, coverage) = host_ms(
            lambda: numpy_file_set(cov, unc, nfiles, nfuncs, nlines))
        d_off, d_line, d_cov, d_shown, d_coverage = (x.cpu().numpy() for x in res)
        assert kept == st[0] and np.array_equal(d_off, off) and np.array_equal(d_line, line)
        assert np.array_equal(d_cov.astype(bool), covered)
        assert np.array_equal(d_shown, shown) and np.array_equal(d_coverage, coverage)
        row["python_ms"] = None
        if n <= a.py_max:
            cf = list(zip(cov[0].tolist(), cov[1].tolist(), cov[2].tolist()))
            uf = list(zip(unc[0].tolist(), unc[1].tolist(), unc[2].tolist()))
            nll = nlines.tolist()

            def plain():
                fs = R.file_set(cf, uf)
                return fs, {f: R.walk(nll[f], lst) for f, lst in fs.items()}
            row["python_ms"], (fs, wk) = host_ms(plain)
            assert len(fs) == int(np.count_nonzero(np.diff(off)))
            for f, lst in fs.items():
                assert [x[0] for x in lst] == line[off[f]:off[f + 1]].tolist()
                assert [x[1] for x in lst] == covered[off[f]:off[f + 1]].tolist()
                assert wk[f] == (int(shown[f]), int(coverage[f]))
        rows.append(row)
    print(json.dumps({"tile": report._lib.SYZSIG_FILESET_TILE, "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
