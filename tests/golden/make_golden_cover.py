"""Generate the cover-output golden vectors from the REFERENCE executor itself.

Run in the build container (needs /root/reference and `make -C oracle ref`):
    python tests/golden/make_golden_cover.py [trace set names]
Inputs are synthetic KCOV traces; expected outputs are the per-call cover lists
written by the reference's own write_coverage_signal with flag_collect_cover
(executor/executor.h:514-527: std::sort + std::unique under flag_dedup_cover,
truncation to u32), compiled from its sources by oracle/Makefile and run in
the harness's cover mode.  Every trace set is written twice, once per value of
flag_dedup_cover: tests/golden/cover/<set>_dedup<0|1>.npz, plain arrays (load
with allow_pickle=False):
  pcs u64[], call_start u64[], call_len u32[], call_failed u8[], prog_call u32[], dedup u8 (scalar)
  exp_cover u32[] (call c's list at call_start[c]..+exp_cover_cnt[c]; 0 elsewhere),
  exp_cover_cnt u32[], exp_completed u32[]
`abort` also holds the raw output regions as the executor wrote them (signal and
cover lists, executor.h:566-604): regions u32[], region_off u64[nprog + 1].
`big` is the trace of ../executor_big.npz (one call of kCoverSize - 1 PCs); its
files hold no pcs / call arrays of their own, the tests take them from there.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import oracle as O  # noqa: E402
from syzkaller_amd import _lib, synth  # noqa: E402
from make_golden import pack, synth_programs  # noqa: E402

T = _lib.SYZSIG_COVER_TILE
HI = np.uint64(0xFFFFFFFF00000000)
LO, END = 0x80000000, 0xFF000000  # cover_check's range, low words (executor_linux.cc:196-204)
LENGTHS = [0, 1, 2, T - 1, T, T + 1, 2 * T + 3]
KINDS = ["equal", "asc", "desc", "dups", "span"]


def contents(kind, n, rng):
    """A call's PCs.  Long calls draw from small pools, so the fixture compresses."""
    if kind == "equal":
        low = np.full(n, 0x81000010, np.uint64)
    elif kind == "asc":  # already sorted, distinct
        low = LO + 3 * np.arange(n, dtype=np.uint64)
    elif kind == "desc":  # reverse-sorted, distinct
        low = END - 1 - 5 * np.arange(n, dtype=np.uint64)
    elif kind == "dups":  # about 70 % duplicates
        low = 0x81000000 + 5 * rng.integers(0, max(1, int(0.3 * n)), n).astype(np.uint64)
    else:  # "span": both bounds of cover_check and a pool between them
        pool = np.concatenate([[LO, END - 1], rng.integers(LO, END, 997)]).astype(np.uint64)
        low = pool[rng.integers(0, pool.size, n)]
        low[: min(n, 2)] = [END - 1, LO][: min(n, 2)]
    return HI | low.astype(np.uint64)


def lengths_programs():
    """One program per length, one call per content kind; every third call failed
    (its cover record is written all the same, executor.h:566-599)."""
    rng = np.random.default_rng(31)
    progs, k = [], 0
    for n in LENGTHS:
        prog = []
        for kind in KINDS:
            prog.append((k % 3 == 1, contents(kind, n, rng)))
            k += 1
        progs.append(prog)
    return progs


def abort_programs():
    """Programs aborted by an out-of-range PC (cover_check -> doexit(0) in the
    signal loop, executor.h:502-503): seeded ones, and by hand the two values
    next to cover_check's bounds, in the first call, in a later one, as the
    first and as the last PC of a call."""
    progs = synth_programs(synth.synth_default(bad_pc_ppm=700), 8, 6, (0, 1500), 33, prog_base=900)
    rng = np.random.default_rng(34)
    below, above = np.uint64(0xFFFFFFFF7FFFFFFF), np.uint64(0xFFFFFFFFFF000000)

    def ok(n):
        return contents("dups", n, rng)

    def bad_at(n, i, v):
        p = ok(n)
        p[i] = v
        return p
    progs.append([(False, bad_at(40, 0, below)), (False, ok(30))])
    progs.append([(False, ok(T + 9)), (True, ok(70)), (False, bad_at(50, 49, above)), (False, ok(20))])
    progs.append([(False, ok(5)), (False, bad_at(T + 2, T + 1, below)), (False, ok(5))])
    progs.append([(False, ok(64)), (False, np.array([HI | np.uint64(LO), HI | np.uint64(END - 1)], np.uint64)),
                  (False, bad_at(1, 0, above))])
    return progs


def big_programs():
    with np.load(os.path.join(HERE, "executor_big.npz"), allow_pickle=False) as f:
        assert f["call_len"].tolist() == [262143]
        return [[(bool(f["call_failed"][0]), f["pcs"])]]


def expected(fx, programs, dedup, raw=False):
    ref, inf = O.run_reference_executor(programs, mode="cover", dedup=dedup, info=True)
    assert not any(inf["status"])  # an abort is doexit(0)
    cover = np.zeros(fx["pcs"].size, np.uint32)
    cnt = np.zeros(fx["call_len"].size, np.uint32)
    comp = np.zeros(len(programs), np.uint32)
    for p, (completed, calls) in enumerate(ref):
        comp[p] = completed
        for idx, _e, _sigs, cov in calls:
            c = int(fx["prog_call"][p]) + idx
            s = int(fx["call_start"][c])
            assert cov.size <= int(fx["call_len"][c])
            cover[s: s + cov.size] = cov
            cnt[c] = cov.size
    out = dict(dedup=np.uint8(dedup), exp_cover=cover, exp_cover_cnt=cnt, exp_completed=comp)
    if raw:
        regions = O.run_reference_executor(programs, raw=True, mode="cover", dedup=dedup)
        out["regions"] = np.concatenate(regions)
        out["region_off"] = np.concatenate([[0], np.cumsum([r.size for r in regions])]).astype(np.uint64)
    return out


def main(only=None):
    sets = {"lengths": lengths_programs, "abort": abort_programs, "big": big_programs}
    os.makedirs(os.path.join(HERE, "cover"), exist_ok=True)
    for name, make in sets.items():
        if only and name not in only:
            continue
        programs = make()
        fx = pack(programs)
        for dedup in (0, 1):
            out = dict(fx)
            out.update(expected(fx, programs, dedup, raw=name == "abort"))
            if name == "big":  # the trace lives in executor_big.npz
                out = {k: v for k, v in out.items() if k not in fx}
            path = os.path.join(HERE, "cover", f"{name}_dedup{dedup}.npz")
            np.savez_compressed(path, **out)
            print(f"{name}_dedup{dedup}: {len(programs)} programs, {fx['call_len'].size} calls, {fx['pcs'].size} PCs, "
                  f"{int(out['exp_cover_cnt'].sum())} cover words, completed {out['exp_completed'].tolist()}, "
                  f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:] or None)
