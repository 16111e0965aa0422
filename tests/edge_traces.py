"""Trace builders for K1+K2 (csrc/edge.hip), chosen for the kernel's own
structure instead of a workload's: dense conflicts at the bin and mark-word
boundaries of K2's rounds, call lengths at the chunk / prefetch-group / buffer
edges of K1, cover_check failures by position, and a batch that makes one
workgroup run several programs.  Plain numpy, deterministic by seed, no GPU:
tests/test_edge_rounds_cpu.py checks their shape with the round restatement
and the oracle, tests/test_gpu_edge.py runs them through the kernel, and
tests/golden/make_golden.py runs two of them through the reference executor
(executor_dense, executor_geometry).

Programs are lists of calls (failed, pcs u64[]) as in make_golden.py.  `gaps`
maps (program, call) to PCs that lie in the flat buffer after that call and
belong to no call (the sparse call_start layout)."""
import functools

import numpy as np

from tests.golden.make_golden import craft_free

M = 8192
PC_BASE = 0xFFFFFFFF81000000

# name -> (homes, craft_free's filler window: at least 1024 slots from every home)
HOME_SETS = {
    # a bin boundary: h & 7 in {5, 6, 7} marks a second bin
    "bin_edge": (list(range(3, 13)), (2048, 6144)),
    # a mark-word boundary (h & 31 >= 29 spills into the next fm1/fm2 word) with a bin boundary
    "word_edge": (list(range(26, 38)), (2048, 6144)),
    # the last mark words (254 -> 255), short of the windows that hold slot 0
    "last_words": (list(range(8156, 8167)), (2048, 6144)),
    # the windows that hold slot 0 (marked whole; word 255 -> 0), without the zero write
    "zero_window": (list(range(M - 8, M)) + list(range(0, 9)), (2048, 6144)),
    # two clusters with the same in-bin offsets in independent bins
    "two_clusters": (list(range(100, 108)) + list(range(4100, 4108)), (5200, 7100)),
}
DENSE_FIXTURE_SEEDS = {"bin_edge": 26, "word_edge": 22, "last_words": 23, "zero_window": 24, "two_clusters": 25}

# chunk = 256 signals, prefetch group = 4 chunks, two buffers = 2048 signals per turn
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2100]
ABORT_POSITIONS = [(1, 0), (64, 63), (65, 64), (256, 255), (257, 256), (1024, 1023), (1025, 1024), (1025, 0),
                   (2049, 2048), (2100, 1500)]
GRID_CAP = 1024  # edge.hip: grid = min(nprog, 256 * 4)


def boundary_homes(homes):
    """The homes whose window crosses a bin (h & 7 >= 5) or a mark word (h & 31 >= 29)."""
    return [h for h in homes if (h & 7) >= 5 or (h & 31) >= 29]


def dense_conflict_programs(homes, nvals=3, nprog=8, seed=0, far=(2048, 6144), ntargets=(40, 600), meta=False):
    """zero_stress_programs for any set of adjacent homes, without sig == 0: a
    fill call that sets each home's slot with probability 0 / 0.5 / 0.9 / 1.0
    (by program), then three calls of ntargets signals drawn from k * 8192 + h,
    h in homes, k in 1..nvals, so that matches, inserts into empty slots and
    forced overwrites of a few repeated values meet in one bin inside one
    256-signal chunk.  With meta: also the target count of every call (None
    for a fill call); the other signals are craft_free's fillers, homed in
    `far`."""
    rng = np.random.default_rng(seed)
    vals = np.array([k * M + h for h in homes for k in range(1, nvals + 1)], np.uint64)
    progs, counts = [], []
    for p in range(nprog):
        dens = [0.0, 0.5, 0.9, 1.0][p % 4]
        fill = [int(rng.integers(1, 6)) * M + h for h in homes if rng.random() < dens]
        calls = [(False, craft_free(fill, seed * 1000 + p * 10, far=far))] if fill else []
        cnt = [None] * len(calls)
        for c in range(3):
            # uneven over the homes, anew for every call: where every home is busy the
            # lanes of a slot's own home hide what its neighbours' marks do
            w = np.repeat(rng.dirichlet(np.full(len(homes), 0.5)), nvals)
            tg = vals[rng.choice(vals.size, int(rng.integers(ntargets[0], ntargets[1] + 1)), p=w / w.sum())]
            calls.append((False, craft_free(tg.tolist(), seed * 1000 + p * 10 + c + 1, far=far)))
            cnt.append(tg.size)
        progs.append(calls)
        counts.append(cnt)
    return (progs, counts) if meta else progs


@functools.lru_cache(maxsize=None)
def dense_set(name, nprog=8, seed=None, meta=False):
    """The programs of one HOME_SETS entry (default: the executor_dense draw)."""
    homes, far = HOME_SETS[name]
    return dense_conflict_programs(homes, nprog=nprog, seed=DENSE_FIXTURE_SEEDS[name] if seed is None else seed,
                                   far=far, meta=meta)


def region_walk(rng, n, entry, region_log2):
    """n PCs of a walk over the 2^region_log2 blocks from `entry` (four
    out-edges per block, back to the entry with probability 1/32): two walks
    of one region share edges, and at region_log2 = 12 its 16384 edges
    overflow the 8192-slot table."""
    wmask = (1 << region_log2) - 1
    r = rng.integers(0, 128, n).tolist()
    x, out = int(rng.integers(0, wmask + 1)), []
    for i in range(n):
        out.append(PC_BASE + 5 * ((entry + x) & 0xFFFFF))
        x = 0 if r[i] >= 124 else (4 * x + 1 + (r[i] & 3)) & wmask
    return np.array(out, np.uint64)


def bad_pc(i):
    """A PC that fails cover_check: below the kernel text, or (odd i) with a
    low half inside it under a wrong high half."""
    return 0x1000 + i if i % 2 == 0 else 0x0000000081000000 + 5 * i


def geometry_programs(seed=31):
    """-> (programs, gaps).  One program per length of LENGTHS: two calls of
    that length over one wide region, so that the second both matches and
    overwrites what the first left; then one program with every length as
    consecutive calls, 1..7 unused PCs between them."""
    rng = np.random.default_rng(seed)
    progs, gaps = [], {}
    for n in LENGTHS:
        entry = int(rng.integers(0, 1 << 20))
        progs.append([(False, region_walk(rng, n, entry, 12)) for _ in range(2)])
    entry = int(rng.integers(0, 1 << 20))
    progs.append([(False, region_walk(rng, n, entry, 12)) for n in LENGTHS])
    for c in range(len(LENGTHS) - 1):
        gaps[(len(progs) - 1, c)] = region_walk(rng, 1 + c % 7, entry, 12)
    return progs, gaps


def abort_position_programs(seed=32):
    """-> (programs, gaps, completed).  For each (len, pos) of ABORT_POSITIONS
    a program of three calls whose middle call (of len PCs) fails cover_check
    at pos (completed = 1), and one whose first call does (completed = 0).
    Last, a program of valid calls whose gaps hold failing PCs: they belong to
    no call, so every call completes."""
    rng = np.random.default_rng(seed)
    progs, gaps, completed = [], {}, []
    for i, (n, pos) in enumerate(ABORT_POSITIONS):
        for at in (1, 0):
            entry = int(rng.integers(0, 1 << 20))
            calls = [region_walk(rng, 96, entry, 10) for _ in range(3)]
            calls[at] = region_walk(rng, n, entry, 10)
            calls[at][pos] = bad_pc(i)
            progs.append([(False, c) for c in calls])
            completed.append(at)
    entry = int(rng.integers(0, 1 << 20))
    lens = [1, 255, 256, 1025, 64]
    progs.append([(False, region_walk(rng, n, entry, 10)) for n in lens])
    for c in range(len(lens)):
        gaps[(len(progs) - 1, c)] = np.array([bad_pc(c + j) for j in range(1 + (3 * c) % 7)], np.uint64)
    completed.append(len(lens))
    return progs, gaps, np.array(completed, np.uint32)


@functools.lru_cache(maxsize=None)
def stride_batch(seed=33):
    """-> (programs, origin).  2100 programs for a grid of GRID_CAP workgroups:
    program p + 1024 is a copy of program p < 1024 and programs 2048..2099 are
    copies of 0..51 (origin[p] = the program p copies, p itself for the first
    1024), so a workgroup runs a program again on the LDS state its first run
    left.  Programs are 2 calls of 24..48 PCs; every tenth is a
    dense_conflict program on homes 3..12, whose copy then meets the table,
    stamps and marks of the same bins."""
    rng = np.random.default_rng(seed)
    homes, far = HOME_SETS["bin_edge"]
    dense = dense_conflict_programs(homes, nprog=(GRID_CAP + 9) // 10, seed=seed, far=far, ntargets=(40, 200))
    progs = []
    for p in range(GRID_CAP):
        if p % 10 == 0:
            progs.append(dense[p // 10])
            continue
        entry = int(rng.integers(0, 1 << 20))
        progs.append([(False, region_walk(rng, int(rng.integers(24, 49)), entry, 8)) for _ in range(2)])
    origin = list(range(GRID_CAP)) + list(range(GRID_CAP)) + list(range(52))
    return [progs[o] for o in origin], np.array(origin)


def pack(programs, gaps=None):
    """make_golden.pack with the sparse layout: gaps[(p, c)] follows call c of program p."""
    pcs, cs, cl, cf, pc = [], [], [], [], [0]
    pos = 0
    for p, prog in enumerate(programs):
        for c, (failed, t) in enumerate(prog):
            t = np.asarray(t, np.uint64)
            g = np.asarray((gaps or {}).get((p, c), ()), np.uint64)
            pcs += [t, g]
            cs.append(pos)
            cl.append(t.size)
            cf.append(int(failed))
            pos += t.size + g.size
        pc.append(pc[-1] + len(prog))
    return dict(pcs=np.concatenate(pcs) if pcs else np.empty(0, np.uint64), call_start=np.array(cs, np.uint64),
                call_len=np.array(cl, np.uint32), call_failed=np.array(cf, np.uint8), prog_call=np.array(pc, np.uint32))


def flat(programs, gaps=None):
    """-> (pcs, call_start, call_len, prog_call) of pack()."""
    fx = pack(programs, gaps)
    return fx["pcs"], fx["call_start"], fx["call_len"], fx["prog_call"]


def dup_heavy_batch():
    """The region walk, 16 programs x 8 calls x 2048 PCs: mostly duplicates."""
    from syzkaller_amd import synth

    cl = synth.call_lengths(16, 8, 2048)
    pcs, cs, _ = synth.traces(synth.synth_default(), 0, 16, 8, cl)
    return pcs, cs, cl, synth.prog_call_index(16, 8)
