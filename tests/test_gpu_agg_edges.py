"""GPU: k_agg (csrc/agg.hip agg_partition + k_agg) and Minimize's entry-mode
scatters on inputs built for their machinery, against the sequential oracle.

Triage front end (gpu.triage at set_agg(2, parts) vs O.triage_batch, through
test_gpu_triage.compare: bits, call_new, the exact pair set, maxSignal and
newSignal):
  A  probe chains of one LDS home bucket, the wrap 1855 -> 0 included
  B  many lanes and waves inserting one chain at once; the level staircase
  C  the per-wave first-sight queue at its flush boundaries
  D  the overflow bound kAggLimit, exactly
  E  the virtual-run cell walk: group sizes 8..64, empty cells, cell
     boundaries at batch edges, a single non-empty cell
Minimize front end (gpu.minimize vs O.minimize, survivors and count):
  F  entry tiles of 640 records and the split between the two scatters
  G  ties and winners
  H  per-entry prio handling (the optimistic run, the prio mask's tail)
  I  k_agg's queue path with per-record levels

Every case that asserts retries == 0 first asserts on the CPU
(agg_keys.fits_capped) that no capped cell spills: a spill is a legitimate
redo with counted cells and would hide the path under test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import agg_keys as AK
from tests.table_keys import fmix32_inv_np
from tests.test_gpu_triage import compare

pytestmark = pytest.mark.gpu

PB = 3  # 8 partitions: a work item is parts / 4 = 2 calls
LIMIT = AK.AGG_LIMIT


def _dev(gpu, hb):
    hs, hcs, hcnt, hprio = hb
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)  # noqa: E731
    return t(hs, np.int32), t(hcs, np.int64), t(hcnt, np.int32), t(hprio, np.uint8)


def _m0(rng, elems, n=4000):
    """A few thousand maxSignal elements, half of them the batch's own at
    random prios 0..3: lower, equal and higher than the calls' all occur."""
    own = rng.choice(np.unique(elems), size=min(n // 2, np.unique(elems).size), replace=False)
    e = np.unique(np.concatenate([own, rng.integers(0, 1 << 32, n // 2, np.uint64).astype(np.uint32)]))
    return e, rng.integers(0, 4, e.size).astype(np.int8)


def _cut(rng, stream, ncalls, prios=None):
    """stream as ncalls calls with random cuts and random prios 0..3."""
    cuts = np.sort(rng.choice(np.arange(1, stream.size), size=ncalls - 1, replace=False))
    hcs = np.concatenate([[0], cuts]).astype(np.uint64)
    hcnt = np.diff(np.concatenate([hcs, [stream.size]])).astype(np.uint32)
    hprio = rng.integers(0, 4, size=ncalls).astype(np.uint8) if prios is None else prios
    return stream.astype(np.uint32), hcs, hcnt, hprio


def _from_calls(calls, hprio):
    hcnt = np.array([c.size for c in calls], np.uint32)
    hcs = (np.cumsum(hcnt, dtype=np.uint64) - hcnt).astype(np.uint64)
    hs = np.concatenate(calls).astype(np.uint32) if hcnt.sum() else np.empty(0, np.uint32)
    return hs, hcs, hcnt, np.asarray(hprio, np.uint8)


def _triage(gpu, rng, hb, parts=8, dbg=0, fits=True, **kw):
    """compare() at a fixed partition count; asserts first that no capped cell
    spills (fits), so that retries == 0 can be asserted by the caller."""
    pbits = parts.bit_length() - 1
    if fits:
        assert AK.fits_capped(AK.cell_counts(hb[0], hb[1], hb[2], pbits, pbits - 2))
    gpu.eng.set_debug(dbg)
    try:
        st = compare(gpu, _m0(rng, hb[0]), hb, _dev(gpu, hb), agg=2, parts=parts, **kw)
    finally:
        gpu.eng.set_debug(0)
    assert st["parts"] == parts, st
    return st


# ---------------------------------------------------------------- A: probe chains
def _chain_pools(rng, clusters, per=1500):
    """8 partitions of `per` distinct elements; partition 3 holds the clusters
    (lists of (bucket, n, skip)) and uniformly hashed filler."""
    keys = [AK.agg_at(PB, 3, b, n, skip) for b, n, skip in clusters]
    cl = np.concatenate(keys)
    assert np.unique(cl).size == cl.size
    pools = [AK.agg_random(PB, p, per, rng) for p in range(8)]
    pools[3] = np.concatenate([cl, AK.agg_random(PB, 3, max(per - cl.size, 0), rng, exclude=cl)])
    return cl, pools


def _shuffled_batch(rng, elems, ncalls=600):
    """Every element once in a shuffled first pass, then 2x random repeats."""
    stream = np.concatenate([rng.permutation(elems), rng.choice(elems, size=2 * elems.size)])
    return _cut(rng, stream, ncalls)


CHAINS = [(b, n, ()) for b in (0, 927, 1855) for n in (1, 4, 5, 8, 9, 64, 65, 600)] + \
         [(1855, 9, ((0, 9, 0),)), (1855, 9, ((1854, 9, 0),)), (1855, 600, ((0, 9, 0),)), (1855, 600, ((1854, 9, 0),))]


@pytest.mark.parametrize("b,n,more", CHAINS, ids=lambda v: str(v).replace(" ", ""))
def test_agg_probe_chain_in_one_bucket(gpu, b, n, more):
    """n keys of partition 3 share LDS home bucket b: with n > 4 the keys past
    the home bucket take the wave queue on every record, and with b = 1855 the
    chain wraps into bucket 0 -- onto a second cluster homed there, or merged
    with a chain from bucket 1854 (more)."""
    rng = np.random.default_rng(1000 * b + n + len(more))
    cl, pools = _chain_pools(rng, [(b, n, 0)] + list(more))
    assert (AK.elem_home(cl[:n], PB)[1] == b).all() and (AK.elem_home(cl, PB)[0] == 3).all()
    elems = np.concatenate(pools)
    st = _triage(gpu, rng, _shuffled_batch(rng, elems))
    assert st["overflow_parts"] == 0 and st["retries"] == 0 and st["distinct"] == elems.size, st


@pytest.mark.parametrize("mode", ["idx64", "counted"])
def test_agg_probe_chain_wrap_other_kernels(gpu, mode):
    """The 600-key chain of bucket 1855 through the 64-bit index kernel and
    through counted cells (kCap = false)."""
    from syzkaller_amd._lib import SYZSIG_DEBUG_AGG_IDX64, SYZSIG_DEBUG_EXACT_CELLS

    rng = np.random.default_rng(77)
    cl, pools = _chain_pools(rng, [(1855, 600, 0)])
    elems = np.concatenate(pools)
    st = _triage(gpu, rng, _shuffled_batch(rng, elems),
                 dbg=SYZSIG_DEBUG_AGG_IDX64 if mode == "idx64" else SYZSIG_DEBUG_EXACT_CELLS)
    assert st["overflow_parts"] == 0 and st["retries"] == 0 and st["distinct"] == elems.size, st


# ---------------------------------------------------------------- B: insert races
@pytest.mark.parametrize("stair", [False, True])
def test_agg_insert_race_on_one_chain(gpu, stair):
    """The 600 keys of bucket 1855 adjacent in one call, and that call at the
    head of each of the first 20 groups of 8 work items: the 16 waves of the
    partition's workgroup start on those groups together, so 64 lanes of a wave
    and several waves insert into the same chain at once (atomicCAS losers
    re-read the bucket).  Each such call also holds 600 records of every other
    partition, so no capped cell spills.  stair: the 20 calls' prios rise 0..3
    in serial order, so every key has a different level first per level."""
    rng = np.random.default_rng(5 + stair)
    cl, pools = _chain_pools(rng, [(1855, 600, 0)])
    elems = np.concatenate(pools)
    rest = _shuffled_batch(rng, elems[~np.isin(elems, cl)], 580)
    calls = [rest[0][int(s): int(s) + int(c)] for s, c in zip(rest[1], rest[2])]
    prios = list(rest[3])
    assert AK.agg_group_size(300) == 8
    for g in range(20):  # call 16 g = the first call of work item 8 g = the head of group g
        big = np.concatenate([rng.permutation(cl)] + [rng.choice(pools[p], 600) for p in range(8) if p != 3])
        calls.insert(16 * g, big)
        prios.insert(16 * g, min(g // 5, 3) if stair else int(rng.integers(0, 4)))
    assert len(calls) == 600 and all(np.array_equal(np.sort(calls[16 * g][:600]), np.sort(cl)) for g in range(20))
    st = _triage(gpu, rng, _from_calls(calls, prios))
    assert st["overflow_parts"] == 0 and st["retries"] == 0 and st["distinct"] == elems.size, st


# ---------------------------------------------------------------- C: queue fill
def _queue_stream(kind, rng, pool, nblk):
    """Partition 3's records, 256 (one batch of a wave) per block."""
    out, used = [], 0
    for _ in range(nblk):
        if kind == "all_distinct":
            blk = pool[used: used + 256]
            used += 256
        elif kind in ("first64", "first65"):
            k = 64 if kind == "first64" else 65
            new = pool[used: used + k]
            used += k
            blk = np.concatenate([new, rng.choice(new, 256 - k)])
        else:  # hot: one element all along, one new element per block
            blk = np.full(256, pool[0], np.uint32)
            blk[int(rng.integers(0, 256))] = pool[1 + used]
            used += 1
        out.append(blk)
    return np.concatenate(out)


@pytest.mark.parametrize("kind", ["all_distinct", "first64", "first65", "hot"])
def test_agg_queue_fill_boundaries(gpu, kind):
    """First sightings per 256-record batch of partition 3: all 256 (a flush
    before most records), exactly 64 (the queue full, no flush until the next
    batch), 65 (one over), and one per batch among a hot element's repeats.
    The order of a cell's records is the scatter's, so these are shapes of at
    least this pressure; asserted are exactness and no overflow.  The eight
    partitions' streams are interleaved record by record: equal cells."""
    rng = np.random.default_rng(len(kind))
    nblk = 22  # 22 x 256 = 5632 <= kAggLimit distinct in the all-distinct stream
    pool = AK.agg_random(PB, 3, nblk * 256, rng)
    s3 = _queue_stream(kind, rng, pool, nblk)
    streams = [s3 if p == 3 else rng.choice(AK.agg_random(PB, p, 1500, rng), s3.size) for p in range(8)]
    hs = np.stack(streams, axis=1).reshape(-1)  # record i of every partition in turn
    ncalls = hs.size // 512
    hb = (hs, np.arange(ncalls, dtype=np.uint64) * 512, np.full(ncalls, 512, np.uint32),
          rng.integers(0, 4, ncalls).astype(np.uint8))
    assert (AK.cell_counts(*hb[:3], PB, 1) == 128).all()
    st = _triage(gpu, rng, hb)
    assert st["overflow_parts"] == 0 and st["retries"] == 0 and st["distinct"] == np.unique(hs).size, st


# ---------------------------------------------------------------- D: the overflow bound
def _bound_batch(rng, p, n):
    """Partition p holds n distinct elements, the others kAggLimit - 300; h = 0
    is in partition 0 and h = 0xFFFFFFFF in partition 7.  Every partition gets
    the same number of records."""
    per = 3 * (LIMIT + 1)
    parts = []
    for q in range(8):
        k = n if q == p else LIMIT - 300
        low = rng.choice(1 << 29, size=k, replace=False).astype(np.uint32)
        if q == 0:
            low[0] = 0
        if q == 7:
            low[0] = (1 << 29) - 1
        low = np.unique(low)
        while low.size < k:  # (the forced value was drawn as well)
            low = np.unique(np.concatenate([low, rng.integers(1, (1 << 29) - 1, k - low.size).astype(np.uint32)]))
        e = fmix32_inv_np((np.uint32(q) << np.uint32(29)) | low)
        parts.append(np.concatenate([e, rng.choice(e, size=per - k)]))
    elems = np.concatenate(parts)
    d = np.unique(elems)
    assert d.size == n + 7 * (LIMIT - 300) and 0 in AK.fmix32_np(d) and 0xFFFFFFFF in AK.fmix32_np(d)
    assert (np.bincount(AK.elem_home(d, PB)[0], minlength=8)[p]) == n
    return _cut(rng, rng.permutation(elems), 600), d.size


@pytest.mark.parametrize("p", [0, 7])
@pytest.mark.parametrize("over", [0, 1])
def test_agg_overflow_bound_is_exact(gpu, p, over):
    """k_agg counts successful inserts, so a partition of exactly kAggLimit
    distinct elements stays in LDS and one of kAggLimit + 1 is voided and
    committed from the HBM fallback -- whatever the order of its records."""
    rng = np.random.default_rng(10 * p + over)
    hb, distinct = _bound_batch(rng, p, LIMIT + over)
    st = _triage(gpu, rng, hb)
    assert st["overflow_parts"] == over and st["distinct"] == distinct, st
    if not over:
        assert st["retries"] == 0, st


@pytest.mark.parametrize("p", [0, 7])
def test_agg_overflow_bound_one_sync_direct_pairs(gpu, p):
    """kAggLimit + 1 in the one-sync run (no per-record bits) writing its
    pairs straight to the caller's buffer of 4 x 8 x kAggLimit entries."""
    rng = np.random.default_rng(30 + p)
    hb, distinct = _bound_batch(rng, p, LIMIT + 1)
    st = _triage(gpu, rng, hb, want_bits=False, pairs_cap=4 * 8 * LIMIT)
    assert st["overflow_parts"] == 1 and st["retries"] == 0, st


# ---------------------------------------------------------------- E: cell walk
# Work items (2 calls each at 8 partitions).  500, 513, 1030 and 2060 are the
# counts the group sizes were first thought to change at; agg_group_size
# divides with truncation, so they give 8, 8, 16 and 32 cells per group, and
# 521, 1041 and 2081 give 16, 32 and 64.  The last group is partial in all.
WALK_ITEMS = {500: 8, 513: 8, 1030: 16, 2060: 32, 521: 16, 1041: 32, 2081: 64}
WALK_PATTERNS = ["all8", "alt0_16", "empty_first", "empty_mid", "empty_last", "big-1", "big0", "big1",
                 "one1", "one255", "one256", "one257", "one512", "one513", "shared"]


def _walk_counts(pattern, nitems, gsz):
    n = np.full(nitems, 8, np.int64)
    ngroups = (nitems + gsz - 1) // gsz
    if pattern == "alt0_16":
        n[0::2], n[1::2] = 0, 16
    elif pattern.startswith("empty_"):
        g = {"first": 0, "mid": ngroups // 2, "last": ngroups - 1}[pattern[6:]]
        n[g * gsz: (g + 1) * gsz] = 0
    elif pattern.startswith("big"):
        # the first cell of a group: the next cell starts at virtual record
        # 2048 + r, a batch edge (8 x 256) and the prefetch distance's multiple
        n[(ngroups // 2) * gsz] = 2048 + int(pattern[3:])
    elif pattern.startswith("one"):
        n[:] = 0
        n[nitems // 2] = int(pattern[3:])
    return n


def _walk_batch(rng, n, gsz, shared, call_prio=None):
    """Items of n[i] records in 2 calls ([0, n], [n, 0] or halves by i % 3), all
    elements distinct, every item's records spread evenly over the 8
    partitions.  shared: one element of the last item of every group replaces a
    record (same partition) of the next group's first item."""
    total = int(n.sum())
    pools = [AK.agg_random(PB, p, total // 8 + n.size + 8, rng) for p in range(8)]
    ptr = [0] * 8
    items = []
    for i, k in enumerate(n.tolist()):
        cnt = k // 8 + (((np.arange(8) - i) % 8) < k % 8)
        rec = [pools[p][ptr[p]: ptr[p] + cnt[p]] for p in range(8)]
        for p in range(8):
            ptr[p] += int(cnt[p])
        items.append(rng.permutation(np.concatenate(rec)))
    assert np.unique(np.concatenate(items)).size == total
    if shared:
        for i in range(gsz - 1, n.size - 1, gsz):
            x = items[i][0]
            same = np.nonzero(AK.elem_home(items[i + 1], PB)[0] == AK.elem_home(x, PB)[0][0])[0]
            items[i + 1][same[0]] = x
    calls = []
    for i, it in enumerate(items):
        a = (0, it.size, it.size // 2)[i % 3]
        calls += [it[:a], it[a:]]
    prio = np.full(len(calls), 2, np.uint8) if shared else rng.integers(0, 4, len(calls)).astype(np.uint8)
    return _from_calls(calls, prio)


@pytest.mark.parametrize("pattern", WALK_PATTERNS)
@pytest.mark.parametrize("nitems", list(WALK_ITEMS))
def test_agg_cell_walk_geometry(gpu, nitems, pattern):
    """The virtual run over a group's cells: about one record per cell (up to
    63 cells starting inside one 256-record batch at 64 cells per group), empty
    cells sharing their successor's start, a whole group of empty cells, a cell
    boundary at 2048 - 1, 2048 and 2048 + 1 records, a single non-empty cell of
    1..513 records, and an element shared across a group boundary (equal prios:
    only the earlier call is new).  Elements are otherwise all distinct, so a
    record attributed to a neighbouring cell changes the pairs and the bits."""
    gsz = AK.agg_group_size(nitems)
    assert gsz == WALK_ITEMS[nitems] and nitems % gsz != 0  # the last group is partial
    rng = np.random.default_rng(nitems * 31 + WALK_PATTERNS.index(pattern))
    n = _walk_counts(pattern, nitems, gsz)
    hb = _walk_batch(rng, n, gsz, pattern == "shared")
    assert hb[2].size == 2 * nitems
    np.testing.assert_array_equal(AK.cell_counts(*hb[:3], PB, 1).sum(axis=1), n)
    st = _triage(gpu, rng, hb)
    assert st["overflow_parts"] == 0 and st["retries"] == 0, st
    assert st["distinct"] == np.unique(hb[0]).size, st


def test_agg_cell_walk_2048_partitions(gpu):
    """64 cells per group at 2048 partitions: 2100 work items of 512 calls of
    0 or 1 records (about 1 M calls, half of them empty), all elements
    distinct."""
    rng = np.random.default_rng(2048)
    nitems, parts = 2100, 2048
    assert AK.agg_group_size(nitems) == 64 and nitems % 64 != 0
    hcnt = rng.integers(0, 2, nitems * 512).astype(np.uint32)
    hcnt[:512] = 0  # the first work item is empty
    total = int(hcnt.sum())
    e = np.unique(rng.integers(0, 1 << 32, 2 * total, np.uint64).astype(np.uint32))
    hs = rng.permutation(e)[:total]
    hb = (hs, (np.cumsum(hcnt, dtype=np.uint64) - hcnt).astype(np.uint64), hcnt,
          rng.integers(0, 4, hcnt.size).astype(np.uint8))
    st = _triage(gpu, rng, hb, parts=parts)
    assert st["overflow_parts"] == 0 and st["retries"] == 0 and st["distinct"] == total, st


# ---------------------------------------------------------------- Minimize (entry mode)
MIN_ITEMS = 2048                          # agg.hip kMinItems
ENTRY_TILE, SCAT3_FILL = 640, 85          # agg.hip kScat3TileEntry (kScat3KEntry * 64), kScat3Fill


def min_ibits(nctx, parts):
    """agg_aggregate's work-item size for Minimize: 2^ibits contexts, from a
    chunk (cbits = pbits - 2) down while there are fewer than kMinItems items."""
    ibits = parts.bit_length() - 1 - 2
    while ibits > 0 and (nctx >> ibits) < MIN_ITEMS:
        ibits -= 1
    return ibits


def entry_scat3_takes(lens):
    """scat3_takes for one work item of Minimize: k_scat3<10, true, *> takes it
    when its one-context tiles of 640 entries would be at least 85 % full."""
    lens = np.asarray(lens, np.uint64)
    tiles = int(((lens + ENTRY_TILE - 1) // ENTRY_TILE).sum())
    return int(lens.sum()) * 100 >= tiles * ENTRY_TILE * SCAT3_FILL


def _corpus(rng, lens, universe, prio_vals=(0, 1, 2, 3)):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    e = [rng.choice(universe, size=int(L), replace=False) for L in lens]
    e = np.concatenate(e).astype(np.uint32) if off[-1] else np.empty(0, np.uint32)
    return off, e, rng.choice(np.array(prio_vals, np.int8), size=e.size)


def _minimize(gpu, off, e, p, parts=0, dprios=None):
    """gpu.minimize at a fixed partition count (0: the library's own) against
    the oracle: the survivor list and the count."""
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)  # noqa: E731
    gpu.eng.set_agg(1, parts)
    try:
        keep, cnt = gpu.minimize(t(off, np.int64), t(e, np.int32), t(p, np.int8) if dprios is None else dprios)
    finally:
        gpu.eng.set_agg(1, 0)
    exp = O.minimize(off, e, p)
    assert np.nonzero(keep.cpu().numpy())[0].tolist() == exp
    assert cnt == len(exp)
    return exp


def _rank_order(off):
    lens = np.diff(off.astype(np.int64))
    return np.lexsort((np.arange(lens.size), -lens))  # Len desc, index asc


EDGE_LENS = [0, 1, 63, 64, 65, 543, 544, 545, 639, 640, 641, 1279, 1280, 1281, 1500, 6400]


@pytest.mark.parametrize("parts", [8, 1024, 2048])
def test_minimize_entry_tile_edges_and_split(gpu, parts):
    """Context lengths at the entry tile's edges (640, 1280) and either side of
    the split (0.85 x 640 = 544), four of each (ties: Len desc, index asc),
    among ~2400 contexts of 1..8 entries, through the 128-byte-block scatters
    (8 and 1024 partitions) and the 64-byte-block ones (2048).  With ~2500
    contexts every work item is one context (ibits = 0).  gpu.minimize reports
    no per-kernel counts: which scatter takes an item is asserted on the
    restated rule only, and a run in which one kernel took every item would
    still have to be exact."""
    rng = np.random.default_rng(parts)
    lens = np.array(EDGE_LENS * 4 + list(rng.integers(1, 9, 2500 - 4 * len(EDGE_LENS))), np.int64)
    lens = rng.permutation(lens)
    lens[-1] = max(lens[-1], 1)
    assert min_ibits(lens.size, parts) == 0
    takes = {L: entry_scat3_takes([L]) for L in EDGE_LENS}
    assert [L for L in EDGE_LENS if not takes[L]] == [1, 63, 64, 65, 543, 641, 1281, 1500]
    universe = np.unique(rng.integers(0, 1 << 32, {8: 20_000, 1024: 200_000, 2048: 400_000}[parts], np.uint64)
                         .astype(np.uint32))
    off, e, p = _corpus(rng, lens, universe)
    pbits = parts.bit_length() - 1
    order = _rank_order(off)
    counts = AK.cell_counts(e, off[:-1][order], lens[order], pbits, 0)
    assert AK.fits_capped(counts) and counts.sum() == e.size
    assert np.count_nonzero(counts) > 2 * lens.size  # (cells in use: more than two per context)
    assert np.bincount(AK.elem_home(np.unique(e), pbits)[0]).max() <= LIMIT
    _minimize(gpu, off, e, p, parts)


@pytest.mark.parametrize("parts", [0, 8])
@pytest.mark.parametrize("case", ["identical", "one_higher", "longer_wins", "top_in_last_rank", "all_empty",
                                  "one_context", "one_entry"])
def test_minimize_ties_and_winners(gpu, case, parts):
    rng = np.random.default_rng(len(case))
    universe = np.unique(rng.integers(0, 1 << 32, 20_000, np.uint64).astype(np.uint32))
    if case in ("identical", "one_higher"):
        # 64 contexts, one element set of 700, equal prios: the first wins every element
        s = rng.choice(universe, 700, replace=False)
        e = np.concatenate([rng.permutation(s) for _ in range(64)])
        off = np.arange(65, dtype=np.uint64) * 700
        p = np.full(e.size, 2, np.int8)
        if case == "one_higher":
            p[37 * 700 + 5] = 3
        assert _minimize(gpu, off, e, p, parts) == ([0] if case == "identical" else [0, 37])
        return
    if case == "longer_wins":
        # nested contexts of 10..640 entries in a shuffled order, equal prios:
        # the longest covers them all
        s = rng.choice(universe, 640, replace=False)
        lens = rng.permutation(np.arange(10, 650, 10))
        off, e, p = _corpus(rng, lens, universe)
        e = np.concatenate([s[:L] for L in lens]).astype(np.uint32)
        p[:] = 1
        assert _minimize(gpu, off, e, p, parts) == [int(np.argmax(lens))]
        return
    if case == "top_in_last_rank":
        # x at prio 3 only in the last context by rank (the shortest, highest index)
        lens = np.concatenate([rng.integers(2, 300, 999), [1]])
        off, e, p = _corpus(rng, lens, universe[1:], (0, 1, 2))
        x = universe[0]
        for c in range(0, 999, 7):
            e[off[c]] = x
        e[-1], p[-1] = x, 3
        assert _rank_order(off)[-1] == 999 and 999 in _minimize(gpu, off, e, p, parts)
        return
    lens = {"all_empty": [0] * 300, "one_context": [700], "one_entry": [1]}[case]
    exp = _minimize(gpu, *_corpus(rng, lens, universe), parts)
    assert exp == ([] if case == "all_empty" else [0])


@pytest.mark.parametrize("parts", [0, 8])
@pytest.mark.parametrize("case", ["redo_tail5", "fifth_prio_last"] + [f"mask_r{r}_o{o}" for r in (1, 7, 15)
                                                                      for o in (0, 1)])
def test_minimize_per_entry_prios(gpu, case, parts):
    """redo_tail5: prios 0 and 3 all along and -2, -1 only among the last 5
    entries: the optimistic 0..3 run voids itself and the exact run (4 levels)
    gives the oracle's result.  fifth_prio_last: 0..3 and a fifth prio in the
    last entry: the atomic path takes over.  mask_r*_o*: an entry count
    = r mod 16 with prio -1 only in the last entry (k_min_prio_mask's tail
    loop), the prios also passed as a view at byte offset 1 of a larger tensor
    (its unaligned path: the wrapper passes the pointer on as it is)."""
    rng = np.random.default_rng(len(case) + parts)
    universe = np.unique(rng.integers(0, 1 << 32, 20_000, np.uint64).astype(np.uint32))
    lens = list(rng.geometric(1.0 / 60, size=1500))
    dprios = None
    if case == "redo_tail5":
        off, e, p = _corpus(rng, lens + [9], universe, (0, 3))
        p[-5:] = [-2, -1, 0, 3, -2]
    elif case == "fifth_prio_last":
        off, e, p = _corpus(rng, lens + [9], universe)
        p[-1] = 7
    else:
        r, o = int(case.split("_")[1][1:]), int(case[-1])
        lens.append(16 + (r - sum(lens)) % 16)
        off, e, p = _corpus(rng, lens, universe, (-2, 0, 3))
        p[-1] = -1
        assert e.size % 16 == r and (p[:-1] != -1).all()
        if o:
            big = torch.zeros(e.size + 64, dtype=torch.int8, device=gpu.dev)
            dprios = big[1: 1 + e.size]
            dprios.copy_(torch.from_numpy(p))
            assert dprios.data_ptr() % 16 == 1 and dprios.is_contiguous()
    _minimize(gpu, off, e, p, parts, dprios)


def test_minimize_probe_chain_with_entry_levels(gpu):
    """Case A's 600-key chain of bucket 1855 (partition 3 of 8) as a corpus:
    600 contexts of about 700 entries drawn from the chain and the filler, with
    per-entry prios 0..3 -- level bits from per-record prios through k_agg's
    queue path."""
    rng = np.random.default_rng(1855)
    cl, pools = _chain_pools(rng, [(1855, 600, 0)])
    universe = np.concatenate(pools)
    lens = rng.integers(650, 750, 600)
    off, e, p = _corpus(rng, lens, universe)
    assert np.isin(cl, e).all()
    order = _rank_order(off)
    assert min_ibits(600, 8) == 0
    assert AK.fits_capped(AK.cell_counts(e, off[:-1][order], lens[order], PB, 0))
    _minimize(gpu, off, e, p, 8)
