"""Elements with a chosen aggregation partition and LDS home bucket, and the
capped-cell capacity rule (no GPU use).

k_agg (csrc/agg.hip) cuts a run into P = 2^pbits partitions by the top pbits
of h = fmix32(e) and keeps a partition's distinct elements in an LDS table of
kAggBuckets buckets of kAggBW keys, keyed by the residual (the low 32 - pbits
bits of h) and homed by the residual's top bits.  fmix32 is a bijection of
u32, so picking h picks both the partition and the home bucket: keys that
share one bucket form a probe chain as long as the test wants, which
uniformly hashed elements at the design load of 0.4 never do.

Restated from csrc/agg.hip (the line each comes from):
  kAggSlots, kAggBW, kAggBuckets, kAggLimit   :61-67
  AggGeom.part / rec / resid                  :89, :94, :95
  agg_home_bucket                             :101-104
  agg_group_size                              :2188-2194
  cell_plan's capacity                        :994-995 (float arithmetic)
and csrc/internal.h:198 kCapSdDefault, the slack a context starts with and
syzsig_ctx_set_agg resets to (runtime.hip:218)."""
import numpy as np

from tests.table_keys import fmix32_inv_np, fmix32_np

AGG_SLOTS = 7424                     # kAggSlots
AGG_BW = 4                           # kAggBW
AGG_BUCKETS = AGG_SLOTS // AGG_BW    # kAggBuckets = 1856
AGG_LIMIT = AGG_SLOTS * 4 // 5       # kAggLimit = 5939
AGG_GROUP = 8                        # kAggGroup
AGG_BATCH = 4 * 64                   # kAggU * 64: records of one batch of a wave
CAP_SD = 6.0                         # kCapSdDefault
assert AGG_BUCKETS == 1856 and AGG_LIMIT == 5939


def part(h, pbits):
    """AggGeom.part: the partition of h = fmix32(e)."""
    return np.asarray(h, np.uint32) >> np.uint32(32 - pbits)


def resid(h, pbits):
    """The LDS key of h: AggGeom.resid of the packed record (h << pbits) | meta,
    i.e. the low 32 - pbits bits of h."""
    return np.asarray(h, np.uint32) & np.uint32((1 << (32 - pbits)) - 1)


def home_bucket(key, pbits):
    """agg_home_bucket: (((key << pbits) mod 2^32) * kAggBuckets) >> 32."""
    x = (np.asarray(key, np.uint64) << np.uint64(pbits)) & np.uint64(0xFFFFFFFF)
    return ((x * np.uint64(AGG_BUCKETS)) >> np.uint64(32)).astype(np.uint32)


def elem_home(e, pbits):
    """(partition, LDS home bucket) of every element of e."""
    h = fmix32_np(e)
    return part(h, pbits), home_bucket(resid(h, pbits), pbits)


def bucket_resid_range(pbits, b):
    """[lo, hi): the residuals whose home bucket is b."""
    d = AGG_BUCKETS << pbits
    return -((-(b << 32)) // d), -((-((b + 1) << 32)) // d)


def agg_at(pbits, p, b, n, skip=0):
    """n distinct elements of partition p whose LDS home bucket is b: the n
    smallest residuals of that bucket after the first `skip`."""
    assert 0 <= p < (1 << pbits) and 0 <= b < AGG_BUCKETS
    lo, hi = bucket_resid_range(pbits, b)
    assert skip + n <= hi - lo, (n, skip, hi - lo)  # the bucket's share of the residuals
    r = np.arange(lo + skip, lo + skip + n, dtype=np.uint64)
    return fmix32_inv_np(((np.uint64(p) << np.uint64(32 - pbits)) | r).astype(np.uint32))


def agg_random(pbits, p, n, rng, exclude=()):
    """n distinct uniformly hashed filler elements of partition p, none of them in `exclude`."""
    rbits = 32 - pbits
    ex = np.asarray(exclude, np.uint32)
    got = np.empty(0, np.uint32)
    while got.size < n:
        low = rng.integers(0, 1 << rbits, size=2 * n + 16, dtype=np.uint64)
        e = fmix32_inv_np(((np.uint64(p) << np.uint64(rbits)) | low).astype(np.uint32))
        e = e[~np.isin(e, ex)]
        _, first = np.unique(np.concatenate([got, e]), return_index=True)
        got = np.concatenate([got, e])[np.sort(first)]
    return got[:n]


def agg_group_size(ncells):
    """agg_group_size: k_agg's cells per wave work item."""
    gz = AGG_GROUP
    while gz < 64 and ncells // gz > 64:
        gz <<= 1
    return gz


def cell_counts(hs, hcs, hcnt, pbits, ibits):
    """counts[item, partition]: the records of every capped cell of a batch
    whose work items are 2^ibits consecutive calls."""
    hs, hcs, hcnt = np.asarray(hs, np.uint32), np.asarray(hcs, np.int64), np.asarray(hcnt, np.int64)
    P, nitems = 1 << pbits, (hcnt.size + (1 << ibits) - 1) >> ibits
    total = int(hcnt.sum())
    call = np.repeat(np.arange(hcnt.size, dtype=np.int64), hcnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(hcnt) - hcnt, hcnt)
    p = part(fmix32_np(hs[np.repeat(hcs, hcnt) + within]), pbits).astype(np.int64) if total else call
    return np.bincount((call >> ibits) * P + p, minlength=nitems * P).reshape(nitems, P)


def cell_capacity(item_records, P, sd=CAP_SD):
    """cell_plan: cap = m + sd * sqrt(m) + 64 rounded up to 64, m = the item's
    records / P, in the kernel's float arithmetic."""
    m = np.asarray(item_records, np.float32) / np.float32(P)
    k = (m + np.float32(sd) * np.sqrt(m, dtype=np.float32)).astype(np.float32)
    return ((k.astype(np.uint32) + np.uint32(64 + 63)) & ~np.uint32(63)).astype(np.int64)


def fits_capped(counts, sd=CAP_SD):
    """True when no cell of `counts` (cell_counts) exceeds its capacity: the
    capped-cell run then is not redone with counted cells."""
    counts = np.asarray(counts)
    return bool((counts <= cell_capacity(counts.sum(axis=1), counts.shape[1], sd)[:, None]).all())


# ---- the finalize's per-element decision, exhaustively (test_finalize_staircase_every_order)
STAIR_ORDERS = 64   # ordered non-empty selections of the levels 0..3: 4 + 12 + 24 + 24
STAIR_M0 = (None, 0, 1, 2, 3)   # M0[e]: absent, or a prio


def staircase_cases():
    """One element per (order of first appearance of its levels, M0 state):
    64 x 5 = 320 elements.  Returns (elems, orders, batch, m0): elems[o * 5 + m]
    has order orders[o] (a tuple of prios) and M0 state STAIR_M0[m]; batch =
    (sigs, call_start, call_len, call_prio) of 17 calls in serial order --
    call 4 * pos + prio holds the elements whose pos-th first appearance is at
    prio, and call 16 (prio 0) repeats every element, a later dominated record
    for each; m0 = (elems, prios) of maxSignal, sorted by element.

    h = fmix32(e) is chosen so that the elements spread over 8 partitions (top
    3 bits) and crowd a few home buckets of each table's slice: 4 per bucket of
    a 2048-bucket table, 16 per bucket of a 512-bucket one (2 slots each), so
    probe sequences leave the home bucket and inserts of one bucket race."""
    from itertools import permutations

    orders = [p for k in range(1, 5) for p in permutations(range(4), k)]
    i = np.arange(len(orders) * len(STAIR_M0), dtype=np.uint64)
    elems = fmix32_inv_np((((i % 8) << 29) | ((i // 8) << 19)).astype(np.uint32))
    calls = [[] for _ in range(16)]
    m0e, m0p = [], []
    for o, order in enumerate(orders):
        for m, prio0 in enumerate(STAIR_M0):
            e = elems[o * len(STAIR_M0) + m]
            for pos, prio in enumerate(order):
                calls[4 * pos + prio].append(e)
            if prio0 is not None:
                m0e.append(e)
                m0p.append(prio0)
    calls = [np.array(c, np.uint32) for c in calls] + [elems.copy()]
    hcnt = np.array([c.size for c in calls], np.uint32)
    hcs = (np.cumsum(hcnt, dtype=np.uint64) - hcnt).astype(np.uint64)
    hprio = np.array([c % 4 for c in range(16)] + [0], np.uint8)
    m0e, m0p = np.array(m0e, np.uint32), np.array(m0p, np.int8)
    k = np.argsort(m0e)
    return elems, orders, (np.concatenate(calls), hcs, hcnt, hprio), (m0e[k], m0p[k])
