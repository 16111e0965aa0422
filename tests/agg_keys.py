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
  agg_group_size                              :2212-2218
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
