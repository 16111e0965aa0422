"""Keys with a chosen home bucket in a device Signal table (no GPU use).

A table of nb buckets (csrc/internal.h home_bucket) places element e in bucket
(fmix32(e) * nb) >> 32: the top bits of h = fmix32(e).  fmix32 is a bijection
of u32, so picking h picks the bucket: keys that all share one home bucket form
one probe chain, as long as the test wants, which uniformly random keys never
do."""
import numpy as np

BUCKET_SLOTS = 2  # csrc/common.h kBucketSlots


def fmix32_np(x):
    """murmur3 fmix32 (csrc/common.h fmix32), on a u32 array."""
    h = np.array(x, np.uint32, copy=True, ndmin=1)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def fmix32_inv_np(h):
    """Inverse of murmur3 fmix32 (csrc/common.h fmix32_inv), on a u32 array."""
    h = np.asarray(h, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7ED1B41D)
    h ^= (h >> np.uint32(13)) ^ (h >> np.uint32(26))
    h *= np.uint32(0xA5CB9243)
    h ^= h >> np.uint32(16)
    return h


def home_bucket(e, nb):
    """Home bucket of every element of e in a table of nb buckets."""
    return (fmix32_np(e).astype(np.uint64) * np.uint64(nb)) >> np.uint64(32)


def hot_last(n, skip=0):
    """n distinct keys with h = 0xFFFFFFFF - i, skip <= i < skip + n: they home
    to the LAST bucket of every table of up to 2^32 / (skip + n) buckets."""
    i = np.arange(skip, skip + n, dtype=np.uint64)
    return fmix32_inv_np((np.uint64(0xFFFFFFFF) - i).astype(np.uint32))


def hot_first(n, skip=0):
    """n distinct keys with h = i, skip <= i < skip + n: they home to bucket 0
    of every table of up to 2^32 / (skip + n) buckets."""
    return fmix32_inv_np(np.arange(skip, skip + n, dtype=np.uint64).astype(np.uint32))


def hot_at(nb, b, n):
    """n distinct keys homing to bucket b of a table of nb buckets (the n
    smallest h of that bucket; n <= 2^32 / nb, the values of h a bucket owns)."""
    assert 0 <= b < nb and n <= (1 << 32) // nb
    h0 = -((-(b << 32)) // nb)  # the least h with (h * nb) >> 32 == b
    return fmix32_inv_np(np.arange(h0, h0 + n, dtype=np.uint64).astype(np.uint32))
