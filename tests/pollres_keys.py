"""Elements with a chosen home slot in k_pr_short's LDS table (csrc/pollres.hip;
no GPU use).

The table has 2 * SYZSIG_POLLRES_TILE = 8192 slots and places element e at
pr_lds_home(e) = (e * 0x9E3779B1 mod 2^32) >> 19, probing linearly from there.
Elements that share one home slot form one probe chain as long as the test
wants, which uniformly random elements never do.  They are found by brute
force over the hash, as tests/agg_keys.py does for k_agg."""
import numpy as np

TILE = 4096  # include/syzsig.h SYZSIG_POLLRES_TILE
SLOT_BITS = 13  # csrc/pollres.hip kPrSlotBits
SLOTS = 1 << SLOT_BITS
MULT = 0x9E3779B1


def lds_home(e):
    """pr_lds_home on a u32 array."""
    e = np.asarray(e, np.uint32).astype(np.uint64)
    return (((e * np.uint64(MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - SLOT_BITS)).astype(np.uint32)


def same_home(slot, n, start=1):
    """The n smallest elements >= start whose home slot is `slot`."""
    assert 0 <= slot < SLOTS
    out, have, lo = [], 0, start
    while have < n:
        cand = np.arange(lo, lo + (1 << 22), dtype=np.uint64)
        assert cand[-1] < (1 << 32)
        hit = cand[lds_home(cand.astype(np.uint32)) == slot]
        out.append(hit)
        have += hit.size
        lo += 1 << 22
    return np.concatenate(out)[:n].astype(np.uint32)
