"""CPU: tests/agg_keys.py -- the partition and LDS home bucket of the key sets
that tests/test_gpu_agg_edges.py builds k_agg's probe chains from, the group
size and the capped-cell counts."""
import numpy as np
import pytest

from tests import agg_keys as AK
from tests.table_keys import fmix32_np
from tests.test_table_keys_cpu import _fmix32_int


def _home_int(e, pbits):
    """(partition, home bucket) of one element on Python ints (csrc/agg.hip
    AggGeom.part, AggGeom.rec / resid, agg_home_bucket)."""
    h = _fmix32_int(int(e))
    rec = (h << pbits) & 0xFFFFFFFF          # AggGeom.rec with meta 0
    key = rec >> pbits                        # AggGeom.resid
    return h >> (32 - pbits), (((key << pbits) & 0xFFFFFFFF) * 1856) >> 32


def test_constants():
    assert (AK.AGG_SLOTS, AK.AGG_BW, AK.AGG_BUCKETS, AK.AGG_LIMIT) == (7424, 4, 1856, 5939)


@pytest.mark.parametrize("pbits", [3, 8, 11])
@pytest.mark.parametrize("b", [0, 1, 927, 1854, 1855])
def test_agg_at_homes_where_it_says(pbits, b):
    P = 1 << pbits
    for p in sorted({0, 3, P - 1}):
        e = AK.agg_at(pbits, p, b, 600)
        assert np.unique(e).size == 600
        assert all(_home_int(v, pbits) == (p, b) for v in e)
        pp, bb = AK.elem_home(e, pbits)
        assert (pp == p).all() and (bb == b).all()
        # the residual before the bucket's first belongs to the bucket below, the
        # one after its last to the bucket above
        lo, hi = AK.bucket_resid_range(pbits, b)
        assert hi - lo in ((1 << (32 - pbits)) // 1856, (1 << (32 - pbits)) // 1856 + 1)
        if b:
            assert int(AK.home_bucket(np.array([lo - 1]), pbits)[0]) == b - 1
        if b < 1855:
            assert int(AK.home_bucket(np.array([hi]), pbits)[0]) == b + 1
        else:
            assert hi == 1 << (32 - pbits)
        assert int(AK.home_bucket(np.array([hi - 1]), pbits)[0]) == b


def test_agg_at_skip_and_limit():
    a, b = AK.agg_at(3, 3, 1855, 20), AK.agg_at(3, 3, 1855, 20, skip=20)
    np.testing.assert_array_equal(np.concatenate([a, b]), AK.agg_at(3, 3, 1855, 40))
    lo, hi = AK.bucket_resid_range(11, 927)
    assert np.unique(AK.agg_at(11, 5, 927, hi - lo)).size == hi - lo
    with pytest.raises(AssertionError):
        AK.agg_at(11, 5, 927, hi - lo + 1)
    with pytest.raises(AssertionError):
        AK.agg_at(11, 5, 927, hi - lo, skip=1)


@pytest.mark.parametrize("pbits", [3, 8, 11])
def test_agg_random_is_distinct_in_partition_and_disjoint(pbits):
    rng = np.random.default_rng(pbits)
    keys = AK.agg_at(pbits, 3, 1855, 600)
    # (at pbits 11 a partition owns 2^21 residuals: 1500 draws collide with each other and with the keys' range)
    fill = AK.agg_random(pbits, 3, 1500, rng, exclude=keys)
    assert fill.size == 1500 and np.unique(fill).size == 1500
    assert np.intersect1d(fill, keys).size == 0
    assert (AK.elem_home(fill, pbits)[0] == 3).all()
    # uniformly hashed: the filler spreads over the buckets (1500 keys in 1856 buckets)
    assert np.unique(AK.elem_home(fill, pbits)[1]).size > 900
    # exclusion is honoured even when it covers most of what is drawn
    small = AK.agg_random(11, 0, 1000, rng, exclude=AK.agg_random(11, 0, 100_000, rng))
    assert np.unique(small).size == 1000


def test_agg_group_size_thresholds():
    """gz doubles while ncells / gz (integer division) exceeds 64: the steps
    are at 520, 1040 and 2080 cells, not at 513, 1025 and 2049."""
    got = {n: AK.agg_group_size(n) for n in (1, 500, 512, 513, 519, 520, 1024, 1025, 1039, 1040, 2048, 2049, 2079, 2080,
                                             2100, 1 << 20)}
    assert got == {1: 8, 500: 8, 512: 8, 513: 8, 519: 8, 520: 16, 1024: 16, 1025: 16, 1039: 16, 1040: 32, 2048: 32,
                   2049: 32, 2079: 32, 2080: 64, 2100: 64, 1 << 20: 64}


def test_cell_counts_hand_made_batch():
    """8 partitions, items of 2 calls: 3 calls = 2 items, the last short; call 1
    is empty and call 2's records lie before call 0's in the record space."""
    pbits = 3
    e = [int(AK.agg_at(pbits, p, 5, 1)[0]) for p in range(8)]
    hs = np.array([e[7], e[7], e[0],            # call 2: records 0..2
                   e[1], e[1], e[2], e[5],      # call 0: records 3..6
                   0xDEAD], np.uint32)          # (not part of any call)
    hcs, hcnt = np.array([3, 7, 0], np.uint64), np.array([4, 0, 3], np.uint32)
    c = AK.cell_counts(hs, hcs, hcnt, pbits, 1)
    assert c.tolist() == [[0, 2, 1, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0, 2]]
    assert AK.cell_counts(hs, hcs, hcnt, pbits, 0).tolist() == [[0, 2, 1, 0, 0, 1, 0, 0], [0] * 8,
                                                                [1, 0, 0, 0, 0, 0, 0, 2]]
    assert AK.cell_counts(hs[:0], hcs[:0], hcnt[:0], pbits, 1).shape == (0, 8)


def test_cell_capacity_and_fits_capped():
    # m = 0 -> 64; m = 1000: 1000 + 6 * 31.62 = 1189 -> 1189 + 127 = 1316 -> 1280
    # m = 1 -> (1 + 6) + 127 = 134 -> 128
    assert AK.cell_capacity([0, 8000, 8], 8).tolist() == [64, 1280, 128]
    # without slack: m = 0 -> 64, m = 1 -> 128, m = 64 -> 191 -> 128, m = 65 -> 192
    assert AK.cell_capacity([0, 8, 64 * 8, 65 * 8], 8, sd=0.0).tolist() == [64, 128, 128, 192]
    ok = np.zeros((2, 8), np.int64)
    ok[0, 3] = 64
    assert AK.fits_capped(ok)
    ok[0, 3] = 65  # m = 65 / 8 = 8.1: 8.1 + 6 * 2.85 = 25 -> 128
    assert AK.fits_capped(ok)
    ok[0, 3] = 129
    assert not AK.fits_capped(ok)


def test_staircase_cases_cover_every_order_and_m0_state():
    elems, orders, (hs, hcs, hcnt, hprio), (m0e, m0p) = AK.staircase_cases()
    assert len(orders) == AK.STAIR_ORDERS == 64 and len(set(orders)) == 64
    assert all(1 <= len(o) <= 4 and len(set(o)) == len(o) and set(o) <= {0, 1, 2, 3} for o in orders)
    assert elems.size == 320 and np.unique(elems).size == 320
    # every element's calls, read back from the batch: its order, then the dominated repeat
    assert hcnt.size == 17 and hprio.tolist() == [0, 1, 2, 3] * 4 + [0] and int(hcnt.sum()) == hs.size == 1300
    seen = {int(e): [] for e in elems}
    for c in range(17):
        rec = hs[int(hcs[c]):int(hcs[c]) + int(hcnt[c])]
        assert np.unique(rec).size == rec.size
        for e in rec:
            seen[int(e)].append(int(hprio[c]))
    m0 = dict(zip(m0e.tolist(), m0p.tolist()))
    got = {(tuple(seen[int(e)][:-1]), m0.get(int(e))) for e in elems}
    assert all(seen[int(e)][-1] == 0 for e in elems)
    assert got == {(o, m) for o in orders for m in AK.STAIR_M0} and len(got) == 320
    assert m0e.size == 256 and (np.diff(m0e.astype(np.int64)) > 0).all()
    # 8 partitions of 40; 4 elements per home bucket of a 2048-bucket table
    p, _ = AK.elem_home(elems, 3)
    assert np.bincount(p, minlength=8).tolist() == [40] * 8
    hb = np.bincount((fmix32_np(elems) >> np.uint32(21)).astype(np.int64))
    assert set(hb[hb > 0].tolist()) == {4}
    assert AK.fits_capped(AK.cell_counts(hs, hcs, hcnt, 3, 1))
    # table sizes (table.hip buckets_for: the power of two >= n + 1, from 2): the
    # planned run reserves for the 320 distinct elements and stays under 2048
    # buckets; the one-sync run reserves for the 1300 records and reaches them
    buckets_for = lambda n: max(2, 1 << int(n).bit_length())  # noqa: E731
    assert buckets_for(256) == 512 and 256 + 320 <= 0.75 * 2 * 512 and buckets_for(320) == 512
    assert buckets_for(256 + 1300) == 2048 and buckets_for(1300) == 2048
