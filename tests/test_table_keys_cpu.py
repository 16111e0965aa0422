"""CPU: tests/table_keys.py -- the inverse hash and the home buckets of the
key sets that tests/test_gpu_table_edges.py builds its probe chains from."""
import numpy as np
import pytest

from tests import table_keys as TK

NBS = [2, 16, 1 << 10, 1 << 20]


def _fmix32_int(h):
    """murmur3 fmix32 on a Python int (independent of numpy's wrap-around)."""
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def test_fmix32_matches_scalar_definition():
    rng = np.random.default_rng(0)
    x = np.concatenate([np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32),
                        rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)])
    assert TK.fmix32_np(x).tolist() == [_fmix32_int(int(v)) for v in x]


def test_fmix32_inverse_round_trip():
    rng = np.random.default_rng(1)
    edge = np.array([0, 1, 2, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    h = np.concatenate([edge, rng.integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32)])
    np.testing.assert_array_equal(TK.fmix32_np(TK.fmix32_inv_np(h)), h)
    np.testing.assert_array_equal(TK.fmix32_inv_np(TK.fmix32_np(h)), h)


@pytest.mark.parametrize("nb", NBS)
def test_home_bucket_formula(nb):
    rng = np.random.default_rng(nb)
    e = rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32)
    assert TK.home_bucket(e, nb).tolist() == [(_fmix32_int(int(v)) * nb) >> 32 for v in e]


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("n", [1, 9, 3000])
def test_hot_sets_home_where_they_say(nb, n):
    n = min(n, (1 << 32) // nb)
    last, first = TK.hot_last(n), TK.hot_first(n)
    assert (TK.home_bucket(last, nb) == nb - 1).all()
    assert (TK.home_bucket(first, nb) == 0).all()
    assert np.unique(np.concatenate([last, first])).size == 2 * n
    for b in sorted({0, 1, nb // 2, nb - 1}):
        at = TK.hot_at(nb, b, n)
        assert (TK.home_bucket(at, nb) == b).all()
        assert np.unique(at).size == n
        if b:  # the key before the first one belongs to the bucket below
            h0 = int(TK.fmix32_np(at[:1])[0])
            assert (h0 - 1) * nb >> 32 == b - 1


def test_hot_sets_skip_and_limits():
    a, b = TK.hot_last(20), TK.hot_last(20, skip=20)
    np.testing.assert_array_equal(np.concatenate([a, b]), TK.hot_last(40))
    np.testing.assert_array_equal(np.concatenate([TK.hot_first(5), TK.hot_first(7, skip=5)]), TK.hot_first(12))
    # 40000 keys: one home bucket in a table of 2^16 buckets, two in one of 2^17
    big = TK.hot_last(40000)
    assert np.unique(big).size == 40000
    assert (TK.home_bucket(big, 1 << 16) == (1 << 16) - 1).all()
    assert sorted(set(TK.home_bucket(big, 1 << 17).tolist())) == [(1 << 17) - 2, (1 << 17) - 1]
    with pytest.raises(AssertionError):
        TK.hot_at(1 << 20, 3, (1 << 12) + 1)
