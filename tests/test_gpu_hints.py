"""GPU: prog.shrinkExpand (prog/hints.go:164-218, syzsig_shrink_expand_dev)
against the CompMaps of syzsig_comp_map_dev, bit for bit against
tests/comps_ref.py."""
import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, synth
from syzkaller_amd.hints import SPECIAL_INTS, CompMap
from tests import comps_ref as R
from tests.test_gpu_comps import OUT, dev_i32, dev_i64, u32, u64

pytestmark = pytest.mark.gpu

T = _lib.SYZSIG_COMPS_TILE
M64 = (1 << 64) - 1


def csr(gpu, maps):
    """dict maps -> (map_off, pairs) device tensors"""
    ps = [R.map_pairs(m) for m in maps]
    off = np.concatenate([[0], np.cumsum([p.shape[0] for p in ps])]).astype(np.uint64)
    return dev_i64(gpu, off), dev_i64(gpu, np.concatenate(ps)).view(-1, 2)


def run(gpu, maps, calls, values, special=()):
    off, pairs = csr(gpu, maps)
    ro, rep = gpu.shrink_expand(off, pairs, dev_i32(gpu, calls), dev_i64(gpu, values), special)
    ro, rep = u64(ro).tolist(), u64(rep).tolist()
    return [rep[ro[i]:ro[i + 1]] for i in range(len(calls))]


HAND = [  # (v, map, expected replacers): tests/test_comps_ref_cpu.py's cases
    (0x1122334455667788, {0x1122334455667788: {0xdeadbeefcafef00d}}, [0xdeadbeefcafef00d]),  # width 8: mask all ones
    (0x1234, {0x34: {0xab}}, [0x12ab]),                      # shrink at width 1
    (0xaa1234, {0x3412: {0xcdab}}, [0xaaabcd]),              # shrink at width 2, big-endian
    (0xff, {M64: {0x05}}, [0x05]),                           # expand at width -1
    (0x8001, {0x0180: {0x2211}}, [0x1122]),                  # expand, then swapInt truncates; width 2 agrees: once
    (0x8001, {0x0180ffffffffffff: {0x2211}}, []),
    (0x1234, {0x34: {0x1ab}}, []),                           # a wider other operand
    (0x1234, {0x34: {0xffffffffffffff80}}, [0x1280]),        # an all-ones high part
    (0xff, {M64: {M64 - 1}}, [0xfe]),
    (0x1234, {0x34: {0x40}}, []),                            # a special int
    (0x1234, {0x34: {0x41, 0x40, 0x7f}}, [0x1241]),
    (0x34, {0x34: {0xab}}, [0xab]),                          # widths 8, 4, 2, 1: one replacer
    (0x34, {0x34: {0x34}}, [0x34]),                          # equal to v: not excluded
    (0x1234, {}, []),                                        # an empty map
]


def test_shrink_expand_hand_cases(gpu):
    special = [0x40, 0x7f]
    got = run(gpu, [m for _, m, _ in HAND], list(range(len(HAND))), [v for v, _, _ in HAND], special)
    for i, (v, m, exp) in enumerate(HAND):
        assert got[i] == exp, (i, hex(v))
        assert R.shrink_expand(v, m, special) == exp, i
    # without the special ints the rejected value comes back
    assert run(gpu, [{0x34: {0x40}}], [0], [0x1234]) == [[0x1240]]


def test_shrink_expand_random_queries(gpu):
    rng = np.random.default_rng(31)
    ncalls, nq = 64, 2000
    lens = rng.integers(0, 400, ncalls).astype(np.uint32)
    comps, starts = synth.comparisons(32, lens, OUT)
    words, nw, cnt = gpu.exec_comps(dev_i64(gpu, comps), dev_i64(gpu, starts), dev_i32(gpu, lens), OUT)
    m = CompMap.from_exec_output(gpu, words, dev_i64(gpu, starts), nw, cnt)
    est, eoff, epairs, maps = R.comp_map(u32(words), 5 * starts, u32(cnt), 5 * starts + u32(nw))
    np.testing.assert_array_equal(u64(m.off), eoff)
    np.testing.assert_array_equal(u64(m.pairs).reshape(-1, 2), epairs)
    # values from the operand pool as write() and the parse leave them, some
    # below other bytes (so that only a shrink matches), some unknown
    keys = np.unique(epairs[:, 0])
    vals = keys[rng.integers(0, keys.size, nq)].copy()
    kind = rng.integers(0, 10, nq)
    shifted = (vals & np.uint64(0xffff)) | (rng.integers(1, 1 << 40, nq).astype(np.uint64) << np.uint64(16))
    vals = np.where(kind < 3, shifted, vals)
    vals = np.where(kind == 9, rng.integers(0, 1 << 62, nq).astype(np.uint64), vals)
    calls = rng.integers(0, ncalls, nq)
    eo, erep = R.shrink_expand_batch(maps, calls, vals, SPECIAL_INTS)
    ro, rep = m.shrink_expand(calls, dev_i64(gpu, vals))
    np.testing.assert_array_equal(u64(ro), eo)
    np.testing.assert_array_equal(u64(rep), erep)
    per_q = np.diff(eo.astype(np.int64))
    assert (per_q > 0).mean() > 0.5 and (per_q == 0).any()  # most queries have candidates, some have none


def test_shrink_expand_candidates_at_the_tile_edge(gpu):
    """Queries with exactly T and T + 1 candidates: only the width-8 variant of
    v finds a key, every pair of it is a candidate and none is a special int,
    so the first query's segment fills the LDS tile and the second is the
    shortest one that goes through the tiles and one merge pass."""
    v = 0x1122334455667788
    maps = [{v: {(1 << 48) + 3 * i for i in range(T)}}, {v: {(1 << 48) + 3 * i for i in range(T + 1)}}]
    exp = [R.shrink_expand(v, m, SPECIAL_INTS) for m in maps]
    assert [len(x) for x in exp] == [T, T + 1]
    assert run(gpu, maps, [0, 1], [v, v], SPECIAL_INTS) == exp


def test_shrink_expand_candidates_past_the_tile_and_erange(gpu):
    rng = np.random.default_rng(33)
    vs = set(int(x) for x in rng.integers(0, 1 << 40, 3 * T))  # widths 8, 4, 2 and 1 all find key 0x34
    maps = [{0x34: vs, 0x77: {1, 2}}, {}]
    calls, values = [0, 1, 0, 0], [0x34, 0x34, 0x5577, 0x99]
    exp = [R.shrink_expand(v, maps[c], SPECIAL_INTS) for c, v in zip(calls, values)]
    assert len(exp[0]) > T and exp[1] == [] and exp[2] == [0x5502] and exp[3] == []
    assert run(gpu, maps, calls, values, SPECIAL_INTS) == exp
    off, pairs = csr(gpu, maps)
    rep = torch.full((len(exp[0]),), 0x5e, dtype=torch.int64, device=gpu.dev)  # one short
    with pytest.raises(_lib.SyzsigError) as e:
        gpu.shrink_expand(off, pairs, dev_i32(gpu, calls), dev_i64(gpu, values), SPECIAL_INTS, rep=rep)
    assert e.value.code == _lib.SYZSIG_ERANGE and e.value.needed == len(exp[0]) + 1
    assert bool((rep == 0x5e).all())
    with pytest.raises(_lib.SyzsigError) as e:  # a query's call outside the maps
        gpu.shrink_expand(off, pairs, dev_i32(gpu, [2]), dev_i64(gpu, [1]))
    assert e.value.code == _lib.SYZSIG_EINVAL
