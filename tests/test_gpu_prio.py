"""GPU: call priorities and the choice table (syzsig_calc_prios_dev,
syzsig_static_prio_finish_dev, syzsig_choice_table_dev,
syzsig_choice_lookup_dev; syzkaller_amd/prio.py) against tests/prio_ref.py, the
restatement of prog/prio.go:133-245.  Floats are compared bit for bit on their
uint32 view, NaN cells by position; outputs are pre-filled so that an unwritten
or a wrongly written cell shows; the paths taken are asserted from
syzsig_prio_stats."""
import ctypes

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, prio
from tests import prio_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
FILL = -7.25
MAXN = _lib.SYZSIG_PRIO_MAX_CALLS


def assert_same(got, exp):
    got, exp = np.asarray(got, F), np.asarray(exp, F)
    assert got.shape == exp.shape
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), f"NaN cells differ at {np.argwhere(gn != en)[:4].tolist()}"
    g, e = got.view(np.uint32), exp.view(np.uint32)
    bad = np.argwhere((g != e) & ~gn)
    assert bad.size == 0, (f"{len(bad)} cells differ, first {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def dev_prios(gpu, corpus, n, static=None, split=0):
    """calculate_priorities into a pre-filled output with a guard row behind it."""
    out = torch.full((n * n + n,), FILL, dtype=torch.float32, device=gpu.dev)
    got = gpu.calculate_priorities(corpus, n, static=static, split=split, out=out[: n * n].view(n, n))
    o = out.cpu().numpy()
    assert got.data_ptr() == out.data_ptr() and (o[n * n:] == F(FILL)).all(), "wrote past the matrix"
    return o[: n * n].reshape(n, n), gpu.prio_stats()


def sum_sq(corpus):
    return sum(len(p) ** 2 for p in corpus)


def plan(corpus, n, split):
    """(rows whole, rows split, slices) as the header states them"""
    occ = np.bincount(np.concatenate([np.asarray(p, np.int64) for p in corpus] + [np.empty(0, np.int64)]), minlength=n)
    cut = occ > split
    return int((~cut).sum()), int(cut.sum()), int(((occ[cut] + split - 1) // split).sum())


def check_corpus(gpu, corpus, n, static=None, split=0):
    got, stats = dev_prios(gpu, corpus, n, static, split)
    assert_same(got, R.calculate_priorities(corpus, n, static))
    assert stats[3] == sum_sq(corpus)
    assert stats[:3] == plan(corpus, n, split or _lib.SYZSIG_PRIO_SPLIT)
    return got, stats


def rand_corpus(rng, n, nprog, lens, skip=None):
    """programs of the given lengths over ids of [0, n) without `skip`; ids 0 and
    n - 1 are both in the first non-empty program that has room"""
    ids = np.array([i for i in range(n) if i != skip], np.int64)
    out = []
    for k in range(nprog):
        ln = int(lens[k % len(lens)])
        p = ids[rng.integers(0, ids.size, ln)]
        if ln >= 2 and 0 != skip and n - 1 != skip:
            p[0], p[-1] = 0, n - 1
        out.append(p.tolist())
    return out


# ---- corpus shapes ----

@pytest.mark.parametrize("n", [1, 2, 4, 63, 64, 65, 257, 1000])
def test_corpus_shapes(gpu, n):
    """Every N across the wave and block seams x nprog in {0, 1, 2, 257}, with
    program lengths 0, 1, 30 and 300 (past one block), ids 0 and N - 1, and an
    id that occurs nowhere (its row is ones)."""
    rng = np.random.default_rng(n)
    skip = n // 2 if n > 2 else None
    for nprog, lens in ((0, [0]), (1, [30]), (1, [0]), (2, [1, 300]), (257, [30, 0, 1, 300, 7])):
        corpus = rand_corpus(rng, n, nprog, lens, skip)
        got, _ = check_corpus(gpu, corpus, n)
        if skip is not None:
            assert (got[skip] == 1).all()
        if nprog == 0:
            assert (got == 1).all()


def test_one_long_program(gpu):
    """One program of 5000 calls among short ones: 2.5e7 pairs from one posting list."""
    rng = np.random.default_rng(11)
    corpus = rand_corpus(rng, 257, 3, [5, 5000, 12])
    check_corpus(gpu, corpus, 257)


def test_off_ids_tensors(gpu):
    """The (off, ids) form, with empty programs at both ends."""
    corpus = [[], [0, 1, 1], [], [2], []]
    off = torch.tensor([0, 0, 3, 3, 4, 4], dtype=torch.int64)
    ids = torch.tensor([0, 1, 1, 2], dtype=torch.int32)
    got = gpu.calculate_priorities((off, ids), 4).cpu().numpy()
    assert_same(got, R.calculate_priorities(corpus, 4))


# ---- arithmetic ----

CORPUS_13_2_1_0 = [[0, 1], [0, 1], [0, 2]] + [[0]] * 10


def test_row_13_2_1_0_is_not_contracted(gpu):
    """Counts [13, 2, 1, 0]: the second cell is 0.208 (weight 208) only when
    q * 0.9 + 0.1 is two roundings; a fused multiply-add gives 0.20799999 and 207."""
    got, _ = dev_prios(gpu, CORPUS_13_2_1_0, 4)
    assert_same(got[0], np.array([1, 0.208, 0.136, 0.1], F))
    assert_same(got, R.calculate_priorities(CORPUS_13_2_1_0, 4))
    fused = R.calc_dynamic_prio(CORPUS_13_2_1_0, 4, fused=True)
    assert got[0, 1] != fused[0, 1]
    t = gpu.choice_table(got, None, 4)
    assert t.run.cpu().numpy()[0].tolist() == [1000, 1208, 1344, 1444]
    assert np.array_equal(t.run.cpu().numpy(), R.build_choice_table(got, None, 4))


def test_nan_rows(gpu):
    """[a, b] at N = 2: every row is 0 / 0.  calc_prios gives NaN as Go does; the
    choice table refuses it, names the first row and writes nothing."""
    got, _ = dev_prios(gpu, [[0, 1]], 2)
    assert np.isnan(got).all()
    # a matrix whose rows 1 and 2 hold a NaN
    m = np.array([[1, 1, 0.1], [np.nan, 1, 1], [1, np.nan, 1]], F)
    out = torch.full((3, 3), -5, dtype=torch.int32, device=gpu.dev)
    with pytest.raises(_lib.SyzsigError) as ei:
        prio.ChoiceTable.build(gpu, m, None, 3, out=out)
    assert ei.value.code == _lib.SYZSIG_EINVAL and "row 1 " in str(ei.value)
    assert (out.cpu().numpy() == -5).all()
    # disabled, the NaN cells are not looked at
    t = prio.ChoiceTable.build(gpu, m, [1, 0, 0], 3, out=out)
    assert np.array_equal(t.run.cpu().numpy(), R.build_choice_table(m, [1, 0, 0], 3))
    for bad in (-0.5, 2.0 ** 21):  # negative; 2^21 * 1000 >= 2^31 / 3
        m = np.full((3, 3), 0.5, F)
        m[2, 1] = bad
        with pytest.raises(_lib.SyzsigError) as ei:
            gpu.choice_table(m, None, 3)
        assert ei.value.code == _lib.SYZSIG_EINVAL and "row 2 " in str(ei.value)
        assert np.array_equal(gpu.choice_table(m, [1, 0, 1], 3).run.cpu().numpy(),
                              R.build_choice_table(m, [1, 0, 1], 3))


def test_cell_clamped_at_two_to_the_24(gpu):
    """4097 copies of a next to b, b, c: 16785409 pairs on one cell, which a
    float32 `+= 1.0` leaves at 2^24.  4097 postings also pass the default split."""
    corpus = [[0] * 4097 + [1, 1, 2]]
    got, stats = check_corpus(gpu, corpus, 3)
    unclamped = F(F(F(F(4097) / F(F(16785409) - F(4097))) * F(0.9)) + F(0.1))
    assert got[0, 1].view(np.uint32) != unclamped.view(np.uint32)
    assert stats[1] == 1 and stats[2] == 2


# ---- the split path ----

def hot_corpus(rng, n, nprog):
    """id 0 in every program (the mmap of a real corpus), the rest random"""
    if n == 1:
        return [[0]] * nprog
    return [[0] + rng.integers(1, n, int(rng.integers(0, 12))).tolist() for _ in range(nprog)]


@pytest.mark.parametrize("split", [1, 2, 7])
def test_split_gives_the_same_result(gpu, split):
    rng = np.random.default_rng(split)
    n = 65
    corpus = hot_corpus(rng, n, 40)
    whole, ws = dev_prios(gpu, corpus, n, split=0)
    assert ws[1] == 0 and ws[2] == 0 and ws[0] == n  # nothing reaches the default threshold
    got, st = check_corpus(gpu, corpus, n, split=split)
    assert st[1] >= 1 and st[2] >= 40 // split  # id 0's row at the least
    assert_same(got, whole)
    static = rng.random((n, n)).astype(F)
    got_s, _ = check_corpus(gpu, corpus, n, static=static, split=split)
    assert_same(got_s, dev_prios(gpu, corpus, n, static=static)[0])


@pytest.mark.parametrize("split", [1, 2, 7])
def test_slice_boundary(gpu, split):
    """id 1 occurs exactly `split` times: counted whole.  id 2 occurs split + 1
    times: two slices, the second of one posting.  id 3 occurs 2 * split + 1
    times, twice in one program."""
    corpus = [[1, 4]] * split + [[2, 5]] * (split + 1) + [[3, 3, 6]] + [[3]] * (2 * split - 1)
    got, st = check_corpus(gpu, corpus, 8, split=split)
    occ = {1: split, 2: split + 1, 3: 2 * split + 1, 4: split, 5: split + 1, 6: 1}
    exp_cut = sum(1 for c in occ.values() if c > split)
    exp_slices = sum((c + split - 1) // split for c in occ.values() if c > split)
    assert st == (8 - exp_cut, exp_cut, exp_slices, sum_sq(corpus))
    assert_same(got, dev_prios(gpu, corpus, 8)[0])


# ---- errors ----

def raw_calc(gpu, off, ids, n, out, nprog=None, total=None):
    off = torch.as_tensor(np.asarray(off, np.int64)).to(gpu.dev)
    ids = torch.as_tensor(np.asarray(ids, np.uint32).view(np.int32)).to(gpu.dev)
    gpu.sync_stream()
    return gpu.L.syzsig_calc_prios_dev(gpu.eng.h, ctypes.c_void_p(off.data_ptr()),
                                       ctypes.c_void_p(ids.data_ptr() if ids.numel() else 0),
                                       off.numel() - 1 if nprog is None else nprog,
                                       ids.numel() if total is None else total, n, 0, None,
                                       ctypes.c_void_p(out.data_ptr()))


def test_errors_leave_the_output_untouched(gpu):
    n = 5
    out = torch.full((n * n,), FILL, dtype=torch.float32, device=gpu.dev)

    def untouched():
        return (out.cpu().numpy() == F(FILL)).all()

    # an id == N: Go would panic on the index
    assert raw_calc(gpu, [0, 2, 3], [0, 4, n], n, out) == _lib.SYZSIG_EINVAL and untouched()
    assert b"call id" in gpu.L.syzsig_last_error()
    # N past the LDS row: nothing is read (out is far too small for such a matrix)
    assert raw_calc(gpu, [0, 1], [0], MAXN + 1, out) == _lib.SYZSIG_ERANGE and untouched()
    assert raw_calc(gpu, [0, 1], [0], 0, out) == _lib.SYZSIG_EINVAL and untouched()
    # one program of 65536 calls: 2^32 pairs; found before any counting
    assert raw_calc(gpu, [0, 65536], np.zeros(65536, np.uint32), n, out) == _lib.SYZSIG_ERANGE and untouched()
    # ... and 65535 calls next to one more program pass 2^32 together
    assert raw_calc(gpu, [0, 65535, 65535 + 363], np.zeros(65535 + 363, np.uint32), n, out) == _lib.SYZSIG_ERANGE
    assert untouched()
    # offsets that decrease, that do not start at 0, that do not end at total
    for off in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 3]):
        assert raw_calc(gpu, off, [0, 1, 2, 3], n, out) == _lib.SYZSIG_EINVAL and untouched()
    assert raw_calc(gpu, [0], [0, 1], n, out, nprog=0, total=2) == _lib.SYZSIG_EINVAL and untouched()
    # the call after an error is unaffected
    assert raw_calc(gpu, [0, 2], [0, 4], n, out) == _lib.SYZSIG_OK
    assert_same(out.cpu().numpy().reshape(n, n), R.calc_dynamic_prio([[0, 4]], n))


# ---- the static tail and the table ----

@pytest.mark.parametrize("n", [1, 65, 257])
def test_static_tail(gpu, n):
    rng = np.random.default_rng(n)
    m = (rng.random((n, n)) * rng.choice([0, 0, 1, 3], size=(n, n))).astype(F)
    np.fill_diagonal(m, 0)
    if n > 2:
        m[n // 2] = 0          # a call that shares nothing: ones
        m[1, :] = 0
        m[1, 0] = 2.5          # one non-zero cell: the diagonal takes it
    got = gpu.static_finish(m).cpu().numpy()
    exp = R.static_finish(m)
    assert_same(got, exp)
    # ... and as the static factor of CalculatePriorities
    corpus = rand_corpus(rng, n, 20, [3, 9, 1])
    check_corpus(gpu, corpus, n, static=exp)


def masks(rng, n):
    yield None
    yield np.zeros(n, np.uint8)
    one = np.zeros(n, np.uint8)
    one[n - 1] = 1
    yield one
    one = np.zeros(n, np.uint8)
    one[0] = 1
    yield one
    for p in (0.5, 0.9):
        yield (rng.random(n) < p).astype(np.uint8)
    edge = np.ones(n, np.uint8)  # disabled first / last / adjacent
    edge[[0, n - 1]] = 0
    if n > 4:
        edge[[n // 2, n // 2 + 1]] = 0
    yield edge


@pytest.mark.parametrize("n", [1, 4, 64, 257, 1000])
def test_choice_table(gpu, n):
    rng = np.random.default_rng(n)
    prios = R.calculate_priorities(hot_corpus(rng, n, 60), n)
    prios[np.isnan(prios)] = F(0.5)
    for en in masks(rng, n):
        for p in (None, prios):
            out = torch.full((n * n + n,), -3, dtype=torch.int32, device=gpu.dev)
            t = prio.ChoiceTable.build(gpu, p, en, n, out=out[: n * n].view(n, n))
            o = out.cpu().numpy()
            assert (o[n * n:] == -3).all()
            assert np.array_equal(o[: n * n].reshape(n, n), R.build_choice_table_fast(p, en, n))
            assert t.run.data_ptr() == out.data_ptr()


# ---- lookup ----

def test_lookup_every_x(gpu):
    n = 7
    en = np.array([1, 0, 1, 1, 0, 1, 0], np.uint8)
    prios = R.calculate_priorities([[0, 2, 3], [0, 5], [0, 0, 3], [2]], n)
    prios[np.isnan(prios)] = F(0.25)
    t = gpu.choice_table(prios, en, n)
    run = R.build_choice_table(prios, en, n)
    assert np.array_equal(t.run.cpu().numpy(), run)
    calls, xs = [], []
    for c in np.flatnonzero(en):
        total = int(run[c, -1])
        calls += [c] * total
        xs += range(1, total + 1)
    got = t.lookup(calls, xs).cpu().numpy()
    exp = np.array([np.searchsorted(run[c], x, side="left") for c, x in zip(calls, xs)])
    assert np.array_equal(got, exp)
    assert en[got].all() and len(set(got.tolist())) == int(en.sum())
    assert exp.tolist() == [R.lookup(run, en, c, x) for c, x in zip(calls, xs)]
    # the sentinel: call < 0, a disabled row -- whatever x is
    assert t.lookup([-1, -5, 1, 4, 6], [1, 0, 1, 99, -2]).cpu().numpy().tolist() == [n] * 5
    # x outside [1, total], a call >= N: EINVAL, nothing written
    total0 = int(run[0, -1])
    out = torch.full((3,), -9, dtype=torch.int32, device=gpu.dev)
    for c, x in (([0, 0, 0], [1, 0, 2]), ([0, 0, 0], [1, total0 + 1, 2]), ([0, n, 0], [1, 1, 1])):
        with pytest.raises(_lib.SyzsigError) as ei:
            t.lookup(c, x, out=out)
        assert ei.value.code == _lib.SYZSIG_EINVAL and (out.cpu().numpy() == -9).all()
    assert t.lookup([0, 0, 0], [1, total0, 2], out=out).cpu().numpy().tolist() == \
        [R.lookup(run, en, 0, x) for x in (1, total0, 2)]
    assert t.lookup([], []).numel() == 0


def test_choose(gpu):
    n = 7
    en = np.array([1, 0, 1, 1, 0, 1, 0], np.uint8)
    t = gpu.choice_table(None, en, n)
    rng = np.random.default_rng(3)
    got = t.choose(rng, np.array([-1, 0, 1, 2, 3, 4, 5, 6] * 40))
    assert en[got].all() and set(got.tolist()) == set(np.flatnonzero(en).tolist())
    assert isinstance(t.choose(rng, 0), int)


# ---- the chain ----

def test_chain_against_the_restatement(gpu):
    """ids -> calculate_priorities -> ChoiceTable.build -> lookup, end to end:
    N = 300, 2000 programs, Zipf ids, a static matrix, a mask."""
    rng = np.random.default_rng(2024)
    n = 300
    corpus = [np.minimum(rng.zipf(1.3, int(rng.integers(1, 31))) - 1, n - 1).tolist() for _ in range(2000)]
    raw = (rng.random((n, n)) * (rng.random((n, n)) < 0.2)).astype(F)
    np.fill_diagonal(raw, 0)
    static = R.static_finish(raw)
    en = (rng.random(n) < 0.8).astype(np.uint8)
    en[0] = 1
    exp_p = R.calculate_priorities(corpus, n, static)
    exp_run = R.build_choice_table(exp_p, en, n)
    got_static = gpu.static_finish(raw)
    assert_same(got_static.cpu().numpy(), static)
    got_p = gpu.calculate_priorities(corpus, n, static=got_static)
    assert_same(got_p.cpu().numpy(), exp_p)
    t = prio.ChoiceTable.build(gpu, got_p, en, n)
    assert np.array_equal(t.run.cpu().numpy(), exp_run)
    calls = rng.integers(-1, n, 5000)
    tot = np.where(calls >= 0, exp_run[np.clip(calls, 0, None), -1], 0)
    xs = np.where(tot > 0, rng.integers(1, np.maximum(tot, 1) + 1), 1)
    got = t.lookup(calls, xs).cpu().numpy()
    exp = np.array([R.lookup(exp_run, en, int(c), int(x)) for c, x in zip(calls, xs)])
    assert np.array_equal(got, exp)
