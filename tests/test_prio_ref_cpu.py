"""CPU: the restatement of prog/prio.go's numeric part (tests/prio_ref.py) held
to cases worked by hand in the comments below, and the host-compilable half of
csrc/prio.hip -- csrc/prio_args.h, the entry points' argument checks and the
slicing plan -- in tests/prio_driver.cc, a stand-alone program built under
ASan + UBSan.

Notation: a, b, c are call ids 0, 1, 2.  A cell of calcDynamicPrio's matrix
before normalizePrio is count[x][y] = sum over programs of occ(x) * occ(y).
normalizePrio per row: max from 0, min over the non-zero cells from 1e10, nzero
zero cells; min /= 2 * nzero when nzero != 0; max == 0 -> all 1; else a zero
cell takes min and p = (p - min) / (max - min) * 0.9 + 0.1."""
import os
import subprocess

import numpy as np
import pytest

from tests import prio_ref as R
from tests.conftest import ROOT

F = np.float32
LO = F(0.1)                 # what a cell equal to min gets: 0 / d * 0.9 + 0.1
HI = F(F(0.9) + F(0.1))     # what a cell equal to max gets: 1 * 0.9 + 0.1


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(got, exp):
    got, exp = np.asarray(got, F), np.asarray(exp, F)
    return got.shape == exp.shape and np.array_equal(np.isnan(got), np.isnan(exp)) and \
        np.array_equal(bits(got)[~np.isnan(got)], bits(exp)[~np.isnan(exp)])


def test_top_and_bottom_of_the_range():
    """float32(0.9) + float32(0.1) = 0.89999998 + 0.1 = 0.99999998, which lies
    nearer 1 than 1 - 2^-24: the max cell is exactly 1."""
    assert HI == F(1) and LO == F(0.1)


def test_empty_corpus_is_all_ones():
    """No program: every count 0, so max == 0 in every row and every cell is 1."""
    assert same(R.calc_dynamic_prio([], 3), np.ones((3, 3), F))
    assert same(R.calc_dynamic_prio([[], []], 3), np.ones((3, 3), F))
    assert R.calc_dynamic_prio([], 0).shape == (0, 0)


def test_single_call_program():
    """[a] at N = 1: count = [[1]]; max = min = 1, nzero = 0, p = 0 / 0: NaN.
    [a] at N = 2: row a = [1, 0]: nzero = 1, min = 1 / 2 = 0.5; a: 0.5 / 0.5 -> 1;
    the zero cell takes min: 0 / 0.5 -> 0.1.  Row b is all zeros -> ones."""
    got = R.calc_dynamic_prio([[0]], 1)
    assert got.shape == (1, 1) and np.isnan(got[0, 0])
    assert same(R.calc_dynamic_prio([[0]], 2), [[1, LO], [1, 1]])


def test_two_call_program_nan_rows():
    """[a, b] at N = 2: every count is 1, every row [1, 1]: max = min, 0 / 0 in
    every cell -- Go yields NaN, and so does the restatement."""
    assert np.isnan(R.calc_dynamic_prio([[0, 1]], 2)).all()


def test_two_call_program_at_three_calls():
    """[a, b] at N = 3: rows a and b are [1, 1, 0]: min = 1 / 2; the ones give
    0.5 / 0.5 -> 1, the zero cell 0.1.  Row c is zeros -> ones."""
    assert same(R.calc_dynamic_prio([[0, 1]], 3), [[1, 1, LO], [1, 1, LO], [1, 1, 1]])


def test_repeated_call():
    """[a, a, b]: occ(a) = 2, occ(b) = 1: aa = 4, ab = ba = 2, bb = 1 -- self-pairs
    and repeats included.  N = 2: row a = [4, 2]: (4 - 2) / 2 -> 1, (2 - 2) / 2 ->
    0.1; row b = [2, 1] likewise.  N = 3: row a = [4, 2, 0]: min = 2 / 2 = 1;
    4: 3 / 3 -> 1; 2: 1 / 3 * 0.9 + 0.1; 0 -> 0.1."""
    assert np.array_equal(R.pair_counts([[0, 0, 1]], 2), [[4, 2], [2, 1]])
    assert same(R.calc_dynamic_prio([[0, 0, 1]], 2), [[1, LO], [1, LO]])
    third = F(F(F(F(1) / F(3)) * F(0.9)) + F(0.1))
    half = F(F(F(F(0.5) / F(1.5)) * F(0.9)) + F(0.1))  # row b = [2, 1, 0]: min = 1 / 2; 1: 0.5 / 1.5
    assert same(R.calc_dynamic_prio([[0, 0, 1]], 3), [[1, third, LO], [1, half, LO], [1, 1, 1]])


def test_min_is_divided_by_twice_the_zero_cells():
    """Row [8, 4, 0, 0]: min = 4, nzero = 2 -> min = 4 / (2 * 2) = 1.  8: 7 / 7 -> 1;
    4: 3 / 7 * 0.9 + 0.1; the zero cells: (1 - 1) / 7 -> 0.1."""
    row = R.normalize_row(np.array([8, 4, 0, 0], F))
    mid = F(F(F(F(3) / F(7)) * F(0.9)) + F(0.1))
    assert same(row, [1, mid, LO, LO])
    # without the division min would stay 4 and the 4 would fall to 0.1
    assert mid > F(0.4)


CORPUS_13_2_1_0 = [[0, 1], [0, 1], [0, 2]] + [[0]] * 10


def test_row_13_2_1_0_unfused_and_fused():
    """Two [a, b], one [a, c], ten [a], N = 4: row a = [13, 2, 1, 0].  min = 1,
    nzero = 1 -> 0.5; max - min = 12.5.  13 -> 1; 2: 1.5 / 12.5 = 0.12, * 0.9 =
    0.108, + 0.1 = 0.208; 1: 0.5 / 12.5 = 0.04 -> 0.136; 0 -> 0.1.  The weights
    int(p * 1000) are 1000, 208, 136, 100.  With q * 0.9 + 0.1 fused into one
    rounding the second cell is 0.20799999 and its weight 207: the choice table
    differs, which is why the kernel must not contract."""
    assert np.array_equal(R.pair_counts(CORPUS_13_2_1_0, 4)[0], [13, 2, 1, 0])
    row = R.calc_dynamic_prio(CORPUS_13_2_1_0, 4)[0]
    assert same(row, [1, F(0.208), F(0.136), F(0.1)])
    w = [int(F(p * F(1000))) for p in row]
    assert w == [1000, 208, 136, 100]
    fused = R.calc_dynamic_prio(CORPUS_13_2_1_0, 4, fused=True)[0]
    assert int(F(fused[1] * F(1000))) == 207 and fused[1] < row[1]
    assert same(R.normalize_row(np.array([13, 2, 1, 0], F), fused=True), fused)


def test_clamp_to_one():
    """p <= max in every row, a correctly rounded quotient of num <= den is <= 1,
    and 0.9 + 0.1 rounds to exactly 1: with every operation rounded on its own
    the clamp `if p > 1` never fires on finite input, and the max cell is
    exactly 1.  Held on random rows, with negative and huge cells as well."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        row = rng.choice([0, 0, 1, 2, 3, 1000, 16777216, -4, 3e10, 0.37], size=rng.integers(1, 9)).astype(F)
        out = R.normalize_row(row.copy())
        ok = ~np.isnan(out)
        assert (out[ok] <= 1).all()  # (a negative min halved leaves cells below it: no lower bound)
        if ok.all() and row.max() > 0 and np.unique(row[row != 0]).size > 1:
            assert out[np.argmax(row)] == F(1)


def test_cell_sticks_at_two_to_the_24():
    """float32 2^24 + 1 rounds back to 2^24, so `+= 1.0` sticks there.  4096
    copies of a next to b, b, c: aa = 4096^2 = 2^24 exactly.  4097 copies: aa =
    16785409 pairs but the cell is 2^24; ab = 2 * 4097, ac = 4097.  Row a:
    min = 4097, max = 2^24; b: 4097 / (2^24 - 4097) * 0.9 + 0.1."""
    assert F(2 ** 24) + F(1) == F(2 ** 24)
    for copies, pairs in ((4096, 1 << 24), (4097, 16785409)):
        prog = [0] * copies + [1, 1, 2]
        cnt = R.pair_counts([prog], 3)
        assert cnt[0].tolist() == [pairs, 2 * copies, copies]
        assert R.counts_to_f32(cnt)[0, 0] == F(2 ** 24)
        row = R.calc_dynamic_prio([prog], 3)[0]
        b = F(F(F(F(copies) / F(F(2 ** 24) - F(copies))) * F(0.9)) + F(0.1))
        assert same(row, [1, b, LO])
    unclamped = F(F(F(F(4097) / F(F(16785409) - F(4097))) * F(0.9)) + F(0.1))
    assert bits(unclamped) != bits(b)  # the clamp is visible in the row


def test_static_tail():
    """[[0, 3, 1], [2, 0, 0], [0, 0, 0]]: the diagonal takes each row's max:
    [3, 3, 1], [2, 2, 0], [0, 0, 0].  Row 0: min 1, no zeros: 2 / 2 -> 1, 1, 0.1.
    Row 1: min = 2 / 2 = 1: 1 / 1 -> 1, 1, and the zero cell 0.1.  Row 2 -> ones."""
    m = np.array([[0, 3, 1], [2, 0, 0], [0, 0, 0]], F)
    assert same(R.static_finish(m), [[1, 1, LO], [1, 1, LO], [1, 1, 1]])
    assert m[0, 0] == 0  # the input is left alone
    # CalculatePriorities multiplies cell by cell: row a of [a, b] at N = 3 is [1, 1, 0.1]
    st = R.static_finish(m)
    assert same(R.calculate_priorities([[0, 1]], 3, st)[0], [1, 1, F(LO * LO)])


def test_vectorised_rows_match_the_loop():
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 17):
        m = rng.choice([0, 0, 0, 1, 1, 2, 5, 40, 16777216], size=(12, n)).astype(F)
        m[0] = 0
        m[1] = 3
        for fused in (False, True):
            exp = np.stack([R.normalize_row(r.copy(), fused) for r in m])
            assert same(R.normalize_prio(m, fused), exp)
    m = rng.standard_normal((6, 9)).astype(F)
    m[m > 1] = 0
    assert same(R.normalize_prio(m), np.stack([R.normalize_row(r.copy()) for r in m]))


def test_build_choice_table():
    """nil prios: every enabled weight is 1.  A disabled row is zeros; a disabled
    column repeats the sum before it."""
    assert R.build_choice_table(None, None, 4).tolist() == [[1, 2, 3, 4]] * 4
    # first and last disabled
    assert R.build_choice_table(None, [0, 1, 1, 0], 4).tolist() == [[0] * 4, [0, 1, 2, 2], [0, 1, 2, 2], [0] * 4]
    # adjacent disabled columns
    assert R.build_choice_table(None, [1, 0, 0, 1], 4).tolist() == [[1, 1, 1, 2], [0] * 4, [0] * 4, [1, 1, 1, 2]]
    assert R.build_choice_table(None, [0, 0, 0, 0], 4).tolist() == [[0] * 4] * 4
    # weights of the pinned row: 1000, 208, 136, 100
    prios = R.calc_dynamic_prio(CORPUS_13_2_1_0, 4)
    assert R.build_choice_table(prios, None, 4)[0].tolist() == [1000, 1208, 1344, 1444]
    assert R.build_choice_table(prios, [1, 0, 1, 1], 4)[0].tolist() == [1000, 1000, 1136, 1236]
    # a NaN row has no defined weights; disabled, it is not looked at
    nan = R.calc_dynamic_prio([[0, 1]], 2)
    with pytest.raises(ValueError, match="row 0"):
        R.build_choice_table(nan, None, 2)
    assert R.build_choice_table(nan, [0, 0], 2).tolist() == [[0, 0], [0, 0]]
    with pytest.raises(ValueError, match="row 1"):
        R.build_choice_table(np.array([[1, 1], [1, -1]], F), None, 2)
    with pytest.raises(ValueError):
        R.build_choice_table(np.array([[2 ** 21, 1], [1, 1]], F), None, 2)  # 2^21 * 1000 >= 2^31 / 2


def test_vectorised_table_matches_the_loop():
    rng = np.random.default_rng(9)
    for n in (1, 2, 9, 33):
        prios = rng.random((n, n)).astype(F)
        for en in (None, np.zeros(n, np.uint8), (rng.random(n) < 0.6).astype(np.uint8)):
            for p in (None, prios):
                assert np.array_equal(R.build_choice_table_fast(p, en, n), R.build_choice_table(p, en, n))
    bad = np.full((3, 3), 0.5, F)
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="row 1"):
        R.build_choice_table_fast(bad, None, 3)
    assert np.array_equal(R.build_choice_table_fast(bad, [1, 1, 0], 3), R.build_choice_table(bad, [1, 1, 0], 3))


def test_search_ints():
    """run = [1000, 1208, 1344, 1444]: x = 1 and x = 1000 -> 0; 1001 -> 1; each
    boundary belongs to the cell it closes; the total -> the last cell."""
    run = [1000, 1208, 1344, 1444]
    exp = {1: 0, 1000: 0, 1001: 1, 1208: 1, 1209: 2, 1344: 2, 1345: 3, 1444: 3, 1445: 4}
    assert {x: R.search_ints(run, x) for x in exp} == exp
    for x in range(1, 1445):
        assert R.search_ints(run, x) == int(np.searchsorted(run, x, side="left"))
    # disabled columns are never landed on: run = [0, 1, 2, 2] (columns 0 and 3 disabled)
    t = R.build_choice_table(None, [0, 1, 1, 0], 4)
    assert [R.lookup(t, [0, 1, 1, 0], 1, x) for x in (1, 2)] == [1, 2]
    # the sentinel: call < 0 or a disabled row
    assert R.lookup(t, [0, 1, 1, 0], -1, 1) == 4 and R.lookup(t, [0, 1, 1, 0], 0, 1) == 4
    for x in (0, 3):
        with pytest.raises(ValueError):
            R.lookup(t, [0, 1, 1, 0], 1, x)


# ---- csrc/prio_args.h on the CPU, under ASan + UBSan ----

def test_argument_checks_under_sanitizer(tmp_path):
    exe = str(tmp_path / "prio_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "prio_driver.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "0 failures" in r.stdout
