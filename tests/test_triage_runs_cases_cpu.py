"""No GPU: the batches of tests/triage_runs_cases.py.  The restatement of
proc.go:107-160 over the oracle's Signal ops (oracle.triage_runs /
minimize_pred) must give exactly the outcome each builder derived by hand, and
every batch must have the shape the GPU tests rely on."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import triage_runs_cases as C

CASES = C.all_cases() + [("no_runs", C.no_runs)]


def final_keep(case, finals):
    """the oracle's final newSignal per item as a per-element keep array"""
    io, el, pr = case.arrays[:3]
    ek = np.zeros(el.size, np.uint8)
    for i, f in enumerate(finals):
        a, b = int(io[i]), int(io[i + 1])
        got = {int(e): int(p) for e, p in zip(el[a:b], pr[a:b]) if f and int(e) in f}
        assert got == (f or {}), i  # a final set holds the item's own (elem, prio) pairs only
        ek[a:b] = [int(e) in (f or {}) for e in el[a:b]]
    return ek


@pytest.mark.parametrize("name,build", CASES, ids=[n for n, _ in CASES])
def test_oracle_equals_hand_expectation(name, build):
    case = build()
    io, el, pr, fl, ro, rs, rp, re, rx = case.arrays
    n = io.size - 1
    assert fl.size == n == case.keep.size == case.pred.size and case.elem_keep.size == el.size == io[-1]
    assert ro.size == n * case.runs + 1 and rp.size == re.size == rx.size == n * case.runs and ro[-1] == rs.size
    keep, finals = O.triage_runs(io, el, pr, fl, case.runs, ro, rs, rp, re, rx)
    np.testing.assert_array_equal(keep, case.keep)
    np.testing.assert_array_equal(final_keep(case, finals), case.elem_keep)
    np.testing.assert_array_equal(O.minimize_pred(io, el, pr, fl, case.runs, ro, rs, rp, re, rx), case.pred)


@pytest.mark.parametrize("name,build", C.all_cases(), ids=[n for n, _ in C.all_cases()])
def test_batch_has_both_outcomes(name, build):
    case = build()
    assert 0 < case.keep.sum() < case.keep.size
    assert 0 < case.pred.sum() < case.pred.size
    assert 0 < case.elem_keep.sum() < case.elem_keep.size


def _skipped(case):
    """runs the triage loop passes over (proc.go:122-123), per item"""
    io, _, _, fl, ro, _, _, re, rx = case.arrays
    n = io.size - 1
    empty = np.diff(ro.astype(np.int64)) == 0
    failed = (re != 0) & np.repeat((fl & C.ORIG_OK) != 0, case.runs)
    return ((rx == 0) | empty | failed).reshape(n, case.runs).sum(1), (rx == 0).sum(), empty.sum(), failed.sum()


@pytest.mark.parametrize("R", range(1, C.MAX_RUNS + 1))
def test_skip_table_reaches_the_bound(R):
    case = C.skip_table(R)
    k, noexec, empty, failed = _skipped(case)
    assert set(k.tolist()) == set(range(R + 1))  # every count, so the bound R/2 + 1 and one past it where R allows
    assert noexec and empty and failed
    _, _, _, fl, _, _, _, re, _ = case.arrays
    ctl = np.repeat((fl & C.ORIG_OK) == 0, R).reshape(-1, R) & (re.reshape(-1, R) != 0)
    assert set(ctl.sum(1).tolist()) == set(range(R + 1))  # failed runs of a failed original: used
    # apart from the last item (no run holds its elements) the item lives iff skipped <= R/2 + 1
    np.testing.assert_array_equal(case.keep[:-1], k[:-1] <= R // 2 + 1)
    if R >= 3:
        assert case.keep[:-1][k[:-1] == R // 2 + 1].all() and not case.keep[:-1][k[:-1] == R // 2 + 2].any()


def test_prio_grid_types():
    case = C.prio_grid()
    _, _, pr, fl, _, _, rp, _, _ = case.arrays
    assert pr.dtype == np.int8 and rp.dtype == np.uint8
    assert set(pr.tolist()) == {-128, -1, 0, 1, 127} and set(rp.tolist()) == {0, 1, 127, 128, 255}
    pairs = {(int(a), int(b), int(f)) for a, b, f in zip(pr, rp, fl)}
    assert len(pairs) == 50 == fl.size and set(fl.tolist()) == {0, C.MINIMIZED}
    # a byte of 128 or more must decide differently read signed and unsigned
    signed = rp.view(np.int8).astype(int) >= pr.astype(int)
    assert (signed != (rp.astype(int) >= pr.astype(int))).any()
    np.testing.assert_array_equal(case.elem_keep, signed)


def test_sizes_straddle_the_block():
    case = C.sizes()
    io, el, _, _, ro, rs, _, _, _ = case.arrays
    items, runs = np.diff(io.astype(np.int64)), np.diff(ro.astype(np.int64))
    assert {1, 255, 256, 257, 1000} == set(items.tolist())
    assert {1, 255, 256, 257, 5000} == set(runs.tolist())
    assert (items < C.BLOCK).any() and (items > C.BLOCK).any() and (runs < C.BLOCK).any() and (runs > C.BLOCK).any()
    assert 0 in el and 0xFFFFFFFF in el and 0 in rs and 0xFFFFFFFF in rs
    # raw signals carry duplicates
    assert any(np.unique(rs[a:b]).size < b - a for a, b in zip(ro[:-1].astype(int), ro[1:].astype(int)))
    # 0xFFFFFFFF both survives (index 999) and dies (index 256)
    assert {int(k) for e, k in zip(el, case.elem_keep) if e == 0xFFFFFFFF} == {0, 1}


def test_many_passes_the_block_cap():
    case = C.many()
    io, _, _, _, ro, _, _, _, _ = case.arrays
    n = io.size - 1
    assert n > C.GRID_CAP and ro.size - 1 > C.GRID_CAP and case.runs == 2
    items = np.diff(io.astype(np.int64))
    assert items.min() == 1 and items.max() == 3
    # the item a block of a capped grid serves second never has the outcome of its first
    i = np.arange(C.GRID_CAP, n)
    first = io[i].astype(np.int64)
    assert ((case.keep[i] != case.keep[i - C.GRID_CAP]) | (case.pred[i] != case.pred[i - C.GRID_CAP]) |
            (case.elem_keep[first] != case.elem_keep[io[i - C.GRID_CAP].astype(np.int64)])).all()


def test_chains_separates_chained_from_per_attempt():
    """The minimized item emptied by run 0 whose run 2 holds everything: kept, no
    element kept, predicate true; and an unminimized twin that is dropped."""
    case = C.chains()
    io, el, _, fl, _, _, _, _, _ = case.arrays
    hit = [i for i in range(fl.size) if fl[i] & C.MINIMIZED and case.keep[i] and io[i + 1] > io[i] and
           not case.elem_keep[int(io[i]):int(io[i + 1])].any() and case.pred[i]]
    assert len(hit) == 1
    i = hit[0]
    twin = i + 1
    np.testing.assert_array_equal(el[int(io[i]):int(io[i + 1])], el[int(io[twin]):int(io[twin + 1])])
    assert fl[twin] == 0 and not case.keep[twin] and case.pred[twin]
    assert case.runs == 3
