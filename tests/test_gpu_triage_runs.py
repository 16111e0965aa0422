"""GPU: triageInput's signal re-runs (syz-fuzzer/proc.go:107-140) over a batch
of triage items, against the restatement built from the oracle's Signal ops
(Deserialize / FromRaw / Intersection), covering skipped runs (not executed,
empty signal, failed after success), the give-up rule, minimized items and
prio ordering (Intersection keeps e only when the run's prio >= e's prio).

The second half runs the batches of tests/triage_runs_cases.py, built for
csrc/stable.hip (block-stride loops, the 8192-block cap, the int8 prio byte,
the give-up bound, chained against per-attempt Intersections, run keys,
workspace reuse), against the oracle and against the outcome derived by hand."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from syzkaller_amd import _lib
from syzkaller_amd.device import _p
from tests import triage_runs_cases as C

pytestmark = pytest.mark.gpu


def make_items(rng, nitems, runs):
    item_off, elems, prios, flags = [0], [], [], []
    run_off, run_sigs, run_prio, run_errno, run_exec = [0], [], [], [], []
    for i in range(nitems):
        n = int(rng.integers(0, 120)) if i % 11 else 0
        e = np.unique(rng.integers(0, 5000, n).astype(np.uint32) + np.uint32(i * 10000))
        elems.append(e)
        prios.append(rng.integers(-1, 4, e.size).astype(np.int8))
        item_off.append(item_off[-1] + e.size)
        flags.append(int(rng.integers(0, 4)))
        for r in range(runs):
            keep_frac = rng.choice([1.0, 0.97, 0.6, 0.0])
            sig = e[rng.random(e.size) < keep_frac]
            noise = rng.integers(0, 5000, int(rng.integers(0, 50))).astype(np.uint32) + np.uint32(i * 10000)
            sig = np.concatenate([sig, noise]) if rng.random() < 0.9 else np.empty(0, np.uint32)
            rng.shuffle(sig)
            run_sigs.append(sig)
            run_off.append(run_off[-1] + sig.size)
            run_prio.append(int(rng.integers(0, 4)))
            run_errno.append(int(rng.choice([0, 0, 0, 22])))
            run_exec.append(int(rng.random() < 0.9))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.empty(0, dt)  # noqa: E731
    return (np.array(item_off, np.uint64), cat(elems, np.uint32), cat(prios, np.int8), np.array(flags, np.uint8),
            np.array(run_off, np.uint64), cat(run_sigs, np.uint32), np.array(run_prio, np.uint8),
            np.array(run_errno, np.int32), np.array(run_exec, np.uint8))


def _t(gpu, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)


@pytest.mark.parametrize("runs,seed", [(3, 1), (3, 2), (1, 3), (5, 4), (0, 5), (8, 6)])
def test_triage_runs_vs_restatement(gpu, runs, seed):
    rng = np.random.default_rng(seed)
    io, el, pr, fl, ro, rs, rp, re, rx = make_items(rng, 400, runs)
    ik, ek = gpu.triage_runs(_t(gpu, io, np.int64), _t(gpu, el, np.int32), _t(gpu, pr, np.int8),
                             _t(gpu, fl, np.uint8), runs, _t(gpu, ro, np.int64), _t(gpu, rs, np.int32),
                             _t(gpu, rp, np.uint8), _t(gpu, re, np.int32), _t(gpu, rx, np.uint8))
    okeep, finals = O.triage_runs(io, el, pr, fl, runs, ro, rs, rp, re, rx)
    ik, ek = ik.cpu().numpy(), ek.cpu().numpy()
    np.testing.assert_array_equal(ik, okeep)
    assert 0 < okeep.sum() < okeep.size or runs == 0
    for i in range(io.size - 1):
        a, b = int(io[i]), int(io[i + 1])
        got = {int(e): int(p) for e, p, k in zip(el[a:b], pr[a:b], ek[a:b]) if k}
        assert got == (finals[i] or {}), i


def test_triage_runs_empty_batch(gpu):
    z64 = torch.zeros(1, dtype=torch.int64, device=gpu.dev)
    e = torch.empty(0, dtype=torch.int32, device=gpu.dev)
    u8 = torch.empty(0, dtype=torch.uint8, device=gpu.dev)
    ik, ek = gpu.triage_runs(z64, e, u8.view(torch.int8), u8, 3, z64, e, u8, e, u8)
    assert ik.numel() == 0 and ek.numel() == 0


@pytest.mark.parametrize("attempts,seed", [(3, 11), (1, 12), (4, 13), (8, 14)])
def test_minimize_pred_vs_restatement(gpu, attempts, seed):
    rng = np.random.default_rng(seed)
    io, el, pr, fl, ro, rs, rp, re, rx = make_items(rng, 400, attempts)
    pred = gpu.minimize_pred(_t(gpu, io, np.int64), _t(gpu, el, np.int32), _t(gpu, pr, np.int8),
                             _t(gpu, fl, np.uint8), attempts, _t(gpu, ro, np.int64), _t(gpu, rs, np.int32),
                             _t(gpu, rp, np.uint8), _t(gpu, re, np.int32), _t(gpu, rx, np.uint8))
    exp = O.minimize_pred(io, el, pr, fl, attempts, ro, rs, rp, re, rx)
    np.testing.assert_array_equal(pred.cpu().numpy(), exp)
    assert 0 < exp.sum() < exp.size


# ---- batches built for stable.hip (tests/triage_runs_cases.py) ----
CASES = dict(C.all_cases() + [("no_runs", C.no_runs)])
DIRECTED = [n for n, _ in C.all_cases()]
DTYPES = (np.int64, np.int32, np.int8, np.uint8, np.int64, np.int32, np.uint8, np.int32, np.uint8)
FILL = 0xAA


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """(item_keep, elem_keep, pred) of a batch by the oracle's Signal ops, computed once"""
    case = CASES[name]()
    io, el, pr = case.arrays[:3]
    keep, finals = O.triage_runs(*case.arrays[:4], case.runs, *case.arrays[4:])
    ek = np.zeros(el.size, np.uint8)
    for i, f in enumerate(finals):
        a, b = int(io[i]), int(io[i + 1])
        ek[a:b] = [(f or {}).get(int(e)) == int(p) for e, p in zip(el[a:b], pr[a:b])]
        assert int(ek[a:b].sum()) == len(f or {}), i
    pred = O.minimize_pred(*case.arrays[:4], case.runs, *case.arrays[4:])
    for a in (keep, ek, pred):
        a.setflags(write=False)
    return keep, ek, pred


def dev_arrays(gpu, arrays):
    return [torch.from_numpy(a.view(dt).copy()).to(gpu.dev) for a, dt in zip(arrays, DTYPES)]


def filled(gpu, n):
    return torch.full((n,), FILL, dtype=torch.uint8, device=gpu.dev)


def raw_triage_runs(gpu, d, runs):
    """syzsig_triage_runs_dev on outputs pre-filled with 0xAA -> (rc, item_keep, elem_keep)"""
    io, el, pr, fl, ro, rs, rp, re, rx = d
    ik, ek = filled(gpu, io.numel() - 1), filled(gpu, el.numel())
    rc = gpu.L.syzsig_triage_runs_dev(gpu.eng.h, _p(io), io.numel() - 1, _p(el), _p(pr), _p(fl), runs, _p(ro),
                                      _p(rs), _p(rp), _p(re), _p(rx), _p(ik), _p(ek))
    return rc, ik.cpu().numpy(), ek.cpu().numpy()


def raw_minimize_pred(gpu, d, attempts):
    io, el, pr, fl, ro, rs, rp, re, rx = d
    pred = filled(gpu, io.numel() - 1)
    rc = gpu.L.syzsig_minimize_pred_dev(gpu.eng.h, _p(io), io.numel() - 1, _p(el), _p(pr), _p(fl), attempts,
                                        _p(ro), _p(rs), _p(rp), _p(re), _p(rx), _p(pred))
    return rc, pred.cpu().numpy()


def check_triage_runs(gpu, name):
    case = CASES[name]()
    okeep, oek, _ = oracle_of(name)
    d = dev_arrays(gpu, case.arrays)
    rc, ik, ek = raw_triage_runs(gpu, d, case.runs)
    assert rc == _lib.SYZSIG_OK
    assert np.isin(ik, (0, 1)).all() and np.isin(ek, (0, 1)).all()  # no byte left unwritten
    wik, wek = gpu.triage_runs(*d[:4], case.runs, *d[4:])
    for got_k, got_e in ((ik, ek), (wik.cpu().numpy(), wek.cpu().numpy())):
        np.testing.assert_array_equal(got_k, okeep)
        np.testing.assert_array_equal(got_k, case.keep)
        np.testing.assert_array_equal(got_e, oek)
        np.testing.assert_array_equal(got_e, case.elem_keep)


def check_minimize_pred(gpu, name):
    case = CASES[name]()
    _, _, opred = oracle_of(name)
    d = dev_arrays(gpu, case.arrays)
    rc, pred = raw_minimize_pred(gpu, d, case.runs)
    assert rc == _lib.SYZSIG_OK
    assert np.isin(pred, (0, 1)).all()
    wpred = gpu.minimize_pred(*d[:4], case.runs, *d[4:]).cpu().numpy()
    for got in (pred, wpred):
        np.testing.assert_array_equal(got, opred)
        np.testing.assert_array_equal(got, case.pred)


@pytest.mark.parametrize("name", DIRECTED)
def test_triage_runs_directed(gpu, name):
    check_triage_runs(gpu, name)


@pytest.mark.parametrize("name", DIRECTED)
def test_minimize_pred_directed(gpu, name):
    check_minimize_pred(gpu, name)


def test_small_batch_after_large_on_one_engine(gpu):
    """sizes() (the largest set and alive array), then chains(), then a batch
    without runs, on one context: the workspace slots are reused, so stale set
    contents, alive bits or alive counts of the larger call would show."""
    for name in ("sizes", "chains", "no_runs"):
        check_triage_runs(gpu, name)
        check_minimize_pred(gpu, name)


def test_no_attempts_is_no(gpu):
    for name in ("no_runs", "chains"):
        case = CASES[name]()
        io, el, pr, fl = case.arrays[:4]
        none = (np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.uint8), np.empty(0, np.int32),
                np.empty(0, np.uint8))
        rc, pred = raw_minimize_pred(gpu, dev_arrays(gpu, (io, el, pr, fl) + none), 0)
        assert rc == _lib.SYZSIG_OK
        np.testing.assert_array_equal(pred, np.zeros(fl.size, np.uint8))  # proc.go:161
        np.testing.assert_array_equal(pred, O.minimize_pred(io, el, pr, fl, 0, *none))


def test_more_than_eight_runs_is_erange(gpu):
    """runs / attempts = 9 on a well-formed nine-run batch: SYZSIG_ERANGE, outputs untouched."""
    over = C.MAX_RUNS + 1
    arrays = make_items(np.random.default_rng(9), 20, over)
    d = dev_arrays(gpu, arrays)
    rc, ik, ek = raw_triage_runs(gpu, d, over)
    assert rc == _lib.SYZSIG_ERANGE
    assert ik.size == 20 and ek.size > 0 and (ik == FILL).all() and (ek == FILL).all()
    rc, pred = raw_minimize_pred(gpu, d, over)
    assert rc == _lib.SYZSIG_ERANGE
    assert (pred == FILL).all()
    with pytest.raises(_lib.SyzsigError) as e:
        gpu.triage_runs(*d[:4], over, *d[4:])
    assert e.value.code == _lib.SYZSIG_ERANGE
    with pytest.raises(_lib.SyzsigError) as e:
        gpu.minimize_pred(*d[:4], over, *d[4:])
    assert e.value.code == _lib.SYZSIG_ERANGE
