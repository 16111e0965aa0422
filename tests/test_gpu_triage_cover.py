"""GPU: syzsig_triage_cover_dev -- triageInput's inputCover (syz-fuzzer/
proc.go:139 inputCover.Merge(inf.Cover) over the re-runs, :173 Cover:
inputCover.Serialize()) per item -- against the loop written out in
tests/cover_ref.py, with the runs' cover lists taken from an edge_cover
output and from executor output regions through the ingest."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from syzkaller_amd import _lib
from syzkaller_amd import signal as S
from tests import cover_ref as CR

pytestmark = pytest.mark.gpu

T = _lib.SYZSIG_COVER_TILE
HI = np.uint64(0xffffffff00000000)


def _t(gpu, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)


def _cat(xs, dt):
    return np.concatenate(xs).astype(dt) if xs else np.empty(0, dt)


@functools.lru_cache(maxsize=None)
def _items(nitems, runs, seed, big):
    """Seeded items: skip causes, dropped items and minimized flags as in
    test_gpu_triage_runs; every run has a KCOV trace (one call) drawn from its
    item's pool of PCs, so the runs' cover lists overlap heavily.  Item `big`
    (if >= 0) is kept and has runs of 40000 distinct PCs each.  The reference
    result is computed once here."""
    rng = np.random.default_rng(seed)
    item_off, elems, flags = [0], [], []
    run_sigs, run_prio, run_errno, run_exec, traces = [], [], [], [], []
    for i in range(nitems):
        e = np.unique(rng.integers(0, 5000, int(rng.integers(1, 60))).astype(np.uint32) + np.uint32(i * 10000))
        if i % 13 == 5:
            e = e[:0]  # nothing new: proc.go:109-111
        elems.append(e)
        item_off.append(item_off[-1] + e.size)
        flags.append(1 if i == big else int(rng.integers(0, 4)))
        # pool sizes: most items stay below the tile, every seventh goes past it
        pool = 0x81000000 + i * 0x20000 + 5 * np.arange(60000 if i == big else 3000 if i % 7 == 3 else 200, dtype=np.uint64)
        for r in range(runs):
            if i == big:
                sig, ex, err = e.copy(), 1, 0
                tr = rng.permutation(pool)[:40000]
            else:
                keep_frac = rng.choice([1.0, 1.0, 0.9, 0.0])
                sig = e[rng.random(e.size) < keep_frac]
                sig = np.concatenate([sig, rng.integers(0, 99, 5).astype(np.uint32)]) if rng.random() < 0.9 else sig[:0]
                ex, err = int(rng.random() < 0.9), int(rng.choice([0, 0, 0, 22]))
                tr = rng.choice(pool, int(rng.integers(0, 2 * pool.size)))
            run_sigs.append(sig)
            run_prio.append(int(rng.integers(0, 4)))
            run_errno.append(err)
            run_exec.append(ex)
            traces.append(HI | tr.astype(np.uint64))
    d = dict(item_off=np.array(item_off, np.uint64), elems=_cat(elems, np.uint32),
             flags=np.array(flags, np.uint8), runs=runs,
             run_off=np.cumsum([0] + [s.size for s in run_sigs]).astype(np.uint64), run_sigs=_cat(run_sigs, np.uint32),
             run_prio=np.array(run_prio, np.uint8), run_errno=np.array(run_errno, np.int32),
             run_exec=np.array(run_exec, np.uint8), traces=traces)
    d["prios"] = np.zeros(d["elems"].size, np.int8)
    d["run_cover"] = [CR.call_cover(t) for t in traces]
    d["keep"], d["covers"] = CR.triage_cover(d["item_off"], d["elems"], d["prios"], d["flags"], runs, d["run_off"],
                                             d["run_sigs"], d["run_prio"], d["run_errno"], d["run_exec"],
                                             d["run_cover"])
    return d


def _triage_runs(gpu, d):
    dev = dict(flags=_t(gpu, d["flags"], np.uint8), run_off=_t(gpu, d["run_off"], np.int64),
               run_errno=_t(gpu, d["run_errno"], np.int32), run_exec=_t(gpu, d["run_exec"], np.uint8))
    dev["keep"], _ = gpu.triage_runs(_t(gpu, d["item_off"], np.int64), _t(gpu, d["elems"], np.int32),
                                     _t(gpu, d["prios"], np.int8), dev["flags"], d["runs"], dev["run_off"],
                                     _t(gpu, d["run_sigs"], np.int32), _t(gpu, d["run_prio"], np.uint8),
                                     dev["run_errno"], dev["run_exec"])
    np.testing.assert_array_equal(dev["keep"].cpu().numpy(), d["keep"])
    return dev


def _cover_from_edge(gpu, d):
    """The runs' cover lists as ranges into an edge_cover output: run r is
    call r, an item's runs are one program."""
    lens = np.array([t.size for t in d["traces"]], np.uint32)
    starts = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    pcs = np.concatenate(d["traces"])
    pidx = (np.arange(len(lens) // d["runs"] + 1) * d["runs"]).astype(np.uint32)
    a = [_t(gpu, pcs, np.int64), _t(gpu, starts, np.int64), _t(gpu, lens, np.int32), _t(gpu, pidx, np.int32)]
    _, _, comp = gpu.edge_derive(*a)
    cover, cnt = gpu.edge_cover(*a, comp)
    return cover, a[1], cnt


def _cover_from_regions(gpu, d):
    """... and as ranges into executor output regions (executor.h:566-604
    records: index, num, errno, fault, nsig, ncover, ncomps, sig[], cover[])
    through the ingest's cover_start / cover_len: one region per run, holding
    the run's call with its signal and its cover list."""
    a, words, off = d["run_off"], [], [0]
    for r, cov in enumerate(d["run_cover"]):
        sig = d["run_sigs"][int(a[r]):int(a[r + 1])]
        w = np.concatenate([np.array([1, 0, 0, d["run_errno"][r], 0, sig.size, cov.size, 0], np.int64)
                            .astype(np.uint32), sig, cov]) if d["run_exec"][r] else np.zeros(1, np.uint32)
        words.append(w)
        off.append(off[-1] + w.size)
    nruns = len(words)
    out = _t(gpu, np.concatenate(words), np.int32)
    ing = gpu.ingest_exec_output(out, _t(gpu, np.array(off, np.uint64), np.int64),
                                 _t(gpu, np.arange(nruns + 1, dtype=np.uint32), np.int32),
                                 torch.zeros(nruns, dtype=torch.uint8, device=gpu.dev), want_cover=True)
    assert ing["n_failed"] == 0
    return out, ing["cover_start"], ing["cover_len"]


def _check(d, off, cover):
    eoff = np.concatenate([[0], np.cumsum([c.size for c in d["covers"]])]).astype(np.int64)
    np.testing.assert_array_equal(off.cpu().numpy(), eoff)
    np.testing.assert_array_equal(cover.cpu().numpy().view(np.uint32), _cat(d["covers"], np.uint32))


@pytest.mark.parametrize("nitems,runs,seed,big", [(300, 3, 1, -1), (50, 8, 2, 7)])
@pytest.mark.parametrize("source", ["edge_cover", "regions"])
def test_triage_cover_vs_restatement(gpu, nitems, runs, seed, big, source):
    d = _items(nitems, runs, seed, big)
    tot = np.array([sum(d["run_cover"][i * runs + k].size for k in range(runs)) for i in range(nitems)])
    assert (tot[d["keep"] == 1] > T).any() and ((tot > 0) & (tot < T))[d["keep"] == 1].any()
    assert 0 < d["keep"].sum() < nitems
    if big >= 0:
        assert d["keep"][big] and tot[big] == 8 * 40000
    dev = _triage_runs(gpu, d)
    cov = (_cover_from_edge if source == "edge_cover" else _cover_from_regions)(gpu, d)
    off, cover = gpu.triage_cover(dev["flags"], dev["keep"], runs, dev["run_off"], dev["run_errno"], dev["run_exec"],
                                  *cov)
    _check(d, off, cover)


def test_triage_cover_capacity(gpu):
    d = _items(300, 3, 1, -1)
    dev = _triage_runs(gpu, d)
    cov, cs, cl = _cover_from_edge(gpu, d)
    total = sum(c.size for c in d["covers"])

    def call(cap):
        off = torch.full((301,), -7, dtype=torch.int64, device=gpu.dev)
        out = torch.full((total,), 0x12345678, dtype=torch.int32, device=gpu.dev)
        n = ctypes.c_uint64()
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        rc = gpu.L.syzsig_triage_cover_dev(gpu.eng.h, 300, 3, p(dev["flags"]), p(dev["keep"]), p(dev["run_off"]),
                                           p(dev["run_errno"]), p(dev["run_exec"]), p(cov), cov.numel(), p(cs), p(cl),
                                           p(off), p(out), cap, ctypes.byref(n))
        torch.cuda.synchronize()
        return rc, n.value, off, out

    rc, n, off, out = call(total - 1)
    assert rc == _lib.SYZSIG_ERANGE and n == total
    assert bool((off == -7).all()) and bool((out == 0x12345678).all())  # nothing committed
    rc, n, off, out = call(total)
    assert rc == _lib.SYZSIG_OK and n == total
    _check(d, off, out)


def test_traces_to_corpus_cover_end_to_end(gpu):
    """traces -> edge_derive + edge_cover -> triage_runs -> triage_cover ->
    every kept item's slice merged into a Cover (manager.go:998), against the
    Python set union over the reference's run of the same loop."""
    rng = np.random.default_rng(9)
    nitems, runs = 40, 3
    traces = []
    for i in range(nitems):
        base = HI | (0x81000000 + i * 0x800 + 5 * rng.integers(0, 400, int(rng.integers(20, 6000))).astype(np.uint64))
        for r in range(runs):
            tr = base[: int(base.size * rng.uniform(0.5, 1.0))].copy()
            if rng.random() < 0.15:
                tr[int(rng.integers(0, tr.size))] = 0x2000  # fails cover_check: no record, the run is skipped
            traces.append(tr)
    lens = np.array([t.size for t in traces], np.uint32)
    starts = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    pcs = np.concatenate(traces)
    pidx = np.arange(nitems * runs + 1, dtype=np.uint32)  # every run is an execution of its own
    a = [_t(gpu, pcs, np.int64), _t(gpu, starts, np.int64), _t(gpu, lens, np.int32), _t(gpu, pidx, np.int32)]
    sigs, sig_cnt, comp = gpu.edge_derive(*a)
    cover, cover_cnt = gpu.edge_cover(*a, comp)
    # the items: newSignal = the first run's signal (or the second's), prio 0
    hs, hc = sigs.cpu().numpy().view(np.uint32), sig_cnt.cpu().numpy().view(np.uint32)
    run_sigs = [hs[int(starts[r]):int(starts[r]) + int(hc[r])] for r in range(nitems * runs)]
    elems = [np.unique(run_sigs[i * runs] if run_sigs[i * runs].size else run_sigs[i * runs + 1]) for i in range(nitems)]
    item_off = np.cumsum([0] + [e.size for e in elems]).astype(np.uint64)
    elems = _cat(elems, np.uint32)
    prios = np.zeros(elems.size, np.int8)
    flags = rng.integers(0, 4, nitems).astype(np.uint8)
    run_off = np.cumsum([0] + [s.size for s in run_sigs]).astype(np.uint64)
    run_prio = np.full(nitems * runs, 3, np.uint8)
    run_errno = np.zeros(nitems * runs, np.int32)
    run_exec = np.ones(nitems * runs, np.uint8)
    keep, _, slices = gpu.triage_runs(_t(gpu, item_off, np.int64), _t(gpu, elems, np.int32), _t(gpu, prios, np.int8),
                                      _t(gpu, flags, np.uint8), runs, _t(gpu, run_off, np.int64),
                                      _t(gpu, _cat(run_sigs, np.uint32), np.int32), _t(gpu, run_prio, np.uint8),
                                      _t(gpu, run_errno, np.int32), _t(gpu, run_exec, np.uint8),
                                      cover=(cover, a[1], cover_cnt))
    corpus_cover = S.Cover(gpu.eng)
    for s in slices:
        if s is not None:
            corpus_cover.merge_dev(s)
    # the reference side, from the oracle's executor and the restated loop
    osigs, ocnt, ocomp = O.exec_batch(pcs, starts, lens, pidx)
    np.testing.assert_array_equal(comp.cpu().numpy().view(np.uint32), ocomp)
    ecover, ecnt = CR.edge_cover(pcs, starts, lens, pidx, ocomp)
    orun = [osigs[int(starts[r]):int(starts[r]) + int(ocnt[r])] for r in range(nitems * runs)]
    ekeep, ecovers = CR.triage_cover(item_off, elems, prios, flags, runs, run_off, _cat(orun, np.uint32), run_prio,
                                     run_errno, run_exec,
                                     [ecover[int(starts[r]):int(starts[r]) + int(ecnt[r])] for r in range(nitems * runs)])
    np.testing.assert_array_equal(keep.cpu().numpy(), ekeep)
    assert [s is not None for s in slices] == [bool(k) for k in ekeep] and 0 < ekeep.sum()
    union = set()
    for k, c in zip(ekeep, ecovers):
        if k:
            union.update(c.tolist())
    assert len(union) > 0 and ocomp.min() == 0
    assert sorted(corpus_cover.Serialize().tolist()) == sorted(union)
