"""GPU: syzsig_triage_items_dev (proc.go:232-245, :107-111 over a batch) and
syzsig_corpus_add_inputs_dev (fuzzer.go:446-460), word for word against the
loops written out in tests/triage_items_ref.py.  Every output buffer is
pre-filled and compared whole, so a stray write shows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from syzkaller_amd import _lib, synth
from syzkaller_amd import signal as S
from tests import table_keys as TK
from tests import triage_items_ref as R

pytestmark = pytest.mark.gpu

T = _lib.SYZSIG_ITEMS_TILE
FILL32, FILL8, FILLOFF = 0x12345678, 0x5a, -7
GAP = 3  # unused records in front of every call
OUT = [("item_call", "i", torch.int32, FILL32), ("item_prio", "i", torch.int8, FILL8),
       ("input_off", "o", torch.int64, FILLOFF), ("input_elems", "n", torch.int32, FILL32),
       ("item_off", "o", torch.int64, FILLOFF), ("elems", "w", torch.int32, FILL32), ("prios", "w", torch.int8, FILL8)]


def _t(gpu, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)


def _layout(calls):
    """calls = [(records u32[], prio, call_new value), ...] -> the batch's host
    arrays, GAP unused records in front of every call"""
    lens = np.array([len(r) for r, _, _ in calls], np.uint32)
    start = (np.cumsum(lens.astype(np.uint64) + GAP) - lens).astype(np.uint64)
    sigs = np.full(int(start[-1] + lens[-1]) if len(calls) else 0, 0xdeadbeef, np.uint32)
    for (r, _, _), s, n in zip(calls, start, lens):
        sigs[int(s):int(s) + int(n)] = r
    return {"sigs": sigs, "start": start, "len": lens, "prio": np.array([p for _, p, _ in calls], np.uint8),
            "new": np.array([f for _, _, f in calls], np.uint8)}


def _dev(gpu, b):
    return [_t(gpu, b["sigs"], np.int32), _t(gpu, b["start"], np.int64), _t(gpu, b["len"], np.int32),
            _t(gpu, b["prio"], np.uint8), _t(gpu, b["new"], np.uint8)]


def _ref(b, corpus):
    """the restatement's result for batch b against corpus = (elems, prios) or None (nil)"""
    oc = O.deserialize(*corpus) if corpus is not None else O.OSig()
    return R.triage_items(oc, b["sigs"], b["start"], b["len"], b["prio"], b["new"])


def _raw(gpu, d, corpus, caps, nrec=None):
    """syzsig_triage_items_dev into pre-filled buffers of the given capacities"""
    cap = {"i": caps[0], "o": caps[0] + 1, "n": caps[1], "w": caps[2]}
    out = {k: torch.full((cap[c],), fill, dtype=dt, device=gpu.dev) for k, c, dt, fill in OUT}
    n = [ctypes.c_uint64(99), ctypes.c_uint64(99), ctypes.c_uint64(99)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = gpu.L.syzsig_triage_items_dev(
        gpu.eng.h, p(d[0]), d[0].numel() if nrec is None else nrec, p(d[1]), p(d[2]), p(d[3]), d[2].numel(), p(d[4]),
        corpus.handle if corpus is not None else ctypes.c_void_p(0), p(out["item_call"]), p(out["item_prio"]), caps[0],
        p(out["input_off"]), p(out["input_elems"]), caps[1], p(out["item_off"]), p(out["elems"]), p(out["prios"]),
        caps[2], ctypes.byref(n[0]), ctypes.byref(n[1]), ctypes.byref(n[2]))
    torch.cuda.synchronize()
    return rc, tuple(int(x.value) for x in n), out


def _signed(r):
    """a reference array in the dtype its device tensor has"""
    return r.view({8: np.int64, 4: np.int32, 1: np.int8}[r.itemsize])


def _totals(ref):
    return (ref["item_call"].size, ref["input_elems"].size, ref["elems"].size)


def _assert_untouched(out):
    for k, _, _, fill in OUT:
        assert bool((out[k] == fill).all()), k


def _assert_exact(out, ref):
    """every buffer whole: the reference's words, then the fill"""
    for k, _, dt, fill in OUT:
        got = out[k].cpu().numpy()
        exp = np.full(got.size, fill, got.dtype)
        exp[:ref[k].size] = _signed(ref[k])
        np.testing.assert_array_equal(got, exp, err_msg=k)


def _check(gpu, b, corpus=None, slack=5):
    """device call with `slack` spare entries in every buffer against the restatement"""
    ref = _ref(b, corpus)
    dc = S.Serial(*corpus).Deserialize(gpu.eng) if corpus is not None else None
    tot = _totals(ref)
    rc, n, out = _raw(gpu, _dev(gpu, b), dc, tuple(x + slack for x in tot))
    assert rc == _lib.SYZSIG_OK, gpu.L.syzsig_last_error()
    assert n == tot
    _assert_exact(out, ref)
    return ref, gpu.triage_items_stats()


@functools.lru_cache(maxsize=None)
def _length_classes():
    rng = np.random.default_rng(11)
    pool = rng.integers(0, 2 ** 32, 3000, dtype=np.uint64).astype(np.uint32)  # draws repeat: duplicates in a call
    calls = []
    for n in (0, 1, 2, T - 1, T, T + 1, 2 * T + 3, 262143):
        calls.append((rng.choice(pool, n) if n != 262143 else rng.integers(0, 200000, n).astype(np.uint32),
                      int(rng.integers(0, 4)), 1))
        calls.append((rng.choice(pool, int(rng.integers(0, 50))), 3, 0))  # unflagged, between
    calls.append((np.full(777, 0xabcdef01, np.uint32), 2, 1))  # all equal
    calls.append((np.arange(5, 5 + T + 5, dtype=np.uint32), 1, 1))  # ascending, past the tile
    calls.append((np.arange(900, 0, -1, dtype=np.uint32) * 3, 0, 1))  # descending
    calls.append((rng.permutation(np.arange(1 << 20, (1 << 20) + T, dtype=np.uint32)), 3, 1))  # all distinct, one tile
    b = _layout(calls)
    # corpusSignal: a part of the pool and of the small ranges, prios around the calls'
    ce = np.unique(np.concatenate([pool[::2], np.arange(0, 200000, 3, dtype=np.uint32), [0xabcdef01]]).astype(np.uint32))
    cp = rng.integers(-1, 4, ce.size).astype(np.int8)
    return b, (ce, cp)


def test_length_classes(gpu):
    b, corpus = _length_classes()
    ref, st = _check(gpu, b, corpus)
    flagged = b["len"][b["new"] != 0]
    assert ref["item_call"].size == flagged.size == 12
    assert 0 < ref["elems"].size < ref["input_elems"].size < int(flagged.sum())  # duplicates and known elements exist
    nlong = int((flagged > T).sum())
    # both paths ran: calls of at most one tile and longer ones; 262143 records = 64 tiles: 6 doublings
    assert st == (12, nlong, 6, ref["input_elems"].size) and nlong == 4 and 12 - nlong > 0


def test_length_classes_nil_corpus(gpu):
    b, _ = _length_classes()
    ref, st = _check(gpu, b, None)
    np.testing.assert_array_equal(ref["elems"], ref["input_elems"])  # Diff against nil: everything
    assert st[3] == 0


def _small_calls(rng, ncalls, flags):
    lens = rng.integers(1, 4, ncalls)
    return _layout([(rng.integers(0, 5000, int(n)).astype(np.uint32), int(rng.integers(0, 4)), int(f))
                    for n, f in zip(lens, flags)])


@pytest.mark.parametrize("case", ["none", "all", "sparse_past_one_workgroup", "other_values"])
def test_item_list(gpu, case):
    rng = np.random.default_rng(5)
    if case == "none":
        b = _small_calls(rng, 600, np.zeros(600, np.uint8))
    elif case == "all":
        b = _small_calls(rng, 600, np.ones(600, np.uint8))
    elif case == "sparse_past_one_workgroup":
        flags = np.zeros(70000, np.uint8)
        flags[rng.choice(70000, 3000, replace=False)] = 1
        b = _small_calls(rng, 70000, flags)
    else:
        flags = rng.choice(np.array([0, 0, 1, 2, 0x80, 0xff], np.uint8), 2000)
        b = _small_calls(rng, 2000, flags)
    ce = np.arange(0, 5000, 2, dtype=np.uint32)
    ref, st = _check(gpu, b, (ce, rng.integers(0, 4, ce.size).astype(np.int8)))
    assert ref["item_call"].size == int((b["new"] != 0).sum()) and st[0] == ref["item_call"].size and st[1] == 0
    np.testing.assert_array_equal(ref["item_call"], np.flatnonzero(b["new"]))
    if case == "none":
        assert ref["input_off"].tolist() == [0] and ref["item_off"].tolist() == [0]


def test_no_calls(gpu):
    b = {"sigs": np.empty(0, np.uint32), "start": np.empty(0, np.uint64), "len": np.empty(0, np.uint32),
         "prio": np.empty(0, np.uint8), "new": np.empty(0, np.uint8)}
    rc, n, out = _raw(gpu, _dev(gpu, b), None, (2, 2, 2))
    assert rc == _lib.SYZSIG_OK and n == (0, 0, 0)
    assert out["input_off"].tolist() == [0, FILLOFF, FILLOFF] and out["item_off"].tolist() == [0, FILLOFF, FILLOFF]


def test_corpus_probes_on_chosen_keys(gpu):
    """A cluster of 40 corpus elements on the table's last bucket (two slots a
    bucket: it wraps the table's end), present below, at and above the item's
    prio; 20 more elements of that bucket that are absent, behind the whole
    chain; uniform elements beside them."""
    rng = np.random.default_rng(3)
    cluster, absent = TK.hot_last(40), TK.hot_last(20, skip=40)
    uni = rng.integers(0, 2 ** 32, 300, dtype=np.uint64).astype(np.uint32)
    ce = np.concatenate([cluster, uni[:150]])
    cp = np.concatenate([np.tile(np.array([0, 1, 2], np.int8), 14)[:40], rng.integers(-128, 128, 150).astype(np.int8)])
    dc = S.Serial(ce, cp).Deserialize(gpu.eng)
    nb = dc.capacity() // TK.BUCKET_SLOTS
    assert (TK.home_bucket(np.concatenate([cluster, absent]), nb) == nb - 1).all() and 40 > TK.BUCKET_SLOTS
    rec = np.concatenate([cluster, absent, uni, cluster[::3]])
    b = _layout([(rng.permutation(rec), 1, 1), (rng.permutation(rec), 0x80, 1), (rng.permutation(rec), 3, 1),
                 (rng.permutation(rec), 0, 0)])
    ref, st = _check(gpu, b, (ce, cp))
    new0 = set(ref["elems"][int(ref["item_off"][0]):int(ref["item_off"][1])].tolist())
    assert set(absent.tolist()) <= new0  # absent behind the chain: new
    assert new0 & set(cluster.tolist()) == set(cluster[cp[:40] < 1].tolist())  # present: new only below prio 1
    assert st[3] == ref["input_elems"].size
    _check(gpu, b, None)


def test_capacities(gpu):
    b, corpus = _length_classes()
    ref = _ref(b, corpus)
    tot = _totals(ref)
    d, dc = _dev(gpu, b), S.Serial(*corpus).Deserialize(gpu.eng)
    for short in range(3):
        caps = tuple(x - (i == short) for i, x in enumerate(tot))
        rc, n, out = _raw(gpu, d, dc, caps)
        assert rc == _lib.SYZSIG_ERANGE and n == tot
        _assert_untouched(out)
    rc, n, out = _raw(gpu, d, dc, tot)
    assert rc == _lib.SYZSIG_OK and n == tot
    _assert_exact(out, ref)


def test_grow_and_retry_wrapper(gpu):
    b, corpus = _length_classes()
    ref = _ref(b, corpus)
    dc = S.Serial(*corpus).Deserialize(gpu.eng)
    r = gpu.triage_items(*_dev(gpu, b), corpus_signal=dc)
    for k, _, _, _ in OUT:
        np.testing.assert_array_equal(r[k].cpu().numpy(), _signed(ref[k]), err_msg=k)
    with pytest.raises(_lib.SyzsigError) as e:
        gpu.triage_items(*_dev(gpu, b), corpus_signal=dc, caps=(1, 1, 1))
    assert e.value.code == _lib.SYZSIG_ERANGE and e.value.needed == _totals(ref)


def test_errors(gpu):
    rng = np.random.default_rng(8)
    b = _small_calls(rng, 300, rng.integers(0, 2, 300).astype(np.uint8))
    d = _dev(gpu, b)
    last_end = int(b["start"][-1] + b["len"][-1])
    assert last_end == b["sigs"].size
    # the last call (flagged or not) ends one record past nrec
    rc, n, out = _raw(gpu, d, None, (300, 1000, 1000), nrec=last_end - 1)
    assert rc == _lib.SYZSIG_EINVAL and n == (0, 0, 0)
    _assert_untouched(out)
    # a start beyond the records
    bad = dict(b, start=b["start"].copy())
    bad["start"][7] = b["sigs"].size + 1
    rc, n, out = _raw(gpu, _dev(gpu, bad), None, (300, 1000, 1000))
    assert rc == _lib.SYZSIG_EINVAL
    _assert_untouched(out)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    z = ctypes.c_uint64()
    rc = gpu.L.syzsig_triage_items_dev(gpu.eng.h, p(d[0]), d[0].numel(), p(d[1]), p(d[2]), p(d[3]), 300, p(d[4]), None,
                                       None, None, 0, None, None, 0, None, None, None, 0, ctypes.byref(z),
                                       ctypes.byref(z), ctypes.byref(z))
    assert rc == _lib.SYZSIG_EINVAL  # the offset arrays are required
    _check(gpu, b, None)  # a well-formed call afterwards is exact


# ---------------------------------------------------------------- corpus_add_inputs

@functools.lru_cache(maxsize=None)
def _random_items():
    rng = np.random.default_rng(21)
    elems, prios = [], []
    for i in range(200):
        n = 0 if i % 9 == 4 else int(rng.integers(1, 120))
        elems.append(np.unique(rng.integers(0, 6000, n).astype(np.uint32)))
        prios.append(int(rng.integers(-128, 128)))
    off = np.cumsum([0] + [e.size for e in elems]).astype(np.uint64)
    keep = (rng.random(200) < 0.6).astype(np.uint8) * rng.integers(1, 256, 200).astype(np.uint8)
    ce = np.unique(rng.integers(0, 9000, 100).astype(np.uint32))
    me = np.unique(rng.integers(0, 9000, 4000).astype(np.uint32))
    return {"off": off, "elems": np.concatenate(elems), "prio": np.array(prios, np.int8), "keep": keep,
            "corpus": (ce, rng.integers(-128, 128, ce.size).astype(np.int8)),
            "max": (me, rng.integers(-128, 128, me.size).astype(np.int8))}


def _same(g, o):
    assert g.is_nil() == o.is_nil()
    assert g.Len() == o.Len() and g.to_dict() == o.to_dict()
    assert len(g.Serialize().Elems) == o.Len()


@pytest.mark.parametrize("receivers", ["nil", "sets", "nil_corpus"])
@pytest.mark.parametrize("masked", [True, False])
def test_corpus_add_inputs(gpu, receivers, masked):
    it = _random_items()
    keep = it["keep"] if masked else None
    gc = S.Serial(*it["corpus"]).Deserialize(gpu.eng) if receivers == "sets" else S.Signal(None, gpu.eng)
    gm = S.Serial(*it["max"]).Deserialize(gpu.eng) if receivers != "nil" else S.Signal(None, gpu.eng)
    oc = O.deserialize(*it["corpus"]) if receivers == "sets" else O.OSig()
    om = O.deserialize(*it["max"]) if receivers != "nil" else O.OSig()
    d = [_t(gpu, it["off"], np.int64), _t(gpu, it["elems"], np.int32), _t(gpu, it["prio"], np.int8)]
    dk = _t(gpu, keep, np.uint8) if masked else None
    cap0 = gc.capacity()
    gpu.corpus_add_inputs(*d, gc, gm, item_keep=dk)
    R.add_inputs(oc, om, it["off"], it["elems"], it["prio"], keep)
    _same(gc, oc)
    _same(gm, om)
    assert oc.Len() > 1000 and (receivers != "sets" or gc.capacity() > cap0)  # the small corpus table grew
    # the inputs are unchanged
    np.testing.assert_array_equal(d[0].cpu().numpy().view(np.uint64), it["off"])
    np.testing.assert_array_equal(d[1].cpu().numpy().view(np.uint32), it["elems"])
    np.testing.assert_array_equal(d[2].cpu().numpy(), it["prio"])
    if masked:
        np.testing.assert_array_equal(dk.cpu().numpy(), keep)
    # a second time changes nothing (max-merge is idempotent), not even a slot word
    snap_c, snap_m = gc.clone(), gm.clone()
    gpu.corpus_add_inputs(*d, gc, gm, item_keep=dk)
    assert gc.equal(snap_c) and gm.equal(snap_m)


def test_corpus_add_inputs_nothing_kept_and_errors(gpu):
    it = _random_items()
    d = [_t(gpu, it["off"], np.int64), _t(gpu, it["elems"], np.int32), _t(gpu, it["prio"], np.int8)]
    gc, gm = S.Serial(*it["corpus"]).Deserialize(gpu.eng), S.Signal(None, gpu.eng)
    snap = gc.clone()
    none = torch.zeros(200, dtype=torch.uint8, device=gpu.dev)
    gpu.corpus_add_inputs(*d, gc, gm, item_keep=none)
    assert gc.equal(snap) and gm.is_nil()
    # only items whose sign is empty are kept: fuzzer.go:454 guards the Merge, nil stays nil
    only_empty = torch.zeros(200, dtype=torch.uint8, device=gpu.dev)
    only_empty[4::9] = 1
    gn = S.Signal(None, gpu.eng)
    gpu.corpus_add_inputs(*d, gn, gm, item_keep=only_empty)
    assert gn.is_nil() and gm.is_nil()
    # a reversed range and a range past the elements: nothing is touched
    for i, v in ((50, int(it["off"][49]) - 1), (200, int(it["off"][200]) + 1)):
        bad = it["off"].copy()
        bad[i] = v
        with pytest.raises(_lib.SyzsigError) as e:
            gpu.corpus_add_inputs(_t(gpu, bad, np.int64), d[1], d[2], gc, gm)
        assert e.value.code == _lib.SYZSIG_EINVAL
        assert gc.equal(snap) and gm.is_nil()
    with pytest.raises(_lib.SyzsigError):  # corpusSignal and maxSignal are two sets
        h = ctypes.c_void_p(gc.handle.value)
        _lib.check(gpu.L.syzsig_corpus_add_inputs_dev(gpu.eng.h, d[0].data_ptr(), d[1].data_ptr(), d[1].numel(),
                                                      d[2].data_ptr(), 200, None, ctypes.byref(h), ctypes.byref(h)))
    assert gc.equal(snap)


# ---------------------------------------------------------------- the chain

def test_chain_triage_to_corpus(gpu):
    """triage_batch -> triage_items -> triage_runs (three synthetic re-runs that
    drop some elements) -> corpus_add_inputs with item_keep, against the
    oracle's triage_batch_into -> restatement -> oracle.triage_runs -> the
    sequential Merge loop.  The device CSR goes to triage_runs as it is."""
    rng = np.random.default_rng(17)
    cfg = synth.synth_default()
    nprog, cpp, runs = 8, 8, 3
    cl = synth.call_lengths(nprog, cpp, 0, ragged=(0, 600), seed=4)
    pcs, cs, dcl, prio = gpu.synth_traces(cfg, 0, nprog, cpp, torch.from_numpy(cl.view(np.int32)))
    pidx = torch.from_numpy(synth.prog_call_index(nprog, cpp).view(np.int32)).to(gpu.dev)
    sigs, cnt, _ = gpu.edge_derive(pcs, cs, dcl, pidx)
    # the oracle's executor gives the batch's signals; M0 = a small synthetic part plus all of every third call's
    # signal at the top prio, so those calls (and only some others) bring nothing new
    hpcs, hcs, hprio = synth.traces(cfg, 0, nprog, cpp, cl)
    hs, hcnt, _ = O.exec_batch(hpcs, hcs, cl, synth.prog_call_index(nprog, cpp))
    m0e, m0p = synth.m0(cfg, 64, 3000)
    known = np.unique(np.concatenate([hs[int(hcs[c]):int(hcs[c]) + int(hcnt[c])] for c in range(0, hcnt.size, 3)]))
    known = known[~np.isin(known, m0e)]
    m0e, m0p = np.concatenate([m0e, known]), np.concatenate([m0p, np.full(known.size, 3, np.int8)])
    ms, ns = S.Serial(m0e, m0p).Deserialize(gpu.eng), S.Signal(None, gpu.eng)
    _, cnew, _ = gpu.triage(ms, ns, sigs, cs, cnt, prio)
    oms = O.deserialize(m0e, m0p)
    _, _, ocnew = O.triage_batch_into(oms, hs, hcs, hcnt, hprio)
    ocnew = ocnew[:hcnt.size]
    np.testing.assert_array_equal(cnew.cpu().numpy(), ocnew)
    assert 2 < ocnew.sum() < ocnew.size
    # corpusSignal: a third of M0 and some of the batch's own elements
    ce = np.unique(np.concatenate([m0e[::3], hs[hs != 0][::5]]))
    cp = rng.integers(0, 4, ce.size).astype(np.int8)
    gcorp, ocorp = S.Serial(ce, cp).Deserialize(gpu.eng), O.deserialize(ce, cp)
    ref = R.triage_items(ocorp, hs, hcs, hcnt, hprio, ocnew)
    it = gpu.triage_items(sigs, cs, cnt, prio, cnew, corpus_signal=gcorp)
    for k, _, _, _ in OUT:
        np.testing.assert_array_equal(it[k].cpu().numpy(), _signed(ref[k]), err_msg=k)
    ni = ref["item_call"].size
    # three re-runs per item: the item's inputSignal with some elements dropped, a few strangers, some runs skipped
    flags = rng.integers(0, 4, ni).astype(np.uint8)
    run_sigs, run_prio, run_errno, run_exec = [], [], [], []
    for i in range(ni):
        e = ref["input_elems"][int(ref["input_off"][i]):int(ref["input_off"][i + 1])]
        for _ in range(runs):
            kept = e[rng.random(e.size) < rng.choice([1.0, 0.9, 0.5])]
            run_sigs.append(np.concatenate([kept, rng.integers(0, 99, 3).astype(np.uint32)])
                            if rng.random() < 0.9 or i == 0 else kept[:0])
            run_prio.append(int(np.uint8(ref["item_prio"][i])) if rng.random() < 0.8 or i == 0 else int(rng.integers(0, 4)))
            run_errno.append(int(rng.choice([0, 0, 0, 22])) if i != 0 else 0)
            run_exec.append(int(rng.random() < 0.9) if i > 1 else 1 - i)  # item 0 always runs, item 1 never: dropped
    run_off = np.cumsum([0] + [s.size for s in run_sigs]).astype(np.uint64)
    run_sigs = np.concatenate(run_sigs).astype(np.uint32)
    run_prio, run_errno, run_exec = (np.array(run_prio, np.uint8), np.array(run_errno, np.int32),
                                     np.array(run_exec, np.uint8))
    keep, elem_keep = gpu.triage_runs(it["item_off"], it["elems"], it["prios"], _t(gpu, flags, np.uint8), runs,
                                      _t(gpu, run_off, np.int64), _t(gpu, run_sigs, np.int32),
                                      _t(gpu, run_prio, np.uint8), _t(gpu, run_errno, np.int32),
                                      _t(gpu, run_exec, np.uint8))
    okeep, finals = O.triage_runs(ref["item_off"], ref["elems"], ref["prios"], flags, runs, run_off, run_sigs, run_prio,
                                  run_errno, run_exec)
    np.testing.assert_array_equal(keep.cpu().numpy(), okeep)
    ek = elem_keep.cpu().numpy()
    for i, f in enumerate(finals):
        a, b = int(ref["item_off"][i]), int(ref["item_off"][i + 1])
        if f is not None:
            assert set(ref["elems"][a:b][ek[a:b] != 0].tolist()) == set(f)
    assert 0 < okeep.sum() < ni
    gpu.corpus_add_inputs(it["input_off"], it["input_elems"], it["item_prio"], gcorp, ms, item_keep=keep)
    R.add_inputs(ocorp, oms, ref["input_off"], ref["input_elems"], ref["item_prio"], okeep)
    _same(gcorp, ocorp)
    _same(ms, oms)
