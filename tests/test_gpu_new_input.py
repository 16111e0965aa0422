"""GPU: the manager's NewInput over a batch of inputs (csrc/corpus.hip,
syzsig_manager_new_input_batch) against the reference's loop restated over the
oracle's Signal and Cover ops (tests/corpus_ref.py: syz-manager/manager.go:
976-1025), as dicts and sets."""
import ctypes

import numpy as np
import pytest

from tests import corpus_ref as R

pytestmark = pytest.mark.gpu


def _serial(rng, n, U, dup=True):
    e = rng.integers(0, U, size=n).astype(np.uint32)  # duplicates inside a Serial: the later one wins
    if not dup:
        e = np.unique(e)
    p = rng.integers(-3, 5, size=e.size).astype(np.int8)
    return e, p


def _device_sets(gpu, sig0, cov0):
    from syzkaller_amd import signal as S

    cs = S.Serial(*sig0).Deserialize(gpu.eng) if sig0 is not None else S.Signal(None, gpu.eng)
    cc = S.Cover(gpu.eng)
    if cov0 is not None:
        cc.Merge(np.asarray(cov0, np.uint32))
    return cs, cc


def _ref_manager(sig0, cov0):
    from oracle import oracle as O

    mgr = R.Manager(O.deserialize(*sig0) if sig0 is not None else None)
    if cov0 is not None:
        mgr.corpusCover.Merge(cov0)
    return mgr


def _check(gpu, sig0, cov0, rows, nkeys):
    """Device vs corpus_ref on one batch; returns the device's path statistics and `accepted`."""
    from syzkaller_amd import signal as S

    cs, cc = _device_sets(gpu, sig0, cov0)
    acc, new, entries = S.manager_new_input(cs, cc, [(k, S.Serial(*s), c, p) for k, s, c, p in rows], nkeys, gpu.eng)
    stats = S.new_input_stats(gpu.eng)
    mgr = _ref_manager(sig0, cov0)
    racc, rnew, rentries = R.new_input_batch(mgr, rows)
    np.testing.assert_array_equal(acc, racc)
    np.testing.assert_array_equal(new, rnew)
    assert set(entries) == set(rentries)
    for k, (ser, cov) in entries.items():
        e, c = ser.Elems.astype(np.int64), cov.astype(np.int64)
        assert (np.diff(e) > 0).all() and (np.diff(c) > 0).all(), f"key {k}: not ascending and distinct"
        assert dict(zip(ser.Elems.tolist(), ser.Prios.tolist())) == rentries[k][0], f"key {k} signal"
        assert set(cov.tolist()) == rentries[k][1], f"key {k} cover"
    assert cs.is_nil() == mgr.corpusSignal.is_nil()
    assert cs.to_dict() == mgr.corpusSignal.to_dict()
    assert cc.is_nil() == (mgr.corpusCover.c is None)
    assert set(cc.Serialize().tolist()) == (mgr.corpusCover.c or set()) and len(cc) == len(mgr.corpusCover.c or ())
    return stats, acc


def _random_rows(rng, K, U, n, ncov=200, present=0.2):
    nkeys = max(K // 3, 1)
    rows, seen = [], set()
    for _ in range(K):
        k = int(rng.integers(0, nkeys))
        pres = k not in seen and rng.random() < 3 * present  # an old entry comes before its key's inputs
        seen.add(k)
        cov = rng.integers(0, 4 * ncov, size=int(rng.integers(0, ncov))).astype(np.uint32)
        rows.append((k, _serial(rng, int(rng.integers(0, n + 1)), U), cov, bool(pres)))
    return rows, nkeys


@pytest.mark.parametrize("seed,K,U,n", [(0, 40, 3000, 800), (1, 8, 500, 100), (2, 40, 3000, 800), (3, 30, 200, 50)])
def test_new_input_batch_vs_reference_loop(gpu, seed, K, U, n):
    rng = np.random.default_rng(seed)
    rows, nkeys = _random_rows(rng, K, U, n)
    sig0 = _serial(rng, 2 * n, U, dup=False)
    cov0 = rng.integers(0, 800, size=100).astype(np.uint32)
    stats, _ = _check(gpu, sig0, cov0, rows, nkeys)
    assert stats["sequential"] == 0


@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_new_input_hand_derived_cases(gpu, case):
    from syzkaller_amd import signal as S

    _, sig0, cov0, rows, acc, new, entries, sig1, cov1 = case
    cs, cc = _device_sets(gpu, R.ser(sig0) if sig0 is not None else None, cov0)
    nkeys = 1 + max(r[0] for r in rows)
    got_acc, got_new, got = S.manager_new_input(cs, cc, [(k, S.Serial(*s), np.asarray(c, np.uint32), p)
                                                         for k, s, c, p in rows], nkeys, gpu.eng)
    assert got_acc.tolist() == acc and got_new.tolist() == new
    assert {k: (dict(zip(s.Elems.tolist(), s.Prios.tolist())), set(c.tolist())) for k, (s, c) in got.items()} == entries
    assert cs.is_nil() == (sig1 is None) and cs.to_dict() == (sig1 or {})
    assert cc.is_nil() == (cov1 is None) and set(cc.Serialize().tolist()) == (cov1 or set())


@pytest.mark.parametrize("case", ["forced_sequential", "hot_element"])
def test_new_input_sequential_path_vs_reference_loop(gpu, case):
    """The exact fallback of acceptance (the reference loop over the set ops on
    clones): forced (SYZSIG_DEBUG_RECS_GATE gates every element partition), or
    taken because one element is in each of 3000 rows (its partition holds
    more than 2048 entries).  The per-key merge is the batched one."""
    from syzkaller_amd._lib import SYZSIG_DEBUG_RECS_GATE

    rng = np.random.default_rng(11)
    U = 4000
    K, n = (40, 300) if case == "forced_sequential" else (3000, 20)
    rows, nkeys = _random_rows(rng, K, U, n, ncov=10 if case == "hot_element" else 200)
    if case == "hot_element":
        rows = [(k, (np.append(e, np.uint32(7)), np.append(p, np.int8(rng.integers(-3, 5)))), c, pr)
                for k, (e, p), c, pr in rows]
    sig0 = _serial(rng, 1000, U, dup=False)
    gpu.eng.set_debug(SYZSIG_DEBUG_RECS_GATE if case == "forced_sequential" else 0)
    try:
        stats, _ = _check(gpu, sig0, [1, 2, 3], rows, nkeys)
    finally:
        gpu.eng.set_debug(0)
    assert stats["sequential"] == 1


def test_new_input_key_group_sizes_and_long_paths(gpu):
    """Keys whose accepted rows hold 0, 1, 2, 3, T-1, T, T+1, 2T+3, 3T and 4T
    entries (T = SYZSIG_CORPUS_TILE, the LDS sort's tile; past it a key is
    tile-sorted and rank-merged through the workspace: two passes for 2T+3 to
    4T; 3T: an odd tile count, the last run of the first pass has no partner;
    4T: a full last tile; T+1 is copied through the second pass), the entries
    split over two rows that share elements, with duplicates inside a row; and
    one key whose covers hold 2 * SYZSIG_COVER_TILE + 3 PCs (cover.hip's long
    path).  Asserts that the long paths were taken."""
    from syzkaller_amd._lib import SYZSIG_CORPUS_TILE as T, SYZSIG_COVER_TILE as CT

    rng = np.random.default_rng(3)
    sizes = [0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 3, 3 * T, 4 * T]
    rows = []
    for k, sz in enumerate(sizes):
        base = 100_000 * (k + 1)
        if sz == 0:
            rows.append((k, R.ser([]), np.arange(5, dtype=np.uint32), False))  # rejected: no live entry
            continue
        na = sz // 2 if sz >= 2 else 0
        nb = sz - na
        ncov = 2 * CT + 3 if sz == T + 1 else 30
        cov = rng.integers(0, 3 * ncov, size=ncov).astype(np.uint32)
        if na:
            ea = (base + rng.integers(0, max(na // 2, 1), size=na)).astype(np.uint32)
            rows.append((k, (ea, rng.integers(-3, 5, size=na).astype(np.int8)), cov[: ncov // 2], False))
        # the second row shares elements with the first and brings one of its own, so it is accepted too
        eb = (base + rng.integers(0, max(nb // 2, 1), size=nb)).astype(np.uint32)
        eb[int(rng.integers(0, nb))] = base + 50_000
        rows.append((k, (eb, rng.integers(-3, 5, size=nb).astype(np.int8)), cov[ncov // 2:] if na else cov, False))
    # the keys interleaved: every key's first row, then the second rows (a key's rows keep their order)
    nth, seen = [], {}
    for r in rows:
        nth.append(seen.get(r[0], 0))
        seen[r[0]] = nth[-1] + 1
    rows = [rows[i] for i in sorted(range(len(rows)), key=lambda i: nth[i])]
    stats, acc = _check(gpu, None, None, rows, len(sizes))
    assert acc.tolist() == [int(r[1][0].size > 0) for r in rows]  # every non-empty row is live
    live = {k: sum(r[1][0].size for r in rows if r[0] == k) for k in range(len(sizes))}
    assert [live[k] for k in range(len(sizes))] == sizes
    assert stats == {"sequential": 0, "large_keys": 4, "merge_passes": 2, "large_covers": 1}


def _raw_call(eng, cs, cc, keys, flags, sig_off, elems, prios, cov_off, cover, nkeys, sig_cap, cov_cap, bufs):
    def p(a):
        return ctypes.c_void_p(a.ctypes.data)

    sh = ctypes.c_void_p(cs.handle.value or 0)
    ch = ctypes.c_void_p(cc._s.handle.value or 0)
    rc = eng.L.syzsig_manager_new_input_batch(
        eng.h, ctypes.byref(sh), ctypes.byref(ch), len(keys), nkeys, p(keys), p(flags), p(sig_off), p(elems), p(prios),
        p(cov_off), p(cover), p(bufs["accepted"]), p(bufs["new_key"]), p(bufs["touched"]), p(bufs["sig_off"]),
        p(bufs["elems"]), p(bufs["prios"]), sig_cap, p(bufs["cov_off"]), p(bufs["cover"]), cov_cap)
    return rc, sh, ch


def _flat(rows):
    keys = np.array([r[0] for r in rows], np.uint32)
    flags = np.array([1 if r[3] else 0 for r in rows], np.uint8)
    sig_off = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum(np.array([r[1][0].size for r in rows], np.uint64), out=sig_off[1:])
    cov_off = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum(np.array([np.asarray(r[2]).size for r in rows], np.uint64), out=cov_off[1:])
    elems = np.concatenate([r[1][0] for r in rows] + [np.empty(0, np.uint32)]).astype(np.uint32)
    prios = np.concatenate([r[1][1] for r in rows] + [np.empty(0, np.int8)]).astype(np.int8)
    cover = np.concatenate([np.asarray(r[2], np.uint32) for r in rows] + [np.empty(0, np.uint32)]).astype(np.uint32)
    return keys, flags, sig_off, elems, prios, cov_off, cover


def _bufs(K, nkeys, n, c, slack=64):
    return {"accepted": np.full(K + slack, 0xA5, np.uint8), "new_key": np.full(K + slack, 0xA5, np.uint8),
            "touched": np.full(nkeys + slack, 0xA5, np.uint8), "sig_off": np.full(nkeys + 1 + slack, 0xA5A5, np.uint64),
            "elems": np.full(n + slack, 0xA5A5A5A5, np.uint32), "prios": np.full(n + slack, 0x5A, np.int8),
            "cov_off": np.full(nkeys + 1 + slack, 0xA5A5, np.uint64), "cover": np.full(c + slack, 0xA5A5A5A5, np.uint32)}


def test_new_input_outputs_stay_inside_their_ranges(gpu):
    """The raw C call into pre-filled buffers: nothing is written past the
    rows, the keys, or the CSR totals."""
    from syzkaller_amd._lib import SYZSIG_OK

    rng = np.random.default_rng(21)
    rows, nkeys = _random_rows(rng, 24, 2000, 300)
    sig0 = _serial(rng, 500, 2000, dup=False)
    cs, cc = _device_sets(gpu, sig0, [9, 8])
    flat = _flat(rows)
    K, n, c = len(rows), int(flat[2][-1]), int(flat[5][-1])
    bufs = _bufs(K, nkeys, n, c)
    rc, _, _ = _raw_call(gpu.eng, cs, cc, *flat, nkeys, n, c, bufs)
    assert rc == SYZSIG_OK
    mgr = _ref_manager(sig0, [9, 8])
    racc, rnew, rentries = R.new_input_batch(mgr, rows)
    np.testing.assert_array_equal(bufs["accepted"][:K], racc)
    np.testing.assert_array_equal(bufs["new_key"][:K], rnew)
    assert sorted(np.flatnonzero(bufs["touched"][:nkeys]).tolist()) == sorted(rentries)
    so, co = bufs["sig_off"][: nkeys + 1].tolist(), bufs["cov_off"][: nkeys + 1].tolist()
    assert so[0] == 0 and co[0] == 0 and so == sorted(so) and co == sorted(co)
    for k in range(nkeys):
        e, pr, cv = bufs["elems"][so[k]:so[k + 1]], bufs["prios"][so[k]:so[k + 1]], bufs["cover"][co[k]:co[k + 1]]
        exp = rentries.get(k, ({}, set()))
        assert dict(zip(e.tolist(), pr.tolist())) == exp[0] and e.size == len(exp[0])
        assert set(cv.tolist()) == exp[1] and cv.size == len(exp[1])
    assert (bufs["accepted"][K:] == 0xA5).all() and (bufs["new_key"][K:] == 0xA5).all()
    assert (bufs["touched"][nkeys:] == 0xA5).all()
    assert (bufs["sig_off"][nkeys + 1:] == 0xA5A5).all() and (bufs["cov_off"][nkeys + 1:] == 0xA5A5).all()
    assert (bufs["elems"][so[-1]:] == 0xA5A5A5A5).all() and (bufs["prios"][so[-1]:] == 0x5A).all()
    assert (bufs["cover"][co[-1]:] == 0xA5A5A5A5).all()
    assert cs.to_dict() == mgr.corpusSignal.to_dict() and set(cc.Serialize().tolist()) == mgr.corpusCover.c


@pytest.mark.parametrize("what", ["sig_cap", "cover_cap", "key", "sig_off", "cover_off"])
def test_new_input_errors_leave_everything(gpu, what):
    """SYZSIG_ERANGE (a capacity below the rows' totals) and SYZSIG_EINVAL (a
    key >= nkeys, a non-monotone offset) are checked before anything is
    touched: both sets equal clones taken before (syzsig_set_equal) and every
    output buffer is as it was."""
    from syzkaller_amd._lib import SYZSIG_EINVAL, SYZSIG_ERANGE

    rng = np.random.default_rng(5)
    rows, nkeys = _random_rows(rng, 12, 1000, 100, present=0)
    sig0 = _serial(rng, 300, 1000, dup=False)
    cs, cc = _device_sets(gpu, sig0, [1, 2, 3, 4])
    cs0, cc0 = cs.clone(), cc._s.clone()
    keys, flags, sig_off, elems, prios, cov_off, cover = _flat(rows)
    K, n, c = len(rows), int(sig_off[-1]), int(cov_off[-1])
    assert n > 0 and c > 0
    sig_cap, cov_cap, want = n, c, SYZSIG_EINVAL
    if what == "sig_cap":
        sig_cap, want = n - 1, SYZSIG_ERANGE
    elif what == "cover_cap":
        cov_cap, want = c - 1, SYZSIG_ERANGE
    elif what == "key":
        keys[K - 1] = nkeys
    elif what == "sig_off":
        sig_off[K // 2] = sig_off[K // 2 + 1] + 1
    else:
        cov_off[K // 2] = cov_off[K // 2 + 1] + 1
    bufs = _bufs(K, nkeys, n, c)
    before = {k: v.copy() for k, v in bufs.items()}
    rc, sh, ch = _raw_call(gpu.eng, cs, cc, keys, flags, sig_off, elems, prios, cov_off, cover, nkeys, sig_cap, cov_cap,
                           bufs)
    assert rc == want
    assert sh.value == cs.handle.value and ch.value == cc._s.handle.value
    assert cs.equal(cs0) and cc._s.equal(cc0)
    for k, v in bufs.items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)
