"""GPU: the manager's Poll over a batch of polls (csrc/poll.hip,
syzsig_manager_poll_batch) against the reference's sequential loop restated
over the oracle's Signal ops (oracle.poll: syz-manager/manager.go:1027-1052)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.table_keys import fmix32_inv_np, fmix32_np

pytestmark = pytest.mark.gpu


def _serial(rng, n, U, dup=True):
    e = rng.integers(0, U, size=n).astype(np.uint32)  # duplicates inside a Serial: the later one wins
    if not dup:
        e = np.unique(e)
    p = rng.integers(-3, 5, size=e.size).astype(np.int8)
    return e, p


@pytest.mark.parametrize("seed,F,K,U,n,limits", [(0, 5, 40, 3000, 400, None), (1, 1, 8, 500, 100, None),
                                                 (2, 16, 200, 50_000, 3000, None), (3, 3, 30, 200, 50, None),
                                                 (4, 5, 40, 3000, 400, (24, 4000))])
def test_poll_batch_vs_sequential_oracle(gpu, monkeypatch, seed, F, K, U, n, limits):
    """limits: (polls x fuzzers, entries x fuzzers) per library call lowered so
    that signal.manager_poll applies the batch as several consecutive calls."""
    from syzkaller_amd import signal as S

    if limits:
        monkeypatch.setattr(S, "POLL_MAX_NEXT", limits[0])
        monkeypatch.setattr(S, "POLL_MAX_FANOUT", limits[1])
    rng = np.random.default_rng(seed)
    m0 = _serial(rng, 4 * n, U, dup=False)
    pre = [None if rng.random() < 0.3 else _serial(rng, int(rng.integers(0, n)), U, dup=False) for _ in range(F)]
    polls = [(int(rng.integers(0, F)), _serial(rng, int(rng.integers(0, 2 * n)), U)) for _ in range(K)]
    # device
    ms = S.Serial(*m0).Deserialize(gpu.eng)
    nm = [S.Serial(*p).Deserialize(gpu.eng) if p is not None else S.Signal(None, gpu.eng) for p in pre]
    replies = S.manager_poll(ms, nm, [(f, S.Serial(e, p)) for f, (e, p) in polls], gpu.eng)
    # oracle: one poll after the other
    oms = O.deserialize(*m0)
    onm = [O.deserialize(*p) if p is not None else O.OSig() for p in pre]
    for i, (f, ser) in enumerate(polls):
        re, rp = O.poll(oms, onm, f, ser)
        got = dict(zip(replies[i].Elems.tolist(), replies[i].Prios.tolist()))
        assert got == dict(zip(re.tolist(), rp.tolist())), f"reply {i}"
    assert ms.to_dict() == oms.to_dict()
    for g in range(F):
        assert (nm[g].to_dict() if not nm[g].is_nil() else {}) == onm[g].to_dict(), f"fuzzer {g}"
        assert nm[g].is_nil() == onm[g].is_nil() or onm[g].Len() == 0


PBITS = 7  # csrc/recs.hip rp_pbits for a batch of at most 2^17 entries: partition = the top 7 bits of fmix32(e)
GROUP_CAP = 2048  # csrc/internal.h kRpCap


def _in_partition(rng, p, n):
    """n distinct elements of element partition p"""
    r = rng.choice(1 << (32 - PBITS), size=n, replace=False).astype(np.uint64)
    return fmix32_inv_np(((np.uint64(p) << np.uint64(32 - PBITS)) | r).astype(np.uint32))


@pytest.mark.parametrize("case", ["1_2_3", "cap"])
def test_poll_batch_partition_sizes(gpu, case):
    """The LDS sort of k_poll_part_walk at its edges: partitions of exactly 1,
    2 and 3 entries (sorts of 1, 2 and 4 keys, the last one padded), and a
    partition of exactly kRpCap entries (the largest batched case: the
    whole tile, no pad)."""
    from syzkaller_amd import signal as S

    rng = np.random.default_rng(41)
    F = 3
    if case == "1_2_3":
        K = 6
        a, b, c, d = (int(_in_partition(rng, p, 1)[0]) for p in (0, 1, 2, 2))
        special = {0: [(b, 1)], 1: [(c, 3), (c, -1)], 2: [(a, 2)], 3: [(b, 4)], 4: [(d, 0)]}
        want = {0: 1, 1: 2, 2: 3}
        m0_extra = ([b], [2])
        fill = [int(x) for x in range(3, 1 << PBITS)]
    else:
        K = 8
        hot = _in_partition(rng, 9, GROUP_CAP // K)
        special = {i: list(zip(hot.tolist(), rng.integers(-3, 5, hot.size).tolist())) for i in range(K)}
        want = {9: GROUP_CAP}
        m0_extra = (hot[::2].tolist(), rng.integers(-3, 5, hot[::2].size).tolist())
        fill = [p for p in range(1 << PBITS) if p != 9]
    pool = np.concatenate([_in_partition(rng, p, 4) for p in fill])
    polls = []
    for i in range(K):
        e = rng.choice(pool, size=200).astype(np.uint32)
        p = rng.integers(-3, 5, e.size).astype(np.int8)
        se, sp = zip(*special[i]) if special.get(i) else ((), ())
        at = rng.integers(0, e.size + 1)  # the chosen entries in order, somewhere inside the Serial
        polls.append((int(rng.integers(0, F)), (np.concatenate([e[:at], np.array(se, np.uint32), e[at:]]),
                                                np.concatenate([p[:at], np.array(sp, np.int8), p[at:]]))))
    m0e = np.concatenate([rng.choice(pool, size=150, replace=False), np.array(m0_extra[0], np.uint32)]).astype(np.uint32)
    m0 = (m0e, np.concatenate([rng.integers(-3, 5, 150), np.array(m0_extra[1])]).astype(np.int8))
    # the partitions' sizes, before anything runs on the device
    entries = np.concatenate([e for _, (e, _) in polls])
    assert (entries.size >> PBITS) <= 1024  # rp_pbits stays at PBITS
    sizes = np.bincount(fmix32_np(entries) >> np.uint32(32 - PBITS), minlength=1 << PBITS)
    assert all(sizes[p] == n for p, n in want.items()) and sizes.max() <= GROUP_CAP
    ms = S.Serial(*m0).Deserialize(gpu.eng)
    nm = [S.Signal(None, gpu.eng) for _ in range(F)]
    replies = S.manager_poll(ms, nm, [(f, S.Serial(e, p)) for f, (e, p) in polls], gpu.eng)
    oms = O.deserialize(*m0)
    onm = [O.OSig() for _ in range(F)]
    for i, (f, ser) in enumerate(polls):
        re, rp = O.poll(oms, onm, f, ser)
        got = dict(zip(replies[i].Elems.tolist(), replies[i].Prios.tolist()))
        assert got == dict(zip(re.tolist(), rp.tolist())), f"reply {i}"
    assert ms.to_dict() == oms.to_dict()
    for g in range(F):
        assert (nm[g].to_dict() if not nm[g].is_nil() else {}) == onm[g].to_dict(), f"fuzzer {g}"


def test_poll_batch_empty_and_nil_max(gpu):
    from syzkaller_amd import signal as S

    ms = S.Signal(None, gpu.eng)
    nm = [S.Signal(None, gpu.eng) for _ in range(3)]
    rep = S.manager_poll(ms, nm, [(0, S.Serial()), (1, S.Serial([7, 8, 7], [1, 2, 0])), (0, S.Serial())], gpu.eng)
    assert [r.Elems.size for r in rep] == [0, 0, 2]
    assert dict(zip(rep[2].Elems.tolist(), rep[2].Prios.tolist())) == {7: 0, 8: 2}
    assert ms.to_dict() == {7: 0, 8: 2}
    assert nm[0].is_nil() and nm[1].is_nil() and nm[2].to_dict() == {7: 0, 8: 2}


def test_poll_batch_nil_max_stays_nil_without_events(gpu):
    """manager.go:1033-1034: maxSignal.Merge runs only for a non-empty newMax, so
    a nil maxSignal polled with empty Serials stays nil -- while a newMaxSignal
    from before the batch still goes out as its fuzzer's reply."""
    from syzkaller_amd import signal as S

    pre = (np.array([3, 4], np.uint32), np.array([1, 0], np.int8))
    empty = (np.empty(0, np.uint32), np.empty(0, np.int8))
    order = [1, 0, 0]
    ms, nm = S.Signal(None, gpu.eng), [S.Serial(*pre).Deserialize(gpu.eng), S.Signal(None, gpu.eng)]
    rep = S.manager_poll(ms, nm, [(f, S.Serial()) for f in order], gpu.eng)
    oms, onm = O.OSig(), [O.deserialize(*pre), O.OSig()]
    for i, f in enumerate(order):
        re, rp = O.poll(oms, onm, f, empty)
        assert dict(zip(rep[i].Elems.tolist(), rep[i].Prios.tolist())) == dict(zip(re.tolist(), rp.tolist())), f"reply {i}"
    assert dict(zip(rep[1].Elems.tolist(), rep[1].Prios.tolist())) == {3: 1, 4: 0}
    assert ms.is_nil() and oms.is_nil() and nm[0].is_nil() and nm[1].is_nil()
    # an existing maxSignal polled at or below its prios: no event either, nothing changes
    ms = S.Serial(*pre).Deserialize(gpu.eng)
    rep = S.manager_poll(ms, nm, [(0, S.Serial([3, 4, 3], [1, -1, 0]))], gpu.eng)
    assert rep[0].Elems.size == 0 and ms.to_dict() == {3: 1, 4: 0} and ms.Len() == 2
    assert nm[0].is_nil() and nm[1].is_nil()


@pytest.mark.parametrize("case", ["forced_sequential", "hot_element"])
def test_poll_batch_sequential_path_vs_oracle(gpu, case):
    """The batch's exact fallback (csrc/poll.hip poll_sequential: the
    reference loop over the set ops) -- forced (SYZSIG_DEBUG_RECS_GATE gates
    every element partition), or taken because one element is in every one of
    3000 polls (its partition holds more than 2048 entries) -- against the
    oracle's sequential loop."""
    from syzkaller_amd import signal as S
    from syzkaller_amd._lib import SYZSIG_DEBUG_RECS_GATE

    rng = np.random.default_rng(11)
    F, U = 6, 4000
    K, n = (40, 300) if case == "forced_sequential" else (3000, 20)
    m0 = _serial(rng, 1000, U, dup=False)
    pre = [None if g % 3 == 0 else _serial(rng, 50, U, dup=False) for g in range(F)]
    polls = []
    for _ in range(K):
        e, p = _serial(rng, int(rng.integers(0, n)), U)
        if case == "hot_element":
            e, p = np.append(e, np.uint32(7)), np.append(p, np.int8(rng.integers(-3, 5)))
        polls.append((int(rng.integers(0, F)), (e, p)))
    ms = S.Serial(*m0).Deserialize(gpu.eng)
    nm = [S.Serial(*p).Deserialize(gpu.eng) if p is not None else S.Signal(None, gpu.eng) for p in pre]
    gpu.eng.set_debug(SYZSIG_DEBUG_RECS_GATE if case == "forced_sequential" else 0)
    try:
        replies = S.manager_poll(ms, nm, [(f, S.Serial(e, p)) for f, (e, p) in polls], gpu.eng)
    finally:
        gpu.eng.set_debug(0)
    oms = O.deserialize(*m0)
    onm = [O.deserialize(*p) if p is not None else O.OSig() for p in pre]
    for i, (f, ser) in enumerate(polls):
        re, rp = O.poll(oms, onm, f, ser)
        got = dict(zip(replies[i].Elems.tolist(), replies[i].Prios.tolist()))
        assert got == dict(zip(re.tolist(), rp.tolist())), f"reply {i}"
    assert ms.to_dict() == oms.to_dict()
    for g in range(F):
        assert (nm[g].to_dict() if not nm[g].is_nil() else {}) == onm[g].to_dict(), f"fuzzer {g}"


def test_poll_batch_sequential_failure_leaves_sets(gpu):
    """the sequential fallback is all or nothing like
    the batched path -- a failure before its last poll (injected,
    SYZSIG_DEBUG_POLL_FAIL) leaves maxSignal and every fuzzer's newMaxSignal
    as they were (nil ones nil), and hands out no reply."""
    from syzkaller_amd import signal as S
    from syzkaller_amd._lib import SYZSIG_DEBUG_POLL_FAIL, SYZSIG_DEBUG_RECS_GATE, SyzsigError

    rng = np.random.default_rng(5)
    F, U, K = 4, 3000, 12
    m0 = _serial(rng, 800, U, dup=False)
    pre = [None if g % 2 == 0 else _serial(rng, 40, U, dup=False) for g in range(F)]
    polls = [(int(rng.integers(0, F)), S.Serial(*_serial(rng, 200, U))) for _ in range(K)]
    ms = S.Serial(*m0).Deserialize(gpu.eng)
    nm = [S.Serial(*p).Deserialize(gpu.eng) if p is not None else S.Signal(None, gpu.eng) for p in pre]
    before = (ms.to_dict(), [None if s.is_nil() else s.to_dict() for s in nm])
    gpu.eng.set_debug(SYZSIG_DEBUG_RECS_GATE | SYZSIG_DEBUG_POLL_FAIL)
    try:
        with pytest.raises(SyzsigError):
            S.manager_poll(ms, nm, polls, gpu.eng)
    finally:
        gpu.eng.set_debug(0)
    assert (ms.to_dict(), [None if s.is_nil() else s.to_dict() for s in nm]) == before
    # and the same batch then goes through, against the oracle
    replies = S.manager_poll(ms, nm, polls, gpu.eng)
    oms = O.deserialize(*m0)
    onm = [O.deserialize(*p) if p is not None else O.OSig() for p in pre]
    for i, (f, ser) in enumerate(polls):
        re, rp = O.poll(oms, onm, f, (np.asarray(ser.Elems), np.asarray(ser.Prios)))
        assert dict(zip(replies[i].Elems.tolist(), replies[i].Prios.tolist())) == dict(zip(re.tolist(), rp.tolist()))
    assert ms.to_dict() == oms.to_dict()
