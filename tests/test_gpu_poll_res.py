"""GPU: the reply to a fuzzer's poll over a batch of Serials (csrc/pollres.hip,
syzsig_fuzzer_poll_res_dev) against the reference's sequential loop restated
over the oracle's Signal ops (tests/poll_res_ref.py: syz-fuzzer/fuzzer.go:
344-350, :433-460, :468-475).  Compared: both sets' Serialize as sorted
(elem, prio) lists, their Len, and which of them stayed nil."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import poll_res_ref as R
from tests import pollres_keys as K
from tests.table_keys import hot_first, hot_last

pytestmark = pytest.mark.gpu

T = K.TILE
MS, IN = R.SEG_MAXSIGNAL, R.SEG_INPUT
PRIOS = np.array([-128, -3, -2, -1, 0, 1, 2, 3, 4, 127], np.int8)  # test_gpu_poll.py's eight, and the int8 ends


def _pairs(sig):
    """(elems ascending, their prios, Len) of a device Signal or an OSig; a nil one is empty."""
    if sig.is_nil():
        return np.empty(0, np.uint32), np.empty(0, np.int8), 0
    s = sig.Serialize()
    e, p = (s.Elems, s.Prios) if hasattr(s, "Elems") else s
    o = np.argsort(e, kind="stable")
    return np.asarray(e)[o], np.asarray(p)[o], sig.Len()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _rand_set(rng, n, U):
    e = rng.choice(U, size=min(n, U), replace=False).astype(np.uint32)
    return e, rng.choice(PRIOS, size=e.size)


def _rand_seg(rng, kind, n, U):
    return kind, rng.integers(0, U, size=n).astype(np.uint32), rng.choice(PRIOS, size=n)  # duplicates: the last wins


def _dev_sets(gpu, c0, m0):
    from syzkaller_amd import signal as S

    return tuple(S.Serial(*x).Deserialize(gpu.eng) if x is not None else S.Signal(None, gpu.eng) for x in (c0, m0))


def _ora_sets(c0, m0):
    return tuple(O.deserialize(*x) if x is not None else O.OSig() for x in (c0, m0))


def _tensors(gpu, segs):
    import torch

    off = np.zeros(len(segs) + 1, np.int64)
    np.cumsum(np.array([e.size for _, e, _ in segs], np.int64), out=off[1:])
    kind = np.array([k for k, _, _ in segs], np.uint8)
    elems = np.concatenate([e for _, e, _ in segs] + [np.empty(0, np.uint32)]).astype(np.uint32)
    prios = np.concatenate([p for _, _, p in segs] + [np.empty(0, np.int8)]).astype(np.int8)
    return tuple(torch.from_numpy(x).to(gpu.dev) for x in (off, kind, elems.view(np.int32), prios))


def _check(gpu, c0, m0, segs, paths=True):
    """Runs the batch on the device and the restatement, compares, and returns
    the device sets and the stats.  paths: the short / long counts, the losers
    and the scratch bytes follow from the segments alone."""
    cs, ms = _dev_sets(gpu, c0, m0)
    gpu.poll_res(*_tensors(gpu, segs), cs, ms)
    st = gpu.poll_res_stats()
    ocs, oms = _ora_sets(c0, m0)
    R.poll_res(ocs, oms, segs)
    assert _same(_pairs(cs), _pairs(ocs)), "corpusSignal"
    assert _same(_pairs(ms), _pairs(oms)), "maxSignal"
    assert cs.is_nil() == ocs.is_nil() and ms.is_nil() == oms.is_nil()
    if paths:
        lens = [e.size for _, e, _ in segs]
        long_bytes = sum(16 * max(2, 1 << int(n).bit_length()) for n in lens if n > T)  # buckets_for(n) x 16 B
        losers = sum(e.size - np.unique(e).size for _, e, _ in segs)
        assert st == (sum(0 < n <= T for n in lens), sum(n > T for n in lens), losers, long_bytes)
    return cs, ms, st


def _rules_differ(c0, m0, segs):
    """On the CPU: a max over the raw entries is another function on these segments."""
    a, b = _ora_sets(c0, m0), _ora_sets(c0, m0)
    R.poll_res(a[0], a[1], segs)
    R.poll_res_raw_max(b[0], b[1], segs)
    return not (_same(_pairs(a[0]), _pairs(b[0])) and _same(_pairs(a[1]), _pairs(b[1])))


LENGTHS = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 262143]


@pytest.mark.parametrize("which", ["batch"] + LENGTHS)
def test_segment_lengths(gpu, which):
    """Every length at which the code takes another path, in one batch and
    alone; the stats tell that the short ones ran in LDS and the long ones
    through the scratch table."""
    rng = np.random.default_rng(7)
    lens = LENGTHS if which == "batch" else [which]
    U = 3000 if which == "batch" else max(2, int(which) // 2 + 1)
    segs = [_rand_seg(rng, (IN, MS)[i % 2], n, max(U, n // 2 + 1)) for i, n in enumerate(lens)]
    c0, m0 = _rand_set(rng, 500, U), _rand_set(rng, 800, U)
    _, _, st = _check(gpu, c0, m0, segs)
    if which == "batch":
        assert st[0] == 7 and st[1] == 3 and st[3] == 16 * (8192 + 16384 + 262144)
        assert _rules_differ(c0, m0, segs)


def _distinct(rng, n, avoid):
    e = rng.choice(1 << 31, size=n + 8, replace=False).astype(np.uint32) + np.uint32(1 << 31)  # all >= 2^31
    return e[~np.isin(e, avoid)][:n]


@pytest.mark.parametrize("case", ["first_last", "lanes", "long_tile", "descending_T", "descending_T1", "hundred"])
def test_placed_duplicates(gpu, case):
    """Duplicates where an index or a boundary could be mishandled; in each the
    later, lower entry must win inside its segment, so the raw-max rule differs."""
    rng = np.random.default_rng(19)
    X = np.uint32(77)
    if case == "first_last":
        e, p = _distinct(rng, 300, [X]), rng.choice(PRIOS, size=300)
        e[0], e[-1], p[0], p[-1] = X, X, 4, -3
        segs = [(IN, e, p)]
    elif case == "lanes":  # across the 64-lane wave and the 256- / 1024-thread boundaries
        e, p = _distinct(rng, T, np.arange(1, 9)), np.full(T, 1, np.int8)
        for v, (i, j) in enumerate([(63, 64), (255, 256), (1023, 1024), (1023 + 1024, 2048), (5, T - 1)], start=1):
            e[i], e[j], p[i], p[j] = v, v, 3, -2
        segs = [(MS, e, p)]
    elif case == "long_tile":  # across the chunk boundaries of a long segment
        n = 2 * T + 3
        e, p = _distinct(rng, n, np.arange(1, 9)), np.full(n, 1, np.int8)
        for v, (i, j) in enumerate([(T - 1, T), (2 * T - 1, 2 * T), (0, n - 1), (T + 1, 2 * T + 1)], start=1):
            e[i], e[j], p[i], p[j] = v, v, 127, -128
        segs = [(IN, e, p)]
    elif case in ("descending_T", "descending_T1"):  # one element, prios 127 down to -128: only the last counts
        n = T if case == "descending_T" else T + 1
        p = (127 - (np.arange(n, dtype=np.int64) * 256) // n).astype(np.int8)
        assert p[0] == 127 and p[-1] == -128 and (np.diff(p.astype(np.int16)) <= 0).all()
        segs = [(IN, np.full(n, X, np.uint32), p)]
    else:  # the same element in 100 segments, last-low in each; the highest of the lasts wins
        segs = []
        for s in range(100):
            e, p = _distinct(rng, 20, [X]), rng.choice(PRIOS, size=20)
            e[3], e[11], p[3], p[11] = X, X, 127, np.int8(s % 7 - 3)
            segs.append(((IN, MS)[s % 3 == 0], e, p))
    c0, m0 = (np.array([X], np.uint32), np.array([-128], np.int8)), None
    cs, ms, st = _check(gpu, c0, m0, segs)
    assert _rules_differ(c0, m0, segs)
    want = {"first_last": -3, "lanes": None, "long_tile": None, "descending_T": -128, "descending_T1": -128, "hundred": 3}
    if want[case] is not None:
        assert ms.to_dict()[int(X)] == want[case]
    assert (st[0], st[1]) == {"long_tile": (0, 1), "descending_T1": (0, 1), "hundred": (100, 0)}.get(case, (1, 0))


@pytest.mark.parametrize("slot", [5, K.SLOTS - 1])
def test_lds_home_slot_collisions(gpu, slot):
    """T / 2 elements of one segment share one home slot of the LDS table (the
    last slot: the chain wraps), each twice, the second entry lower: a probe
    chain of 2048 slots, resolved in LDS (stats), every winner the second entry."""
    rng = np.random.default_rng(3)
    hot = K.same_home(slot, T // 2)
    assert (K.lds_home(hot) == slot).all()
    e = np.concatenate([hot, rng.permutation(hot)])
    p = np.concatenate([np.full(T // 2, 3, np.int8), np.full(T // 2, -1, np.int8)])
    m0 = (hot[::3].copy(), np.full(hot[::3].size, 0, np.int8))
    _, ms, st = _check(gpu, None, m0, [(IN, e, p)])
    assert st == (1, 0, T // 2, 0)
    d = ms.to_dict()
    assert all(d[int(x)] == (0 if i % 3 == 0 else -1) for i, x in enumerate(hot.tolist()))


@pytest.mark.parametrize("n", [600, T + 100])
def test_hbm_home_bucket_chain_wraps(gpu, n):
    """Keys that share the LAST home bucket of every table (tests/table_keys.py):
    one probe chain that wraps the table's end, in maxSignal, corpusSignal and
    (n > T) the long path's scratch table."""
    rng = np.random.default_rng(23)
    hot = hot_last(300)
    e = np.concatenate([hot, hot_first(40), _distinct(rng, n - 340, np.concatenate([hot, hot_first(40)]))])
    e = np.concatenate([e, hot[:50]])  # duplicates of chain keys
    e = e[rng.permutation(e.size)]
    segs = [(IN, e, rng.choice(PRIOS, size=e.size)), (MS, hot[100:250].copy(), rng.choice(PRIOS, size=150))]
    c0 = (hot[:120].copy(), rng.choice(PRIOS, size=120))
    m0 = (hot[60:200].copy(), rng.choice(PRIOS, size=140))
    _check(gpu, c0, m0, segs)


def test_existing_higher_equal_lower(gpu):
    """M0 / C0 already hold the element above, at and below the arriving prio."""
    e = np.arange(1000, 1300, dtype=np.uint32)
    arriving = (e % 3).astype(np.int8) - 1  # -1, 0, 1 against a stored 0
    c0, m0 = (e.copy(), np.zeros(300, np.int8)), (e.copy(), np.zeros(300, np.int8))
    cs, ms, _ = _check(gpu, c0, m0, [(IN, e, arriving)])
    assert cs.Len() == 300 and ms.Len() == 300
    assert sorted(set(ms.to_dict().values())) == [0, 1] and list(ms.to_dict().values()).count(1) == 100


@pytest.mark.parametrize("c_nil,m_nil", [(False, False), (False, True), (True, False), (True, True)])
def test_nil_receivers(gpu, c_nil, m_nil):
    rng = np.random.default_rng(5)
    U = 400
    c0 = None if c_nil else _rand_set(rng, 100, U)
    m0 = None if m_nil else _rand_set(rng, 150, U)
    segs = [_rand_seg(rng, MS, 90, U), _rand_seg(rng, IN, 0, U), _rand_seg(rng, IN, 70, U), _rand_seg(rng, MS, 0, U)]
    cs, ms, _ = _check(gpu, c0, m0, segs)
    assert not cs.is_nil() and not ms.is_nil()
    # only MAXSIGNAL segments: a nil corpusSignal stays nil; only empty ones: both stay as they were
    cs, ms, _ = _check(gpu, c0, m0, [segs[0], segs[3]])
    assert cs.is_nil() == c_nil and not ms.is_nil()
    cs, ms, st = _check(gpu, c0, m0, [segs[1], segs[3]])
    assert cs.is_nil() == c_nil and ms.is_nil() == m_nil and st == (0, 0, 0, 0)
    cs, ms, _ = _check(gpu, c0, m0, [])
    assert cs.is_nil() == c_nil and ms.is_nil() == m_nil


def test_reversed_segment_order_gives_identical_tables(gpu):
    rng = np.random.default_rng(29)
    U = 5000
    segs = [_rand_seg(rng, (IN, MS)[i % 2], n, U) for i, n in enumerate([300, 2 * T + 3, 17, T, 1, 900])]
    c0, m0 = _rand_set(rng, 700, U), _rand_set(rng, 900, U)
    a = _check(gpu, c0, m0, segs)
    b = _check(gpu, c0, m0, segs[::-1])
    # (as contents: which slot of a probe chain a key takes depends on the order
    # the workgroups ran in, so the slot words themselves are not compared)
    assert _same(_pairs(a[0]), _pairs(b[0])) and _same(_pairs(a[1]), _pairs(b[1]))
    assert _rules_differ(c0, m0, segs)


@pytest.mark.parametrize("case", ["reversed", "past_end", "kind", "aliased"])
def test_errors_leave_both_sets(gpu, case):
    """SYZSIG_EINVAL before anything is committed: both sets bit-identical to their clones."""
    import torch

    from syzkaller_amd._lib import SYZSIG_EINVAL, SyzsigError

    rng = np.random.default_rng(31)
    U = 600
    segs = [_rand_seg(rng, IN, 200, U), _rand_seg(rng, MS, T + 5, U), _rand_seg(rng, IN, 50, U)]
    cs, ms = _dev_sets(gpu, _rand_set(rng, 100, U), _rand_set(rng, 200, U))
    cs0, ms0 = cs.clone(), ms.clone()
    off, kind, elems, prios = _tensors(gpu, segs)
    if case == "reversed":
        off[1], off[2] = off[2].clone(), off[1].clone()
    elif case == "past_end":
        off[3] += 1
    elif case == "kind":
        kind[1] = 2
    with pytest.raises(SyzsigError) as ei:
        gpu.poll_res(off, kind, elems, prios, ms if case == "aliased" else cs, ms)
    torch.cuda.synchronize()
    assert ei.value.code == SYZSIG_EINVAL
    assert cs.equal(cs0) and ms.equal(ms0) and cs.Len() == cs0.Len() and ms.Len() == ms0.Len()
    # nil receivers stay nil on the same errors
    if case != "aliased":
        ncs, nms = _dev_sets(gpu, None, None)
        with pytest.raises(SyzsigError):
            gpu.poll_res(off, kind, elems, prios, ncs, nms)
        assert ncs.is_nil() and nms.is_nil()


def test_chain_manager_poll_then_fuzzer_poll_res(gpu):
    """signal.manager_poll over a few fuzzers, then fuzzer 0's reply Serial and
    two inputs' Serials through signal.fuzzer_poll_res, against the restatement."""
    from syzkaller_amd import signal as S

    rng = np.random.default_rng(37)
    F, U = 3, 2000
    mgr = S.Serial(*_rand_set(rng, 600, U)).Deserialize(gpu.eng)
    new_max = [S.Signal(None, gpu.eng) for _ in range(F)]
    polls = [(f, S.Serial(*_rand_seg(rng, MS, 250, U)[1:])) for f in (1, 2, 0)]
    replies = S.manager_poll(mgr, new_max, polls, gpu.eng)
    reply0 = replies[2]  # fuzzer 0 polled last: it is told what 1 and 2 found
    assert reply0.Elems.size > 0
    inputs = [S.Serial(*_rand_seg(rng, IN, n, U)[1:]) for n in (180, T + 9)]
    c0, m0 = _rand_set(rng, 300, U), _rand_set(rng, 400, U)
    cs, ms = _dev_sets(gpu, c0, m0)
    S.fuzzer_poll_res(cs, ms, reply0, inputs, gpu.eng)
    assert S.poll_res_stats(gpu.eng)[:2] == (2, 1)
    ocs, oms = _ora_sets(c0, m0)
    R.poll_res(ocs, oms, [(MS, reply0.Elems, reply0.Prios)] + [(IN, s.Elems, s.Prios) for s in inputs])
    assert _same(_pairs(cs), _pairs(ocs)) and _same(_pairs(ms), _pairs(oms))
    # a nil pair and an empty reply: nothing is allocated
    ncs, nms = _dev_sets(gpu, None, None)
    S.fuzzer_poll_res(ncs, nms, S.Serial(), [S.Serial()], gpu.eng)
    assert ncs.is_nil() and nms.is_nil()
    S.fuzzer_poll_res(ncs, nms, None, [], gpu.eng)
    assert ncs.is_nil() and nms.is_nil()
