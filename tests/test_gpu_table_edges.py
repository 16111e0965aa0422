"""GPU: the open-addressed signal table (csrc/table.hip, tbl_* in
csrc/internal.h) in the states uniformly random keys never produce -- probe
chains longer than a bucket, chains that wrap from the last bucket to bucket 0,
one chain holding tens of thousands of keys, rehashes that carry such chains,
the exact load at which a table grows -- plus the state operations (clone,
copy_from, clear, reserve, equal, a capped Serialize), the value edges of
elements and prios, and the set algebra on a table that a triage path has just
written.  Everything is compared exactly with the oracle's Signal and Cover."""
import ctypes
import time

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import kat_runner as KR
from tests import table_keys as TK

pytestmark = pytest.mark.gpu

I8 = (-128, 128)


def buckets_for(n):
    """csrc/table.hip buckets_for: a power of two, load 0.5 at n entries."""
    want, b = int(n / (TK.BUCKET_SLOTS * 0.5)) + 1, 2
    while b < want:
        b <<= 1
    return b


def slots_for(n):
    return buckets_for(n) * TK.BUCKET_SLOTS


def same(g, o):
    """A device Signal against the oracle's: nil-ness, dict and Len."""
    assert KR.as_result(g) == KR.as_result(o)
    assert g.Len() == o.Len()


def rand_set(rng, n, lo=I8[0], hi=I8[1]):
    e = np.unique(rng.integers(0, 1 << 32, n + n // 8 + 8, dtype=np.uint64).astype(np.uint32))
    e = rng.permutation(e)[:n]
    return e, rng.integers(lo, hi, e.size).astype(np.int8)


def both(S, eng, e, p):
    return S.Serial(e, p).Deserialize(eng), O.deserialize(e, p)


@pytest.fixture(scope="module")
def uniform5000():
    """The uniformly random partner set of sections A and B (never changed)."""
    return rand_set(np.random.default_rng(5000), 5000)


# ---------------------------------------------------------------- A. clusters and wrap-around

def cluster_keys(kind, n):
    if kind == "last":
        return TK.hot_last(n)
    if kind == "first":
        return TK.hot_first(n)
    return np.concatenate([TK.hot_last(n), TK.hot_first(n)])


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17, 3000])
@pytest.mark.parametrize("kind", ["last", "first", "union"])
def test_cluster_algebra_vs_oracle(gpu, uniform5000, kind, n):
    """One probe chain of n (or 2n) keys at the table's last bucket, at bucket
    0, or wrapping from the one into the other, through every operation."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    rng = np.random.default_rng(1000 * n + len(kind))
    ce = rng.permutation(cluster_keys(kind, n))
    cp = rng.integers(*I8, ce.size).astype(np.int8)
    if ce.size >= 4:
        cp[:4] = [-128, 127, 0, -1]
    gc, oc = both(S, eng, ce, cp)
    same(gc, oc)
    assert gc.capacity() == slots_for(ce.size)
    # the uniform partner, alone and with half of the cluster in it at other prios
    ue, up = uniform5000
    half = ce[::2]
    partners = [(ue, up), (np.concatenate([ue, half]),
                           np.concatenate([up, rng.integers(*I8, half.size).astype(np.int8)]))]
    for pe, pp in partners:
        gu, ou = both(S, eng, pe, pp)
        same(gc.Diff(gu), oc.Diff(ou))
        same(gu.Diff(gc), ou.Diff(oc))
        same(gc.Intersection(gu), oc.Intersection(ou))
        same(gu.Intersection(gc), ou.Intersection(oc))
        for prio in (0, 0x80, int(rng.integers(0, 256))):
            same(gc.DiffRaw(pe, prio), oc.DiffRaw(pe, prio))
            same(gu.DiffRaw(ce, prio), ou.DiffRaw(ce, prio))
        a, oa = gc.clone(), O.deserialize(ce, cp)
        a.Merge(gu)
        oa.Merge(ou)
        same(a, oa)
        b, ob = gu.clone(), O.deserialize(pe, pp)
        b.Merge(gc)
        ob.Merge(oc)
        same(b, ob)
    # FromRaw, with every key twice
    raw = rng.permutation(np.concatenate([ce, ce]))
    for prio in (3, 0x80, 0xFF):
        same(S.FromRaw(raw, prio, eng), O.from_raw(raw, prio))
    # Cover.Merge: the cluster into a nil cover, then the uniform keys (grows it)
    gcov, ocov = S.Cover(eng), O.OCover()
    for r in (raw, ue, ce):
        gcov.Merge(r)
        ocov.Merge(r)
        assert sorted(gcov.Serialize().tolist()) == ocov.Serialize() and len(gcov) == len(ocov.Serialize())
    # Serialize round trip and the batch Serialize
    ser = gc.Serialize()
    assert ser.Elems.size == ser.Prios.size == gc.Len()
    same(ser.Deserialize(eng), oc)
    gu = S.Serial(ue, up).Deserialize(eng)
    many = S.serialize_many([gc, None, gu, gc], eng)
    want = [oc.to_dict(), {}, dict(zip(ue.tolist(), up.tolist())), oc.to_dict()]
    for m, w in zip(many, want):
        assert m.Elems.size == len(w) and dict(zip(m.Elems.tolist(), m.Prios.tolist())) == w


@pytest.mark.parametrize("hint", [0, 100, 10 ** 5])
@pytest.mark.parametrize("n", [9, 3000])
def test_cluster_merge_into_receiver_through_rehashes(gpu, uniform5000, hint, n):
    """The wrapping cluster merged into make(hint) -- 2 buckets (the least), 128
    and 2^17 -- then uniform sets merged on top: every growth re-places the
    wrapped chain (k_rehash), in tables of every size on the way."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    rng = np.random.default_rng(n + hint)
    ce = cluster_keys("union", n)
    cp = rng.integers(*I8, ce.size).astype(np.int8)
    recv, orecv = S.Signal.make(hint, eng), O.OSig()
    assert recv.capacity() == slots_for(hint)
    ue, up = uniform5000
    caps = [recv.capacity()]
    for e, p in [(ce, cp), (ue[:40], up[:40]), (ue[40:600], up[40:600]), (ue[600:], up[600:]),
                 (ce, np.full(ce.size, 127, np.int8))]:
        g, o = both(S, eng, e, p)
        recv.Merge(g)
        orecv.Merge(o)
        assert recv.to_dict() == orecv.to_dict() and recv.Len() == orecv.Len()
        caps.append(recv.capacity())
    assert caps == sorted(caps)
    assert (len(set(caps)) >= 3) == (hint < 10 ** 5), caps  # several rehashes, or none in the roomy table
    same(recv.Serialize().Deserialize(eng), orecv)


# ---------------------------------------------------------------- B. one chain past 4096 buckets

BIG = [32768 - 8, 40000]


@pytest.fixture(scope="module")
def big_cluster():
    """hot_last(n) with full-range prios, its oracle Signal (never changed)."""
    out = {}
    for n in BIG:
        rng = np.random.default_rng(n)
        e = rng.permutation(TK.hot_last(n))
        p = rng.integers(*I8, n).astype(np.int8)
        out[n] = (e, p, O.deserialize(e, p))
    return out


def timed(what, f):
    t0 = time.perf_counter()
    r = f()
    print(f"{what}: {time.perf_counter() - t0:.3f} s")
    return r


@pytest.mark.parametrize("op", ["deserialize", "from_raw", "diff_raw_empty", "merge_make", "merge_holding_5000",
                                "cover_merge"])
@pytest.mark.parametrize("n", BIG)
def test_one_home_bucket_past_4096_buckets(gpu, big_cluster, uniform5000, n, op):
    """n keys with ONE home bucket, in tables of 2^16 and 2^17 buckets: a probe
    chain of n / 2 buckets, far past the 4096 an insert once gave up after.  The
    contract: an insert probes the whole table, the writers
    reserve room first, so every operation succeeds and equals the oracle."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    e, p, oc = big_cluster[n]
    assert (TK.home_bucket(e, buckets_for(n)) == buckets_for(n) - 1).all() and buckets_for(n) > 4096
    if op == "deserialize":
        g = timed(op, lambda: S.Serial(e, p).Deserialize(eng))
        assert g.capacity() == slots_for(n)
        same(g, oc)
        same(g.Serialize().Deserialize(eng), oc)
    elif op == "from_raw":
        same(timed(op, lambda: S.FromRaw(e, 0x80, eng)), O.from_raw(e, 0x80))
    elif op == "diff_raw_empty":
        same(timed(op, lambda: S.Signal.make(0, eng).DiffRaw(e, 0xFF)), O.OSig().DiffRaw(e, 0xFF))
    elif op == "cover_merge":
        gcov, ocov = S.Cover(eng), O.OCover()
        timed(op, lambda: gcov.Merge(e))
        ocov.Merge(e)
        assert sorted(gcov.Serialize().tolist()) == ocov.Serialize() and len(gcov) == n
    else:
        src = S.Serial(e, p).Deserialize(eng)
        recv, orecv = S.Signal.make(10 ** 5, eng), O.OSig()
        if op == "merge_holding_5000":
            g, o = both(S, eng, *uniform5000)
            recv.Merge(g)
            orecv.Merge(o)
        cap = recv.capacity()
        assert cap == slots_for(10 ** 5) and cap // TK.BUCKET_SLOTS > 4096
        timed(op, lambda: recv.Merge(src))
        orecv.Merge(oc)
        assert recv.capacity() == cap  # 45000 of 2^18 slots: no growth, the chain stands in this table
        assert recv.Len() == orecv.Len() == len(recv.Serialize().Elems)
        assert recv.to_dict() == orecv.to_dict()


# ---------------------------------------------------------------- C. growth boundary and state operations

def test_growth_exactly_at_the_load_bound(gpu):
    """Merge grows a table when len + extra exceeds 0.75 of its slots, not at
    it, and then to buckets_for(len + extra); hot_last(100) rides through."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    rng = np.random.default_rng(75)
    recv, orecv = S.Signal.make(100, eng), O.OSig()
    cap = recv.capacity()
    assert cap == slots_for(100) == 256
    bound = int(0.75 * cap)
    assert bound == 0.75 * cap
    re_, rp = rand_set(rng, bound)
    parts = [(TK.hot_last(100), rng.integers(*I8, 100).astype(np.int8)),  # well inside
             (re_[:bound - 100], rp[:bound - 100]),                        # lands exactly on the bound
             (re_[bound - 100:bound - 99], rp[bound - 100:bound - 99])]    # one past it
    want_caps = [cap, cap, slots_for(bound + 1)]
    assert want_caps[2] > cap
    for (e, p), wc in zip(parts, want_caps):
        g, o = both(S, eng, e, p)
        recv.Merge(g)
        orecv.Merge(o)
        assert recv.capacity() == wc
        assert recv.to_dict() == orecv.to_dict() and recv.Len() == orecv.Len()
    assert recv.Len() == bound + 1


def test_reserve(gpu):
    from syzkaller_amd import signal as S

    eng = gpu.eng
    rng = np.random.default_rng(76)
    e = np.concatenate([TK.hot_last(30), TK.hot_first(30), rand_set(rng, 240)[0]])
    s, o = both(S, eng, e, rng.integers(*I8, e.size).astype(np.int8))
    cap, d = s.capacity(), o.to_dict()
    snap = s.clone()
    s.reserve(0)
    assert s.capacity() == cap and s.equal(snap)
    bound = int(0.75 * cap)
    s.reserve(bound - s.Len())  # up to the bound: nothing moves
    assert s.capacity() == cap and s.equal(snap)
    s.reserve(bound - s.Len() + 1)
    assert s.capacity() == slots_for(bound + 1) > cap
    assert s.to_dict() == d and s.Len() == len(d)
    s.reserve(10 ** 5)
    assert s.capacity() == slots_for(len(d) + 10 ** 5)
    assert s.to_dict() == d and s.Len() == len(d)


def test_clone_equal_copy_from_clear(gpu):
    from syzkaller_amd import signal as S
    from syzkaller_amd._lib import SyzsigError

    eng = gpu.eng
    rng = np.random.default_rng(77)
    e = np.concatenate([TK.hot_last(50), TK.hot_first(50), rand_set(rng, 900)[0]])
    p = rng.integers(-128, 127, e.size).astype(np.int8)  # below 127: every prio can be raised
    s, o = both(S, eng, e, p)
    d = o.to_dict()
    c = s.clone()
    assert c.equal(s) and s.equal(c) and c.capacity() == s.capacity()
    assert c.to_dict() == d and c.Len() == len(d)
    assert S.Signal(None, eng).clone().is_nil()
    # one prio raised: same Len, not equal
    c.Merge(S.Serial(e[7:8], p[7:8] + 1).Deserialize(eng))
    assert c.Len() == s.Len() and not c.equal(s)
    assert c.to_dict() == {**d, int(e[7]): int(p[7]) + 1}
    c.copy_from(s)
    assert c.equal(s) and c.to_dict() == d
    # one element inserted: not equal
    extra = np.array([0x13572468], np.uint32)
    assert int(extra[0]) not in d
    c.Merge(S.Serial(extra, [0]).Deserialize(eng))
    assert c.Len() == s.Len() + 1 and c.capacity() == s.capacity() and not c.equal(s)
    c.copy_from(s)
    assert c.equal(s) and c.Len() == s.Len() and c.to_dict() == d
    # another capacity: refused, the destination as it was
    other = S.Signal.make(10 * e.size, eng)
    other.Merge(S.Serial(e[:10], p[:10]).Deserialize(eng))
    before = other.to_dict()
    assert other.capacity() != s.capacity() and not other.equal(s)
    with pytest.raises(SyzsigError):
        other.copy_from(s)
    assert other.to_dict() == before and other.Len() == 10
    # clear: empty, same table, usable
    cap = c.capacity()
    c.clear()
    assert c.Len() == 0 and c.Serialize().Elems.size == 0 and c.to_dict() == {} and c.capacity() == cap
    assert not c.is_nil() and not c.equal(s)
    e2 = np.concatenate([e[:300], TK.hot_last(20, skip=50)])
    p2 = rng.integers(*I8, e2.size).astype(np.int8)
    g2, o2 = both(S, eng, e2, p2)
    c.Merge(g2)
    assert c.to_dict() == o2.to_dict() and c.Len() == o2.Len() and c.capacity() == cap


def test_serialize_capped_output(gpu):
    """syzsig_serialize with less room than Len: n_out is Len, exactly cap
    entries are written, each a distinct entry of the set, nothing after them.
    The set's live slots lie in a few of the 2048 chunks of a 2^19-slot table
    (k_count_live mostly counts zero, k_scan_counts takes two steps)."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    rng = np.random.default_rng(78)
    hint = 200_000
    nb = buckets_for(hint)
    assert nb * TK.BUCKET_SLOTS == 1 << 19
    e = rng.permutation(TK.hot_at(nb, nb // 3, 3000))
    p = rng.integers(-128, 50, e.size).astype(np.int8)
    s = S.Signal.make(hint, eng)
    s.Merge(S.Serial(e, p).Deserialize(eng))
    assert s.capacity() == 1 << 19
    # The full Serialize comes first: the library's output scratch then holds Len
    # entries, so a writer that ignored cap would stay inside it and show below
    # as a wrong entry.
    d = s.to_dict()
    n = s.Len()
    assert d == dict(zip(e.tolist(), p.tolist())) and n == 3000
    SE, SP = 0xDEADBEEF, 0x55
    assert SE not in d and SP not in d.values()
    for cap in (0, 1, n // 2, n - 1):
        elems = np.full(n + 8, SE, np.uint32)
        prios = np.full(n + 8, SP, np.int8)
        out = ctypes.c_uint64(12345)
        rc = eng.L.syzsig_serialize(eng.h, s.handle, ctypes.c_void_p(elems.ctypes.data),
                                    ctypes.c_void_p(prios.ctypes.data), cap, ctypes.byref(out))
        assert rc == 0 and out.value == n
        assert (elems[cap:] == SE).all() and (prios[cap:] == SP).all()
        got = list(zip(elems[:cap].tolist(), prios[:cap].tolist()))
        assert len(set(x for x, _ in got)) == cap
        bad = [(x, y) for x, y in got if d.get(x, None) != y]
        assert not bad, (cap, bad[:5])


# ---------------------------------------------------------------- D. value edges

# (fmix32_inv(0) is 0 again: six distinct elements)
EDGE_ELEMS = np.unique(np.concatenate([np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32),
                                       TK.fmix32_inv_np(np.array([0, 0xFFFFFFFF], np.uint32))]))
EDGE_PRIOS = [-128, -1, 0, 1, 127]
EDGE_BYTES = [0, 1, 0x7F, 0x80, 0xFF]


def test_prio_pairs_signed_order(gpu):
    """Every (prio in s, prio in s1) pair on every edge element: Diff keeps on
    >=, Intersection on s1 >= s, Merge takes the signed max (127 over -128)."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    pairs = [(a, b) for a in EDGE_PRIOS for b in EDGE_PRIOS]
    fill = rand_set(np.random.default_rng(79), len(pairs) - EDGE_ELEMS.size)[0]
    keys = np.concatenate([EDGE_ELEMS, fill])
    assert np.unique(keys).size == len(pairs) == 25
    for rot in range(len(pairs)):
        pa = np.array([pairs[(k + rot) % 25][0] for k in range(25)], np.int8)
        pb = np.array([pairs[(k + rot) % 25][1] for k in range(25)], np.int8)
        gs, os_ = both(S, eng, keys, pa)
        g1, o1 = both(S, eng, keys, pb)
        da, db = dict(zip(keys.tolist(), pa.tolist())), dict(zip(keys.tolist(), pb.tolist()))
        diff = gs.Diff(g1)
        same(diff, os_.Diff(o1))
        assert (diff.to_dict() if not diff.is_nil() else {}) == {k: v for k, v in db.items() if not da[k] >= v}
        inter = gs.Intersection(g1)
        same(inter, os_.Intersection(o1))
        assert inter.to_dict() == {k: v for k, v in da.items() if db[k] >= v}
        gs.Merge(g1)
        os_.Merge(o1)
        same(gs, os_)
        assert gs.to_dict() == {k: max(v, db[k]) for k, v in da.items()}


def test_raw_prio_bytes(gpu):
    """DiffRaw and FromRaw take the prio as a byte and compare it as int8."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    raw = np.concatenate([EDGE_ELEMS, np.array([2, 0xFFFFFFFE], np.uint32), EDGE_ELEMS[:3]])
    for byte in EDGE_BYTES:
        sp = int(np.uint8(byte).view(np.int8))
        f = S.FromRaw(raw, byte, eng)
        same(f, O.from_raw(raw, byte))
        assert f.to_dict() == {int(k): sp for k in raw}
        for rot in range(len(EDGE_PRIOS)):
            p = np.array([EDGE_PRIOS[(k + rot) % 5] for k in range(EDGE_ELEMS.size)], np.int8)
            gs, os_ = both(S, eng, EDGE_ELEMS, p)
            have = dict(zip(EDGE_ELEMS.tolist(), p.tolist()))
            r = gs.DiffRaw(raw, byte)
            same(r, os_.DiffRaw(raw, byte))
            assert (r.to_dict() if not r.is_nil() else {}) == {int(k): sp for k in raw
                                                                if not (int(k) in have and have[int(k)] >= sp)}


def test_element_zero_at_lowest_prio_is_live(gpu):
    """Element 0 at prio -128 has every value bit of its slot word zero: only
    the state bits tell it from an empty slot."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    z = np.zeros(1, np.uint32)
    for s in (S.Serial(z, [-128]).Deserialize(eng), S.FromRaw(z, 0x80, eng),
              S.Signal.make(0, eng).DiffRaw(z, 0x80)):
        assert s.Len() == 1 and s.to_dict() == {0: -128}
        ser = s.Serialize()
        assert ser.Elems.tolist() == [0] and ser.Prios.tolist() == [-128]
        recv = S.Signal.make(0, eng)
        recv.Merge(s)
        assert recv.Len() == 1 and recv.to_dict() == {0: -128}
        assert s.Diff(recv).is_nil() and recv.Intersection(s).to_dict() == {0: -128}
        c = S.Cover(eng)
        c.Merge(z)
        assert c.Serialize().tolist() == [0]


def test_one_element_repeated(gpu):
    from syzkaller_amd import signal as S

    eng = gpu.eng
    rng = np.random.default_rng(80)
    for elem in (0, 0xFFFFFFFF, int(TK.hot_last(1)[0])):
        raw = np.full(10 ** 5, elem, np.uint32)
        f = S.FromRaw(raw, 0x80, eng)
        assert f.Len() == 1 and f.to_dict() == {elem: -128}
        r = S.Signal.make(0, eng).DiffRaw(raw, 0x7F)
        assert r.Len() == 1 and r.to_dict() == {elem: 127}
        p = rng.integers(*I8, raw.size).astype(np.int8)
        p[-1] = -77  # the last one wins, whatever came before
        g = S.Serial(raw, p).Deserialize(eng)
        same(g, O.deserialize(raw, p))
        assert g.Len() == 1 and g.to_dict() == {elem: -77}


# ---------------------------------------------------------------- E. algebra on a table that triage has written

STD_PRIOS = [0, 1, 2, 3]
MANY_PRIOS = [0, 1, 2, 3, 7, 127, 128, 200, 255]  # as bytes; int8 order, more than 4 levels: several runs


def _i8(byte_list, rng, n):
    return rng.choice(np.array(byte_list, np.uint8), n).view(np.int8)


def edge_m0(rng, prios, nrand=3000):
    e = np.concatenate([TK.hot_last(20), TK.hot_first(20), rand_set(rng, nrand)[0]])
    assert np.unique(e).size == e.size
    return e, _i8(prios, rng, e.size)


def edge_batch(rng, known, prios, skip):
    """Calls over known elements (so: lower, equal and higher prio than the
    table's), new ones homing to the last bucket and to bucket 0, and random
    new ones.  Every element appears, and at most once per call."""
    pool = np.unique(np.concatenate([rng.choice(known, min(1500, known.size), replace=False), TK.hot_last(40),
                                     TK.hot_first(40), TK.hot_last(20, skip=skip), TK.hot_first(20, skip=skip),
                                     rand_set(rng, 800)[0]]))
    pool = rng.permutation(pool)
    calls = [pool[i:i + 25] for i in range(0, pool.size, 25)]
    calls += [rng.choice(pool, int(rng.integers(1, 60)), replace=False) for _ in range(60)]
    calls.append(np.empty(0, np.uint32))
    calls = [calls[i] for i in rng.permutation(len(calls))]
    hcnt = np.array([c.size for c in calls], np.uint32)
    hcs = np.zeros(len(calls), np.uint64)
    hcs[1:] = np.cumsum(hcnt[:-1].astype(np.uint64))
    hs = np.concatenate(calls).astype(np.uint32)
    hprio = rng.choice(np.array(prios, np.uint8), len(calls))
    return hs, hcs, hcnt, hprio, pool


def run_writer(gpu, mode, ms, ns, batch):
    """One batch through one writer of maxSignal; returns the per-record new
    flags (None where the path computes none) and call_new (None: records mode)."""
    hs, hcs, hcnt, hprio, _ = batch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)  # noqa: E731
    nrec = hs.size
    if mode == "records":
        serial = np.repeat(np.arange(hcnt.size, dtype=np.uint64), hcnt)
        lvl = np.repeat(hprio.astype(np.uint64), hcnt)
        rec = (hs.astype(np.uint64) << np.uint64(32)) | (lvl << np.uint64(24)) | serial
        perm = np.random.default_rng(nrec).permutation(nrec)
        flags = torch.zeros(nrec, dtype=torch.uint8, device=gpu.dev)
        gpu.triage_records(ms, ns, t(rec[perm], np.int64), STD_PRIOS, flags)
        new = np.zeros(nrec, np.uint8)
        new[perm] = flags.cpu().numpy()
        return new, None
    want_bits = mode != "agg_one_sync"
    bits, cnew, st = gpu.triage(ms, ns, t(hs, np.int32), t(hcs, np.int64), t(hcnt, np.int32), t(hprio, np.uint8),
                                want_bits=want_bits)
    assert (st["parts"] > 0) == mode.startswith("agg"), st
    new = None
    if want_bits:
        new = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:nrec]
    return new, cnew.cpu().numpy()


def check_written_table(gpu, g, o, others, rng):
    """The set algebra on a table a triage path wrote, against the oracle's."""
    from syzkaller_amd import signal as S

    eng = gpu.eng
    d = o.to_dict()
    assert g.to_dict() == d
    assert g.Len() == o.Len() == len(d)
    assert len(g.Serialize().Elems) == g.Len()
    ke = np.array(sorted(d), np.uint32)
    # every element one prio up: a word compared with leftover bits above the prio would lose this
    kp = np.array([min(d[int(k)] + 1, 127) for k in ke], np.int8)
    c, oc = g.clone(), O.deserialize(*o.Serialize())
    assert c.equal(g)
    # in pieces that fit under the growth bound: merged into the slot words triage
    # left, not into a rehashed copy (a table too close to the bound grows anyway)
    cap = c.capacity()
    room = int(0.75 * cap) - c.Len()
    step = max(min(room, 1 + ke.size // 4), 1 + ke.size // 64)
    for i in range(0, ke.size, step):
        gi, oi = both(S, eng, ke[i:i + step], kp[i:i + step])
        c.Merge(gi)
        oc.Merge(oi)
    assert c.capacity() == cap or step > room
    assert c.to_dict() == oc.to_dict() == dict(zip(ke.tolist(), kp.tolist())) and c.Len() == oc.Len()
    # full-range prios over the same elements and the batch's: a slot left marked "absent" reads as -128
    te = np.unique(np.concatenate([ke, others]))
    tp = rng.integers(*I8, te.size).astype(np.int8)
    tp[::3] = -128
    gt, ot = both(S, eng, te, tp)
    same(g.Diff(gt), o.Diff(ot))
    same(gt.Diff(g), ot.Diff(o))
    same(g.Intersection(gt), o.Intersection(ot))
    same(gt.Intersection(g), ot.Intersection(o))
    for byte in (0x80, 0, 2, 0x7F):
        same(g.DiffRaw(te, byte), o.DiffRaw(te, byte))
    # growth and clone keep the contents
    c2 = g.clone()
    c2.reserve(int(0.75 * c2.capacity()) - c2.Len() + 1)
    assert c2.capacity() > g.capacity()
    assert c2.to_dict() == d and c2.Len() == len(d)
    assert g.clone().to_dict() == d


WRITERS = [("probe", STD_PRIOS), ("probe", MANY_PRIOS), ("probe_restart", STD_PRIOS), ("agg", STD_PRIOS),
           ("agg", MANY_PRIOS), ("agg_defer", STD_PRIOS), ("agg_defer", MANY_PRIOS), ("agg_one_sync", STD_PRIOS),
           ("records", STD_PRIOS)]


@pytest.mark.parametrize("mode,prios", WRITERS, ids=[f"{m}-{len(p)}prios" for m, p in WRITERS])
def test_algebra_after_triage_wrote_the_table(gpu, mode, prios):
    """Two batches through one writer of maxSignal -- the probe path (also from
    a table so small that the run restarts on a bigger one), the aggregation
    path at 8 partitions with the slice-exclusive finalize (new elements homing
    to the last bucket leave the last slice and wrap into slice 0) and with
    every walk deferred, the one-sync run, records mode -- and after each the
    algebra on maxSignal and newSignal."""
    from syzkaller_amd import signal as S
    from syzkaller_amd._lib import SYZSIG_DEBUG_FIN_DEFER

    eng = gpu.eng
    rng = np.random.default_rng(len(mode) * 100 + len(prios))
    restart = mode == "probe_restart"
    m0e, m0p = edge_m0(rng, prios, nrand=60 if restart else 3000)
    # a roomy maxSignal: neither the batches nor the Merge in check_written_table
    # rehash it, so what a writer leaves in the slot words stays there
    ms = S.Signal.make(0 if restart else 8 * m0e.size, eng)
    ms.Merge(S.Serial(m0e, m0p).Deserialize(eng))
    ns = S.Signal(None, eng)
    oms, ons = O.deserialize(m0e, m0p), O.OSig()
    eng.set_agg(2 if mode.startswith("agg") else 0, 8 if mode.startswith("agg") else 0)
    eng.set_debug(SYZSIG_DEBUG_FIN_DEFER if mode == "agg_defer" else 0)
    try:
        for round_ in range(2):
            batch = edge_batch(rng, np.array(sorted(oms.to_dict()), np.uint32), prios, skip=40 + 20 * round_)
            hs, hcs, hcnt, hprio, pool = batch
            cap = ms.capacity()
            new, cnew = run_writer(gpu, mode.replace("probe_restart", "probe"), ms, ns, batch)
            if not restart:
                assert ms.capacity() == cap
            elif round_ == 0:
                assert ms.capacity() > cap  # the table filled up: rehashed mid-run, the run restarted
            me, mp = oms.Serialize()
            oms, ons, obits, ocnew = O.triage_batch(me, mp, hs, hcs, hcnt, hprio,
                                                    ons.Serialize() if round_ else None)
            if new is not None:
                np.testing.assert_array_equal(new, np.unpackbits(obits.view(np.uint8), bitorder="little")[:hs.size])
            if cnew is not None:
                np.testing.assert_array_equal(cnew, ocnew)
            assert ons.Len() > 0
            check_written_table(gpu, ms, oms, pool, rng)
            check_written_table(gpu, ns, ons, pool, rng)
    finally:
        eng.set_agg(1, 0)
        eng.set_debug(0)


def test_failed_run_leaves_no_hints_behind(gpu):
    """A records-mode run that fails on device (a record with a level the call
    did not declare) has already put run hints and absent markers into
    maxSignal; the same-size rehash that reports the error must take both out.
    The next run carries the same elements in the reverse serial order, so a
    surviving hint would settle records that are new; and Merge, which compares
    whole slot words, would lose a higher prio to a word with hint bits."""
    from syzkaller_amd import signal as S
    from syzkaller_amd._lib import SyzsigError

    eng = gpu.eng
    rng = np.random.default_rng(81)
    m0e = np.concatenate([TK.hot_last(20), TK.hot_first(20), rand_set(rng, 2000)[0]])
    m0p = np.full(m0e.size, -5, np.int8)  # below every level: each element's first record is new
    ms, oms = both(S, eng, m0e, m0p)
    ns = S.Signal(None, eng)
    ncalls, per = 1024, 3  # serials past 255: hints compare serials in units of 256
    idx = (rng.integers(0, m0e.size, ncalls)[:, None] + np.arange(per)[None, :] * 7919) % m0e.size
    sigs = m0e[idx.ravel()]
    lvl = rng.integers(0, 3, ncalls).astype(np.uint64)
    serial = np.repeat(np.arange(ncalls, dtype=np.uint64), per)

    def recs(ser):
        return (sigs.astype(np.uint64) << np.uint64(32)) | (np.repeat(lvl, per) << np.uint64(24)) | ser

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(gpu.dev)  # noqa: E731
    flags = torch.zeros(sigs.size, dtype=torch.uint8, device=gpu.dev)
    bad = recs(serial)
    bad[-1] |= np.uint64(3 << 24)  # level 3 of 3
    perm = rng.permutation(sigs.size)
    eng.set_agg(0, 0)
    try:
        cap = ms.capacity()
        with pytest.raises(SyzsigError):
            gpu.triage_records(ms, ns, t(bad[perm]), [0, 1, 2], flags)
        assert ms.to_dict() == oms.to_dict() and ms.Len() == oms.Len() and ms.capacity() == cap
        assert ns.Len() == 0
        # Merge on the slot words the failed run left (no growth: 2040 + 500 of 4096 slots)
        c, oc = ms.clone(), O.deserialize(m0e, m0p)
        up, oup = both(S, eng, m0e[:500], np.full(500, -4, np.int8))
        c.Merge(up)
        oc.Merge(oup)
        assert c.capacity() == cap and c.to_dict() == oc.to_dict()
        # the same calls in reverse order
        gpu.triage_records(ms, ns, t(recs(ncalls - 1 - serial)[perm]), [0, 1, 2], flags)
    finally:
        eng.set_agg(1, 0)
    rev = np.arange(ncalls)[::-1]
    hs = m0e[idx[rev].ravel()]
    hcs = np.arange(ncalls, dtype=np.uint64) * per
    oms2, ons2, obits, _ = O.triage_batch(m0e, m0p, hs, hcs, np.full(ncalls, per, np.uint32), lvl[rev].astype(np.uint8))
    # record r of the device order is call (ncalls - 1 - r // per) of the oracle's, same place in the call
    onew = np.unpackbits(obits.view(np.uint8), bitorder="little")[:hs.size].reshape(ncalls, per)[rev].ravel()
    np.testing.assert_array_equal(flags.cpu().numpy(), onew[perm])
    assert onew.sum() > 0
    check_written_table(gpu, ms, oms2, m0e, rng)
    check_written_table(gpu, ns, ons2, m0e, rng)
