"""GPU: pkg/db's write side -- syzsig_deflate_dev, syzsig_db_records_dev,
syzsig_db_apply_dev and syzkaller_amd.db.DB's save / delete / flush / compact --
against syzsig_deflate_host (the same compressor on the CPU), zlib,
syzsig_inflate_dev and tests/dbw_ref.py (pkg/db/db.go:55-175 restated).  No
expected value comes from the device; output buffers are pre-filled so that an
unwritten or overwritten byte shows; the paths taken are asserted from
syzsig_deflate_stats."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, db, hashing, progtext
from tests import db_ref as R
from tests import dbw_cases as C
from tests import dbw_ref as W
from tests.test_dbw_ref_cpu import deflate_inputs, host_streams, stored_bound

pytestmark = pytest.mark.gpu

FILL = 0xCD
LONG = _lib.SYZSIG_DEFLATE_LONG
TILE = _lib.SYZSIG_SIGSET_TILE
DEL = C.DEL
TEXT = deflate_inputs()["text"]
RNG = np.random.default_rng(23)
NOISE = bytes(RNG.integers(0, 256, 6000, dtype=np.uint8))


def p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def u8(gpu, b):
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(gpu.dev) if len(b) else \
        torch.empty(0, dtype=torch.uint8, device=gpu.dev)


def pair(gpu, vals):
    """a list of byte strings as (data, off) on the device"""
    off = np.zeros(len(vals) + 1, np.int64)
    np.cumsum([len(v) for v in vals], out=off[1:])
    return u8(gpu, b"".join(vals)), torch.from_numpy(off).to(gpu.dev)


@functools.lru_cache(maxsize=None)
def host(v):
    return db.deflate_host(v)


def raw_deflate(gpu, vals, lead=0, cap=None, extra_cap=1, null_out=False):
    """The values laid back to back `lead` bytes into a source tensor that ends
    where they end; -> (rc, total, out, off), pre-filled with FILL / -1."""
    src = u8(gpu, b"\x5a" * lead + b"".join(vals))
    soff = np.zeros(len(vals), np.int64)
    if vals:
        soff[:] = lead + np.cumsum([0] + [len(v) for v in vals[:-1]])
    d_soff = torch.from_numpy(soff).to(gpu.dev)
    d_slen = torch.from_numpy(np.array([len(v) for v in vals], np.int32)).to(gpu.dev)
    cap = sum(len(host(v)) for v in vals) if cap is None else cap
    out = torch.full((cap + extra_cap,), FILL, dtype=torch.uint8, device=gpu.dev)
    off = torch.full((len(vals) + 2,), -1, dtype=torch.int64, device=gpu.dev)
    total = ctypes.c_uint64(12345)
    rc = gpu.L.syzsig_deflate_dev(gpu.eng.h, p(src), src.numel(), p(d_soff), p(d_slen), len(vals),
                                  None if null_out else p(out), 0 if null_out else cap, p(off), ctypes.byref(total))
    return rc, total.value, out.cpu().numpy(), off.cpu().numpy()


def check_deflate(gpu, vals, lead=0):
    """every stream equal to deflate_host's, byte for byte; -> stats"""
    exp = [host(v) for v in vals]
    rc, total, out, off = raw_deflate(gpu, vals, lead)
    n = len(vals)
    assert rc == 0, gpu.L.syzsig_last_error()
    lens = [len(s) for s in exp]
    assert off[: n + 1].tolist() == [0] + np.cumsum(lens).tolist() and off[n + 1] == -1
    assert total == sum(lens)
    got = out[:total].tobytes()
    if got != b"".join(exp):
        bad = [i for i in range(n) if got[off[i]:off[i + 1]] != exp[i]]
        raise AssertionError("streams %s differ from deflate_host's" % bad[:10])
    assert (out[total:] == FILL).all(), "wrote past out_bytes"
    st = db.deflate_stats(gpu)
    assert st[0] + st[1] == sum(1 for v in vals if v) == st[2] + st[3]
    assert (st[0], st[1]) == (sum(1 for v in vals if 0 < len(v) <= LONG), sum(1 for v in vals if len(v) > LONG))
    return st


# ---- the compressor ----

def test_device_bytes_equal_host_bytes_on_every_case(gpu):
    """... of tests/test_dbw_ref_cpu.py's inputs up to 200 KB, in one batch; and each
    reads back through zlib (there) and through syzsig_inflate_dev (here)"""
    names = [n for n, v in deflate_inputs().items() if len(v) <= 200_000]
    vals = [deflate_inputs()[n] for n in names]
    exp = [host_streams()[n] for n in names]
    data, off = db.deflate(gpu, *_ranges(gpu, vals))
    stats = db.deflate_stats(gpu)
    off_h = off.cpu().numpy()
    assert off_h.tolist() == [0] + np.cumsum([len(s) for s in exp]).tolist()
    got = data.cpu().numpy().tobytes()
    bad = [names[i] for i in range(len(names)) if got[off_h[i]:off_h[i + 1]] != exp[i]]
    assert not bad, bad[:10]
    assert stats[1] == sum(1 for v in vals if len(v) > LONG) > 20 and stats[2] > 300 and stats[3] > 2000
    back, boff, status = db.inflate(gpu, data, off[:-1].contiguous(), (off[1:] - off[:-1]).to(torch.int32))
    assert not status.any()
    assert back.cpu().numpy().tobytes() == b"".join(vals)
    assert boff.cpu().numpy().tolist() == [0] + np.cumsum([len(v) for v in vals]).tolist()


def _ranges(gpu, vals, lead=0):
    data, off = pair(gpu, [b"\x5a" * lead] + list(vals))
    return data, off[1:-1].contiguous(), (off[2:] - off[1:-1]).to(torch.int32)


@pytest.mark.parametrize("align", range(8))
def test_seams_at_every_source_alignment(gpu, align):
    """value i is P + P[:k] and value i + 1 begins with P[k:]: a match, a hash or a
    compare that ran over the seam would show against deflate_host"""
    P = TEXT[:300]
    vals = []
    for k in (1, 2, 3, 7, 64, 150, 299):
        vals += [P + P[:k], P[k:] + P[: k + 1]]
    for v in vals:
        assert R.inflate_class(host(v)) == (R.OK, v) and len(host(v)) <= stored_bound(len(v))
    check_deflate(gpu, vals, lead=align)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_shapes_with_empty_values_between(gpu, n):
    vals = [b"" if i % 3 == 1 else (TEXT[i:i + 40 + 5 * i] if i % 3 == 0 else NOISE[i:i + 200 + i]) for i in range(n)]
    st = check_deflate(gpu, vals, lead=n % 5)
    if n == 257:
        assert st[2] == 85 and st[3] == 86  # noise goes out stored, program text fixed


def test_same_value_in_any_lane_and_workgroup(gpu):
    v = TEXT[:1500]
    want = host(v)
    for at, n in ((0, 1), (0, 64), (63, 64), (64 + 17, 130)):
        vals = [NOISE[i:i + 200 + i] if i % 2 else TEXT[i:i + 900] for i in range(n)]
        vals[at] = v
        rc, total, out, off = raw_deflate(gpu, vals)
        assert rc == 0 and out[off[at]:off[at + 1]].tobytes() == want, (at, n)


def test_long_list_threshold_and_one_mib(gpu):
    text = (TEXT * (LONG // len(TEXT) + 2))
    for n, path in ((LONG - 1, 0), (LONG, 0), (LONG + 1, 1)):
        st = check_deflate(gpu, [text[:n], NOISE[:400]])
        assert st == (2 - path, path, 1, 1)
    big = (TEXT * ((1 << 20) // len(TEXT) + 1))[: 1 << 20]
    st = check_deflate(gpu, [TEXT[:50], big, NOISE[: LONG + 5]], lead=1)
    assert st == (1, 2, 1, 2)
    assert R.inflate_class(host(big)) == (R.OK, big)


def test_capacity_and_sizing(gpu):
    vals = [TEXT[:700], b"", NOISE[:500], TEXT[100:131]]
    need = sum(len(host(v)) for v in vals)
    rc, total, out, off = raw_deflate(gpu, vals, cap=need - 1)
    assert rc == _lib.SYZSIG_ERANGE and total == need and b"deflate" in gpu.L.syzsig_last_error()
    assert (out == FILL).all() and (off == -1).all()
    rc, total, out, off = raw_deflate(gpu, vals, cap=need, extra_cap=64)
    assert rc == 0 and total == need and (out[need:] == FILL).all()
    assert out[:need].tobytes() == b"".join(host(v) for v in vals)
    rc, total, out, off = raw_deflate(gpu, vals, null_out=True)  # the sizing call
    assert rc == 0 and total == need and (out == FILL).all()
    assert off[:5].tolist() == [0] + np.cumsum([len(host(v)) for v in vals]).tolist()


def test_bad_ranges_and_null_arguments(gpu):
    src = u8(gpu, TEXT[:100])
    out = torch.full((256,), FILL, dtype=torch.uint8, device=gpu.dev)
    off = torch.full((3,), -1, dtype=torch.int64, device=gpu.dev)
    total = ctypes.c_uint64(7)
    L, h = gpu.L, gpu.eng.h

    def call(soff, slen, src_=src, out_=out, off_=off, total_=total, cap=256, n=2):
        a = torch.tensor(soff, dtype=torch.int64, device=gpu.dev)
        b = torch.from_numpy(np.array(slen, np.uint32).view(np.int32)).to(gpu.dev)
        return L.syzsig_deflate_dev(h, p(src_), 100, p(a), p(b), n, p(out_), cap, p(off_),
                                    ctypes.byref(total_) if total_ is not None else None)

    for soff, slen in (([0, 90], [10, 11]), ([0, 101], [10, 1]), ([0, -8], [10, 16]), ([0, 1 << 62], [10, 0xFFFFFFFF])):
        assert call(soff, slen) == _lib.SYZSIG_EINVAL, (soff, slen)
        assert total.value == 0 and (out == FILL).all() and (off == -1).all()
    assert call([0, 100], [100, 0]) == 0 and total.value == len(host(TEXT[:100]))  # an empty value at the very end
    out.fill_(FILL)
    off.fill_(-1)
    assert call([0, 0], [1, 1], src_=None) == _lib.SYZSIG_EINVAL
    assert call([0, 0], [1, 1], off_=None) == _lib.SYZSIG_EINVAL
    assert call([0, 0], [1, 1], total_=None) == _lib.SYZSIG_EINVAL
    assert call([0, 0], [1, 1], out_=None) == _lib.SYZSIG_EINVAL  # NULL output with a capacity
    assert L.syzsig_deflate_dev(None, p(src), 100, p(off), p(off), 1, p(out), 256, p(off), ctypes.byref(total)) == \
        _lib.SYZSIG_EINVAL
    assert L.syzsig_deflate_dev(h, p(src), 100, p(off), p(off), (1 << 25) + 1, p(out), 256, p(off), ctypes.byref(total)) == \
        _lib.SYZSIG_ERANGE
    assert (out == FILL).all() and (off == -1).all()


# ---- the frames ----

def sigs_of(gpu, keys):
    return torch.from_numpy(np.frombuffer(b"".join(bytes.fromhex(k.decode()) for k in keys), np.uint8)
                            .reshape(-1, 20).copy()).to(gpu.dev) if keys else \
        torch.empty((0, 20), dtype=torch.uint8, device=gpu.dev)


def i64(gpu, seqs):
    return torch.from_numpy(np.array(seqs, np.uint64).view(np.int64)).to(gpu.dev)


def rand_key(rng):
    return bytes(rng.integers(0, 256, 20, dtype=np.uint8)).hex().encode()


@pytest.mark.parametrize("n", [0, 1, 300])
def test_records_equal_serialize_record(gpu, n):
    rng = np.random.default_rng(n)
    recs = []
    for i in range(n):
        kind = i % 4
        val = b"" if kind in (1, 2) else (TEXT[i:i + 3 * i + 1] if kind == 0 else NOISE[i:2 * i + 1])
        recs.append((rand_key(rng), val, DEL if kind == 1 else int(rng.integers(0, 1 << 63)) * 2 + (i & 1)))
    streams = db.deflate(gpu, *_ranges(gpu, [v for _, v, _ in recs]))
    want = [R.serialize_record(k, v, s, stream=host) for k, v, s in recs]
    sigs, seqs = sigs_of(gpu, [k for k, _, _ in recs]), i64(gpu, [s for _, _, s in recs])
    need = sum(len(w) for w in want)
    out = torch.full((need + 32,), FILL, dtype=torch.uint8, device=gpu.dev)
    data, off = db.db_records(gpu, sigs, seqs, streams, out=out[:need])
    assert off.cpu().numpy().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
    assert data.cpu().numpy().tobytes() == b"".join(want)
    assert (out[need:] == FILL).all()
    if n > 2:
        assert [len(want[1]), len(want[2])] == [56, 60]
    if n:
        out.fill_(FILL)
        with pytest.raises(_lib.SyzsigError) as e:
            db.db_records(gpu, sigs, seqs, streams, out=out[: need - 1])
        assert e.value.code == _lib.SYZSIG_ERANGE and e.value.needed == need and (out == FILL).all()


def test_records_delete_with_stream_and_bad_offsets(gpu):
    sigs, streams = sigs_of(gpu, [C.KA, C.KB]), pair(gpu, [b"\x03\x00", b"\x03\x00"])
    with pytest.raises(_lib.SyzsigError) as e:
        db.db_records(gpu, sigs, i64(gpu, [1, DEL]), streams)
    assert e.value.code == _lib.SYZSIG_EINVAL and "deleting record with value" in str(e.value)
    bad = (streams[0], torch.tensor([0, 3, 2], dtype=torch.int64, device=gpu.dev))
    with pytest.raises(_lib.SyzsigError) as e:
        db.db_records(gpu, sigs, i64(gpu, [1, 2]), bad)
    assert e.value.code == _lib.SYZSIG_EINVAL
    bad = (streams[0], torch.tensor([0, 2, 5], dtype=torch.int64, device=gpu.dev))
    with pytest.raises(_lib.SyzsigError) as e:
        db.db_records(gpu, sigs, i64(gpu, [1, 2]), bad)
    assert e.value.code == _lib.SYZSIG_EINVAL


# ---- Save and Delete over a batch ----

def make_db(gpu, live, version=3, uncompacted=None):
    return db.DB(gpu, version, sigs_of(gpu, [k for k, _, _ in live]), np.array([s for _, _, s in live], np.uint64),
                 pair(gpu, [v for _, v, _ in live]), len(live) if uncompacted is None else uncompacted, "eof")


def apply_ops(gpu, d, ops):
    """-> the written flags (the raw entry point, then the same batch through DB.apply)"""
    osigs, oseqs, ovals = sigs_of(gpu, [k for k, _, _ in ops]), i64(gpu, [s for _, _, s in ops]), \
        pair(gpu, [v or b"" for _, v, _ in ops])
    written, keep_live, keep_op, counts = db.db_apply(gpu, d.keys, i64(gpu, d.seqs), d.vals, osigs, oseqs, ovals)
    assert counts == (int(written.sum()), int(keep_live.sum()), int(keep_op.sum()))
    nw = d.apply(osigs, ovals, np.array([s for _, _, s in ops], np.uint64))
    assert nw == counts[0] and d.Len() == counts[1] + counts[2]
    return written.cpu().numpy().astype(bool)


def records_list(d):
    return list(d.records().items())


@pytest.mark.parametrize("name", sorted(C.APPLY))
def test_apply_hand_cases(gpu, name):
    live, ops, written, after = C.APPLY[name]
    d = make_db(gpu, live)
    got = apply_ops(gpu, d, ops)
    assert np.flatnonzero(got).tolist() == written
    assert records_list(d) == [(k, (v, s)) for k, v, s in after]
    assert d.uncompacted == len(live) + len(written)
    pending = b"".join(x.cpu().numpy().tobytes() for x in d.pending)
    assert pending == b"".join(R.serialize_record(*ops[j], stream=host) for j in written)
    if name == "nil_value_twice":
        assert len(pending) == 60


def ref_written(live, ops):
    """written[j] by the reference's own decisions: replay op by op and watch the log grow"""
    r, out = W.RefDB(3, {k: (v, s) for k, v, s in live}, stream=lambda v: b"\x03\x00"), []
    for op in ops:
        before = len(r.log)
        r.apply([op])
        out.append(len(r.log) > before)
    return out


def against_ref(gpu, live, ops):
    ref = W.RefDB(3, {k: (v, s) for k, v, s in live}, stream=host)
    ref.apply(ops)
    d = make_db(gpu, live)
    got = apply_ops(gpu, d, ops) if ops else np.zeros(0, bool)
    assert got.tolist() == ref_written(live, ops)
    assert records_list(d) == list(ref.records.items()) and d.uncompacted == ref.uncompacted
    assert b"".join(x.cpu().numpy().tobytes() for x in d.pending) == (ref.pending or b"")
    return d, ref


def test_apply_keys_that_differ_at_the_sort_words_seams(gpu):
    """the sort key is three words: Sig bytes 0-7, 8-15, 16-19; keys equal but for one byte next to a seam"""
    base = bytearray(b"\x55" * 20)
    keys = []
    for at in (0, 7, 8, 15, 16, 19):
        for delta in (1, 0x80):
            k = bytearray(base)
            k[at] ^= delta
            keys.append(bytes(k).hex().encode())
    live = [(k, b"v%d" % i, i) for i, k in enumerate(keys[::2])]
    ops = [(k, b"v%d" % (i // 2) if i % 2 == 0 else b"w", i // 2) for i, k in enumerate(keys)] + \
          [(k, None, DEL) for k in keys[1::4]] + [(bytes(base).hex().encode(), None, DEL)]
    against_ref(gpu, live, ops[:8])
    against_ref(gpu, live, ops)


@pytest.mark.parametrize("nl,m", [(TILE - 1, 1), (TILE, TILE), (1, TILE + 1), (0, 2 * TILE + 3), (TILE + 5, 0)])
def test_apply_around_the_sort_tile(gpu, nl, m):
    rng = np.random.default_rng(nl + m)
    keys = [rand_key(rng) for _ in range(nl + m // 2 + 1)]
    live = [(keys[i], b"L%d" % (i % 7), i % 3) for i in range(nl)]
    ops = []
    for j in range(m):
        k = keys[int(rng.integers(len(keys)))]
        r = j % 5
        ops.append((k, None, DEL) if r == 0 else (k, b"L%d" % (j % 7), j % 3))
    against_ref(gpu, live, ops)


def test_apply_random_batch_against_ref(gpu):
    rng = np.random.default_rng(99)
    keys = [rand_key(rng) for _ in range(2000)]
    vals = [TEXT[i % 50:i % 50 + 20 + i % 90] for i in range(40)] + [b""]
    live = [(keys[i], vals[i % 41], i % 4) for i in range(0, 2000, 2)]
    ops = []
    for j in range(5000):
        k = keys[int(rng.integers(2000))]
        ops.append((k, None, DEL) if rng.random() < 0.25 else (k, vals[int(rng.integers(41))], int(rng.integers(4))))
    d, ref = against_ref(gpu, live, ops)
    assert ref.uncompacted == 1000 + len(ref.log) and 1500 < len(ref.log) < 5000


def test_apply_argument_errors(gpu):
    d = make_db(gpu, [(C.KA, b"a", 1)])
    with pytest.raises(ValueError):
        d.save(sigs_of(gpu, [C.KB]), pair(gpu, [b"x"]), [DEL])
    with pytest.raises(_lib.SyzsigError) as e:  # a delete that carries a value
        d.apply(sigs_of(gpu, [C.KB]), pair(gpu, [b"x"]), [DEL])
    assert e.value.code == _lib.SYZSIG_EINVAL and "deleting record with value" in str(e.value)
    bad = (u8(gpu, b"xyz"), torch.tensor([0, 4], dtype=torch.int64, device=gpu.dev))
    with pytest.raises(_lib.SyzsigError) as e:
        d.apply(sigs_of(gpu, [C.KB]), bad, [1])
    assert e.value.code == _lib.SYZSIG_EINVAL
    assert records_list(d) == [(C.KA, (b"a", 1))] and d.uncompacted == 1 and not d.pending


# ---- Flush, compact, BumpVersion and the whole loop ----

@pytest.mark.parametrize("n,unc,compacts", C.FLUSH_BOUNDARY)
def test_flush_boundary(gpu, n, unc, compacts):
    recs, unc = C.boundary_db(n, unc)
    d = make_db(gpu, recs, version=7, uncompacted=unc)
    assert d.flush() == (("replace", R.serialize_db(7, recs, stream=host)) if compacts else None)
    d = make_db(gpu, recs, version=7, uncompacted=unc)
    d.pending = [u8(gpu, b"pending")]
    kind, data = d.flush()
    if compacts:
        assert (kind, data, d.uncompacted) == ("replace", R.serialize_db(7, recs, stream=host), n)
    else:
        assert (kind, data, d.uncompacted) == ("append", b"pending", unc)
    assert d.pending == [] and d.flush() is None


def test_bump_version_and_compact(gpu):
    live = [(C.KA, TEXT[:300], 1), (C.KB, b"", 2)]
    d = make_db(gpu, live, version=7)
    assert d.bump_version(7) is None
    d.save(sigs_of(gpu, [C.KC]), pair(gpu, [b"c"]), [3])
    assert d.bump_version(7) == ("append", R.serialize_record(C.KC, b"c", 3, stream=host))
    d.save(sigs_of(gpu, [C.KC]), pair(gpu, [b"c2"]), [3])
    assert d.uncompacted == 4 and d.pending
    kind, data = d.bump_version(8)
    assert kind == "replace" and d.version == 8 and d.pending == [] and d.uncompacted == 3
    want = {C.KA: (TEXT[:300], 1), C.KB: (b"", 2), C.KC: (b"c2", 3)}
    assert R.deserialize_db(data) == (8, want, 3, R.EOF)
    assert data == R.serialize_db(8, [(k, v, s) for k, (v, s) in want.items()], stream=host)


def test_reopen_after_flush_and_after_compact(gpu):
    rng = np.random.default_rng(4)
    keys = [rand_key(rng) for _ in range(60)]
    file0 = R.serialize_db(5, [(keys[i], TEXT[i:i + 10 * i], i) for i in range(40)])
    ops = [(keys[int(rng.integers(60))], None, DEL) if i % 4 == 0 else
           (keys[int(rng.integers(60))], NOISE[i:i + i % 9] + TEXT[i:3 * i], i % 3) for i in range(150)]
    d, ref = db.open_db(gpu, file0), W.RefDB.open(file0, stream=host)

    def step(batch):
        ref.apply(batch)
        d.apply(sigs_of(gpu, [k for k, _, _ in batch]), pair(gpu, [v or b"" for _, v, _ in batch]),
                np.array([s for _, _, s in batch], np.uint64))
        assert records_list(d) == list(ref.records.items()) and d.uncompacted == ref.uncompacted
        got = d.flush()
        assert got == ref.flush()
        return got

    def reopened(data):
        again = db.open_db(gpu, data)
        assert again.records() == ref.records and again.version == 5 and again.ended == "eof"
        version, records, unc, ended = R.deserialize_db(data)
        assert (version, records, ended) == (5, ref.records, R.EOF) and unc == again.uncompacted == d.uncompacted

    # 8 ops: at most 48 records in the file, 48 / 10 * 9 = 36 <= the 38 or more live ones: appended
    kind, tail = step(ops[:8])
    assert kind == "append"
    reopened(file0 + tail)
    # 142 more: the file would hold far more records than are live: compacted
    kind, data = step(ops[8:])
    assert kind == "replace" and d.uncompacted == d.Len()
    reopened(data)
    assert d.compact() == data and d.flush() is None


def test_new_inputs_saved_flushed_and_found_again(gpu):
    """wire bytes -> hash_batch -> save(..., 0) -> flush -> reopen -> new_input_keys (manager.go:1011-1012)"""
    progs = [TEXT[i * 30:i * 30 + 200 + i] for i in range(50)]
    progs[7] = progs[3]  # the same program twice in the batch: one record
    vals = pair(gpu, progs)
    sigs = hashing.hash_batch(gpu, *vals)
    d = db.open_db(gpu, b"")
    assert d.save(sigs, vals, np.zeros(50, np.uint64)) == 49
    kind, tail = d.flush()
    assert kind == "append"
    again = db.open_db(gpu, db.serialize_header(0) + tail)
    assert again.records() == {hashlib.sha1(v).hexdigest().encode(): (v, 0) for v in progs} and again.Len() == 49
    corpus = hashing.SigSet(gpu)
    corpus.add(again.hashes())
    keys = hashing.new_input_keys(gpu, progs[:5] + [b"a new program\n"], corpus)
    assert keys["nkeys"] == 6 and keys["present"].tolist() == [0, 1, 2, 3, 4]
    assert d.save(sigs, vals, np.zeros(50, np.uint64)) == 0 and d.flush() is None


def test_load_corpus_deletes_the_broken_programs(gpu):
    """open_db -> load_corpus -> delete of the broken programs (manager.go:209-216) -> flush -> reopen"""
    names = ["openat$dir", "mmap", "close"]
    good = [b"r0 = openat$dir(0xffffffffffffff9c, &(0x7f0000000000)='./file0\\x00', 0x0, 0x0)\nclose(r0)\n",
            b"mmap(&(0x7f0000000000/0x1000)=nil, 0x1000, 0x3, 0x32, 0xffffffffffffffff, 0x0)\n"]
    broken = [b"r0 = nosuchcall(0x0)\n", b"((((\n"]
    progs = [good[0], broken[0], good[1], broken[1]]
    file0 = R.serialize_db(1, [(hashlib.sha1(v).hexdigest().encode(), v, 0) for v in progs])
    d = db.open_db(gpu, file0)
    tab = progtext.CallTable(gpu, names)
    bad, _, cand = progtext.load_corpus(gpu, tab, d, np.ones(3, np.uint8))
    assert bad.cpu().tolist() == [1, 3] and cand.cpu().tolist() == [0, 2]
    assert d.delete(d.keys[bad]) == 2
    kind, tail = d.flush()
    assert kind == "append" and len(tail) == 2 * 56
    again = db.open_db(gpu, file0 + tail)
    assert again.records() == {hashlib.sha1(v).hexdigest().encode(): (v, 0) for v in good} and again.uncompacted == 6


def test_list_keyed_db_takes_the_host_path(gpu):
    recs = [(b"not-a-hash", TEXT[:100], 1), (C.KA, b"a", 2)]
    file0 = R.serialize_db(2, recs)
    d, ref = db.open_db(gpu, file0), W.RefDB.open(file0, stream=host)
    assert isinstance(d.keys, list)
    ops = [(b"not-a-hash", TEXT[:100], 1), (b"another key", TEXT[50:400], 0), (C.KA, None, DEL), (C.KA, None, DEL),
           (b"not-a-hash", b"", 1)]
    ref.apply(ops)
    assert d.apply([k for k, _, _ in ops], pair(gpu, [v or b"" for _, v, _ in ops]), [s for _, _, s in ops]) == 3
    assert records_list(d) == list(ref.records.items()) and d.uncompacted == ref.uncompacted == 5
    assert d.flush() == ref.flush()
    assert d.compact() == ref.compact()
    assert db.open_db(gpu, d.compact()).records() == ref.records
