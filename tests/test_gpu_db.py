"""GPU: pkg/db's read side -- syzsig_inflate_dev, syzsig_db_live_dev and
syzkaller_amd.db.open_db -- against zlib and tests/db_ref.py (pkg/db/db.go:177-265
restated).  Every expected value comes from zlib or db_ref, none from the
device; output buffers are pre-filled so that an unwritten or overwritten byte
shows; the paths taken are asserted from syzsig_inflate_stats."""
import ctypes
import hashlib
import zlib

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, db, hashing
from tests import db_cases as C
from tests import db_ref as R
from tests.test_db_ref_cpu import HAND_STREAMS, TWO, random_db

pytestmark = pytest.mark.gpu

FILL = 0xCD
LONG = _lib.SYZSIG_INFLATE_LONG
STORED, FIXED, DYNAMIC = (0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY)
RNG = np.random.default_rng(11)
TEXT = b"".join(b"r%d = openat$dir(0xffffffffffffff9c, &(0x7f0000000%03x)='./file%d\\x00', 0x%x, 0x0)\n" % (i, i * 8, i % 5, i)
                for i in range(60))
NOISE = bytes(RNG.integers(0, 256, 70000, dtype=np.uint8))


def raw_inflate(gpu, streams, lead=0, extra_cap=1, cap=None, null_out=False):
    """The streams laid back to back `lead` bytes into a source tensor that
    ends where they end; -> (rc, total, out uint8[cap + 1...], off, status), all
    pre-filled with FILL / -1."""
    src = np.frombuffer(b"\x5a" * lead + b"".join(streams), np.uint8)
    soff = np.zeros(len(streams), np.int64)
    if streams:
        soff[:] = lead + np.cumsum([0] + [len(s) for s in streams[:-1]])
    slen = np.array([len(s) for s in streams], np.int32)
    need = sum(len(R.inflate_class(s)[1]) for s in streams)
    cap = need if cap is None else cap
    d_src = torch.from_numpy(src.copy()).to(gpu.dev) if src.size else torch.empty(0, dtype=torch.uint8, device=gpu.dev)
    out = torch.full((cap + extra_cap,), FILL, dtype=torch.uint8, device=gpu.dev)
    off = torch.full((len(streams) + 2,), -1, dtype=torch.int64, device=gpu.dev)
    status = torch.full((len(streams) + 1,), FILL, dtype=torch.uint8, device=gpu.dev)
    total = ctypes.c_uint64(12345)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)  # noqa: E731
    d_soff, d_slen = torch.from_numpy(soff).to(gpu.dev), torch.from_numpy(slen).to(gpu.dev)
    rc = gpu.L.syzsig_inflate_dev(gpu.eng.h, p(d_src), src.size, p(d_soff), p(d_slen), len(streams),
                                  None if null_out else p(out), 0 if null_out else cap, p(off), p(status),
                                  ctypes.byref(total))
    return rc, total.value, out.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy()


def check_inflate(gpu, streams, lead=0):
    """every stream's (class, bytes) against zlib's; -> stats"""
    exp = [R.inflate_class(s) if s else (R.OK, b"") for s in streams]
    rc, total, out, off, status = raw_inflate(gpu, streams, lead)
    n = len(streams)
    assert rc == 0, gpu.L.syzsig_last_error()
    assert status[:n].tolist() == [c for c, _ in exp] and status[n] == FILL
    lens = [len(b) for _, b in exp]
    assert off[: n + 1].tolist() == [0] + np.cumsum(lens).tolist() and off[n + 1] == -1
    assert total == sum(lens)
    assert out[:total].tobytes() == b"".join(b for _, b in exp)
    assert (out[total:] == FILL).all(), "wrote past out_bytes"
    st = db.inflate_stats(gpu)
    assert st[0] + st[1] == sum(1 for s in streams if s)
    return st


# ---- block types and stream shapes ----

@pytest.mark.parametrize("kind,idx", [(STORED, 2), (FIXED, 3), (DYNAMIC, 4)])
def test_block_types_alone_and_in_the_go_shape(gpu, kind, idx):
    c = zlib.compressobj(kind[0], zlib.DEFLATED, -15, 9, kind[1])
    alone = c.compress(TEXT) + c.flush()
    st = check_inflate(gpu, [alone])
    assert st[idx] == 1 and sum(st[2:]) == 1
    st = check_inflate(gpu, [R.go_stream(TEXT, *kind)], lead=3)
    assert st[idx] == (3 if kind is STORED else 1) and st[2] == (3 if kind is STORED else 2)


def seg(d, kind):
    c = zlib.compressobj(kind[0], zlib.DEFLATED, -15, 9, kind[1])
    return c.compress(d) + c.flush(zlib.Z_SYNC_FLUSH)


def test_three_segments_and_empty_stored_blocks(gpu):
    empty, final = b"\x00\x00\x00\xff\xff", b"\x01\x00\x00\xff\xff"
    s1 = seg(TEXT[:500], STORED) + seg(b"tiny", FIXED) + seg(TEXT, DYNAMIC) + final
    assert R.inflate_class(s1) == (R.OK, TEXT[:500] + b"tiny" + TEXT)
    st = check_inflate(gpu, [s1])
    assert st[2:] == (5, 1, 1)  # stored: the data in two blocks, the three flushes' empty ones, the final one
    s2 = empty + seg(TEXT, DYNAMIC) + empty + empty + seg(b"x", FIXED) + final
    st = check_inflate(gpu, [s2, empty * 3 + final, final])
    assert st[2:] == (1 + 1 + 2 + 1 + 1 + 4 + 1, 1, 1)


def test_stored_block_of_65535_bytes(gpu):
    d = NOISE[:65535]
    s = b"\x01\xff\xff\x00\x00" + d
    assert R.inflate_class(s) == (R.OK, d)
    st = check_inflate(gpu, [s], lead=1)
    assert st[:3] == (0, 1, 1)  # longer than SYZSIG_INFLATE_LONG: the long list


# ---- matches ----

def test_matches(gpu):
    far = NOISE[:32768]
    datas = [b"a" * 1000, b"abc" * 500, NOISE[:257] * 6, far + far[:400], far[:32767] + far[:400], b"\x00" * 70000]
    streams = [R.go_stream(d, *k) for d in datas for k in (FIXED, DYNAMIC)]
    check_inflate(gpu, streams, lead=5)


def test_one_mib_record_takes_the_long_path(gpu):
    d = (TEXT * (1 + (1 << 20) // len(TEXT)))[: 1 << 20]
    big = R.go_stream(d, 6, zlib.Z_DEFAULT_STRATEGY)
    assert len(big) > LONG
    st = check_inflate(gpu, [R.go_stream(TEXT, *DYNAMIC), big, R.go_stream(b"tail", *FIXED)])
    assert st[:2] == (2, 1)


def test_one_long_stream_among_200_short_ones(gpu):
    progs = [TEXT[i * 7 % 900: i * 7 % 900 + 150 + i] for i in range(200)]
    streams = [R.go_stream(p) for p in progs]
    streams.insert(77, R.go_stream(NOISE[:20000], *STORED))
    st = check_inflate(gpu, streams, lead=2)
    assert st[:2] == (200, 1)


def test_long_threshold(gpu):
    mk = lambda n: b"\x01" + int(n - 5).to_bytes(2, "little") + int((n - 5) ^ 0xFFFF).to_bytes(2, "little") + NOISE[: n - 5]  # noqa: E731
    st = check_inflate(gpu, [mk(LONG - 1), mk(LONG), mk(LONG + 1)])
    assert st[:2] == (2, 1)


# ---- alignment ----

def test_every_source_and_output_alignment(gpu):
    s40 = R.go_stream(TEXT[:40], *FIXED)
    for lead in range(16):
        check_inflate(gpu, [s40], lead=lead)
    streams = []
    for k in range(16):  # outputs of 0..15 bytes in front move the next output across every alignment
        streams += [R.go_stream(TEXT[:k], *FIXED), s40]
    check_inflate(gpu, streams, lead=1)


# ---- batch shapes ----

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_shapes(gpu, n):
    rng = np.random.default_rng(n)
    kinds = (STORED, FIXED, DYNAMIC)
    streams = [R.go_stream(TEXT[int(a): int(a) + int(l)], *kinds[i % 3])
               for i, (a, l) in enumerate(zip(rng.integers(0, 2000, n), rng.integers(0, 600, n)))]
    check_inflate(gpu, streams, lead=n % 5)


def test_only_zero_length_entries(gpu):
    st = check_inflate(gpu, [b""] * 70)
    assert st == (0, 0, 0, 0, 0)
    check_inflate(gpu, [b"", R.go_stream(b"x"), b"", b""])


# ---- capacity ----

def test_capacity_exact_short_and_sizing(gpu):
    streams = [R.go_stream(TEXT[:300]), R.go_stream(b"abc", *FIXED)]
    rc, total, out, off, status = raw_inflate(gpu, streams, extra_cap=0)
    assert rc == 0 and total == 303 and out.tobytes() == TEXT[:300] + b"abc"
    rc, total, out, off, status = raw_inflate(gpu, streams, cap=302)
    assert rc == _lib.SYZSIG_ERANGE and total == 303
    assert (out == FILL).all() and (off == -1).all() and (status == FILL).all()
    assert b"inflate" in gpu.L.syzsig_last_error()
    rc, total, out, off, status = raw_inflate(gpu, streams, null_out=True)  # the sizing call
    assert rc == 0 and total == 303 and (out == FILL).all()
    assert off[:3].tolist() == [0, 300, 303] and status[:2].tolist() == [0, 0]


# ---- error classes ----

def bad_streams():
    good = R.go_stream(TEXT[:200], *DYNAMIC)
    fixed = R.go_stream(TEXT[:200], *FIXED)
    return [good[:-1], good[:-6], good[:-11], fixed[: len(fixed) // 2], good + b"\x00"] + HAND_STREAMS


@pytest.mark.parametrize("i", range(len(bad_streams())))
def test_bad_stream_between_two_good_ones(gpu, i):
    bad = bad_streams()[i]
    a, b = R.go_stream(TEXT[:333], *DYNAMIC), R.go_stream(TEXT[100:150], *FIXED)
    check_inflate(gpu, [a, bad, b], lead=i % 4)


def test_every_error_class_is_met():
    classes = {R.inflate_class(s)[0] for s in bad_streams() if s}
    assert classes == {R.OK, R.S_TRUNCATED, R.S_INVALID, R.S_TRAILING}


def test_corruption_sweep(gpu):
    """200 valid streams, one bit flipped in each at a seeded place: the class and the bytes are zlib's."""
    rng = np.random.default_rng(2024)
    streams = []
    for i in range(200):
        a, l = int(rng.integers(0, 3000)), int(rng.integers(1, 900))
        s = bytearray(R.go_stream(TEXT[a: a + l], *(STORED, FIXED, DYNAMIC, DYNAMIC)[i % 4]))
        at = int(rng.integers(len(s) * 8))
        s[at >> 3] ^= 1 << (at & 7)
        streams.append(bytes(s))
    classes = [R.inflate_class(s)[0] for s in streams]
    assert len(set(classes)) >= 3
    check_inflate(gpu, streams, lead=7)


# ---- error paths: nothing is written ----

@pytest.mark.parametrize("what", ["null_off", "null_len", "null_status", "null_out_off", "null_total", "null_src",
                                  "past_nbytes", "offset_past_nbytes", "offset_wraps"])
def test_inflate_errors_write_nothing(gpu, what):
    s = R.go_stream(b"hello")
    src = torch.from_numpy(np.frombuffer(s + s, np.uint8).copy()).to(gpu.dev)
    soff = [0, len(s)]
    slen = [len(s), len(s)]
    if what == "past_nbytes":
        slen[1] += 1
    elif what == "offset_past_nbytes":
        soff[1] = 2 * len(s) + 1
    elif what == "offset_wraps":
        soff[1] = -len(s) + 1  # as u64: offset + length wraps around to 1
    d_off, d_len = torch.tensor(soff, dtype=torch.int64, device=gpu.dev), torch.tensor(slen, dtype=torch.int32, device=gpu.dev)
    out = torch.full((64,), FILL, dtype=torch.uint8, device=gpu.dev)
    ooff = torch.full((3,), -1, dtype=torch.int64, device=gpu.dev)
    status = torch.full((2,), FILL, dtype=torch.uint8, device=gpu.dev)
    total = ctypes.c_uint64(0)
    p = lambda t, name: ctypes.c_void_p(0 if what == "null_" + name else t.data_ptr())  # noqa: E731
    rc = gpu.L.syzsig_inflate_dev(gpu.eng.h, p(src, "src"), src.numel(), p(d_off, "off"), p(d_len, "len"), 2, p(out, "out"),
                                  64, p(ooff, "out_off"), p(status, "status"),
                                  None if what == "null_total" else ctypes.byref(total))
    assert rc == _lib.SYZSIG_EINVAL and b"inflate" in gpu.L.syzsig_last_error()
    assert (out.cpu().numpy() == FILL).all() and (ooff.cpu().numpy() == -1).all() and (status.cpu().numpy() == FILL).all()


def test_db_live_errors_write_nothing(gpu):
    sigs = torch.zeros((3, 20), dtype=torch.uint8, device=gpu.dev)
    seqs = torch.zeros(3, dtype=torch.int64, device=gpu.dev)
    live = torch.full((3,), FILL, dtype=torch.uint8, device=gpu.dev)
    nl, unc = ctypes.c_uint64(9), ctypes.c_uint64(9)
    args = lambda a, b, c, nv: (gpu.eng.h, a, b, 3, nv, c, ctypes.byref(nl), ctypes.byref(unc))  # noqa: E731
    for a, b, c, nv in ((None, seqs.data_ptr(), live.data_ptr(), 3), (sigs.data_ptr(), None, live.data_ptr(), 3),
                        (sigs.data_ptr(), seqs.data_ptr(), None, 3), (sigs.data_ptr(), seqs.data_ptr(), live.data_ptr(), 4)):
        assert gpu.L.syzsig_db_live_dev(*args(a, b, c, nv)) == _lib.SYZSIG_EINVAL
        assert b"db_live" in gpu.L.syzsig_last_error() and (live.cpu().numpy() == FILL).all()


# ---- the live set ----

def test_db_live_against_the_loop(gpu):
    rng = np.random.default_rng(5)
    for n, nkeys, nvalid in ((1, 1, 1), (50, 7, 50), (50, 7, 31), (5000, 900, 4999), (300, 300, 0)):
        keys = rng.integers(0, 256, (nkeys, 20), dtype=np.uint8)
        keys[:, :19] = keys[0, :19] if nkeys < 10 else keys[:, :19]  # few keys: they differ in the last byte alone
        which = rng.integers(0, nkeys, n)
        seqs = np.where(rng.random(n) < 0.25, np.uint64(R.SEQ_DELETED), rng.integers(0, 1 << 40, n).astype(np.uint64))
        model = {}
        for i in range(nvalid):
            k = keys[which[i]].tobytes()
            model.pop(k, None)
            if int(seqs[i]) != R.SEQ_DELETED:
                model[k] = i
        exp = np.zeros(n, np.uint8)
        exp[list(model.values())] = 1
        live, nlive, unc = db.db_live(gpu, torch.from_numpy(keys[which]).to(gpu.dev),
                                      torch.from_numpy(seqs.view(np.int64)).to(gpu.dev), nvalid)
        assert np.array_equal(live.cpu().numpy(), exp) and nlive == len(model) and unc == nvalid


# ---- database level ----

def check_open(gpu, data):
    version, records, unc, ended = R.deserialize_db(data)
    d = db.open_db(gpu, data)
    assert (d.version, d.uncompacted, d.ended, d.Len()) == (version, unc, ended, len(records))
    assert d.records() == records
    assert d.needs_compact() == R.needs_compact(len(records), unc)
    return d


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_open_db_hand_cases(gpu, name):
    data, version, records, unc, ended = C.CASES[name]
    d = check_open(gpu, data)
    assert (d.version, d.records(), d.uncompacted, d.ended) == (version, records, unc, ended)


def test_open_db_every_prefix(gpu):
    for n in range(len(TWO) + 1):
        check_open(gpu, TWO[:n])


def big_db(rng):
    """300 programs, 50 overwrites, 30 deletes, 10 re-adds, shuffled (a re-add after its delete)."""
    progs = [TEXT[int(a): int(a) + int(l)] for a, l in zip(rng.integers(0, 3000, 300), rng.integers(1, 800, 300))]
    key = lambda v: hashlib.sha1(v).hexdigest().encode()  # noqa: E731
    recs = [(key(p), p, i) for i, p in enumerate(progs)]
    extra = [(recs[i][0], progs[(i + 1) % 300], 1000 + i) for i in range(50)]
    extra += [(recs[100 + i][0], None, R.SEQ_DELETED) for i in range(30)]
    order = rng.permutation(len(recs) + len(extra))
    allr = [(recs + extra)[i] for i in order]
    return allr + [(recs[100 + i][0], progs[100 + i], 2000 + i) for i in range(10)]


def test_open_db_300_programs(gpu):
    rng = np.random.default_rng(9)
    recs = big_db(rng)
    data = R.serialize_db(3, recs)
    d = check_open(gpu, data)
    assert 250 <= d.Len() <= 300
    # one corrupted stream at record 0, in the middle, last: the replay keeps what came before
    _, _, ko, kl, sq, vo, vl = db.scan(data)
    with_value = np.flatnonzero(vl)
    for i in (int(with_value[0]), int(with_value[with_value.size // 2]), int(with_value[-1])):
        x = bytearray(data)
        x[int(vo[i])] = 0x07  # block type 3
        d = check_open(gpu, bytes(x))
        assert d.uncompacted == i and d.ended == "inflate"


def test_open_db_non_hex_key_takes_the_host_replay(gpu):
    data, version, records, unc, ended = C.NONHEX
    d = check_open(gpu, data)
    assert isinstance(d.keys, list) and d.records() == records
    rng = np.random.default_rng(3)
    recs, model = random_db(rng, 10, 80)
    recs.insert(40, (b"UPPER" + b"A" * 35, b"v", 5))  # 40 characters, not lower-case hex
    d = check_open(gpu, R.serialize_db(1, recs))
    assert isinstance(d.keys, list)


# ---- the chain: file -> values -> hashes -> NewInput keys ----

def test_chain_from_file_to_new_input_keys(gpu):
    rng = np.random.default_rng(21)
    progs = list({TEXT[int(a): int(a) + int(l)] for a, l in zip(rng.integers(0, 3000, 300), rng.integers(1, 800, 300))})
    recs = [(hashlib.sha1(p).hexdigest().encode(), p, i) for i, p in enumerate(progs)]
    d = db.open_db(gpu, R.serialize_db(1, recs))
    assert d.Len() == len(progs) and d.ended == "eof"
    h = d.hashes().cpu().numpy()
    assert [bytes(x) for x in h] == [hashlib.sha1(p).digest() for p in progs]
    assert np.array_equal(h, d.keys.cpu().numpy())  # hash.String(val) is the record's key
    data, off = d.vals[0].cpu().numpy().tobytes(), d.vals[1].cpu().numpy()
    vals = [data[int(off[i]): int(off[i + 1])] for i in range(d.Len())]
    known = hashing.SigSet(gpu)
    known.add(d.keys[:10])
    ni = hashing.new_input_keys(gpu, vals + vals[:5], known)
    assert ni["nkeys"] == len(progs) and ni["present"].tolist() == list(range(10))
    assert np.array_equal(ni["sigs"].cpu().numpy()[: len(progs)], h)
