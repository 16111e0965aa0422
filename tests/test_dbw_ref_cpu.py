"""CPU: pkg/db's write side restated (tests/dbw_ref.py) on the hand-derived
sequences of tests/dbw_cases.py; the compressor of syzsig_deflate_dev through
its host entry syzsig_deflate_host (the same csrc/deflate_core.h) against zlib:
every stream inflates back to its value and keeps the stored bound, and on
program-like records it beats Huffman-only coding, so matches are really found;
and deflate_core.h in tests/dbw_driver.cc under ASan + UBSan."""
import ctypes
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from syzkaller_amd import _lib, db
from tests import db_ref as R
from tests import dbw_cases as C
from tests import dbw_ref as W
from tests.conftest import ROOT

MAX_DIST = 32768


# ---- the hand cases through the restated reference ----

@pytest.mark.parametrize("name", sorted(C.APPLY))
def test_hand_cases(name):
    live, ops, written, after = C.APPLY[name]
    d = W.RefDB(3, {k: (v, s) for k, v, s in live})
    d.apply(ops)
    assert d.log == [(k, v or None if s == C.DEL else v, s) for k, v, s in (ops[j] for j in written)]
    assert list(d.records.items()) == [(k, (v, s)) for k, v, s in after]
    assert d.uncompacted == len(live) + len(written)
    # the log replays to the same records (deserializeDB over header + live + pending)
    data = R.serialize_db(3, live) + (d.pending or b"")
    assert (d.pending is None) == (not written)
    version, records, unc, ended = R.deserialize_db(data)
    assert (version, records, unc, ended) == (3, d.records, d.uncompacted, R.EOF)  # (as maps: db_ref keeps no order)


def test_nil_value_record_is_60_bytes():
    d = W.RefDB()
    d.apply(C.APPLY["nil_value_twice"][1])
    assert len(d.pending) == 60 and d.pending[-4:] == b"\0\0\0\0"


def test_reserved_seq_and_delete_with_value():
    d = W.RefDB()
    with pytest.raises(ValueError):
        d.save(C.KA, b"x", C.DEL)
    with pytest.raises(AssertionError):
        d.apply([(C.KA, b"x", C.DEL)])


@pytest.mark.parametrize("n,unc,compacts", C.FLUSH_BOUNDARY)
def test_flush_boundary(n, unc, compacts):
    recs, unc = C.boundary_db(n, unc)
    d = W.RefDB(7, {k: (v, s) for k, v, s in recs}, unc)
    d.pending = b"pending"
    kind, data = d.flush()
    assert kind == ("replace" if compacts else "append")
    if compacts:
        assert data == R.serialize_db(7, recs) and d.uncompacted == n
    else:
        assert data == b"pending" and d.uncompacted == unc
    assert d.pending is None
    assert d.flush() is None  # nothing pending, and a compacted database is below the boundary


def test_bump_version_and_compact():
    recs = [(C.KA, b"a", 1), (C.KB, b"", 2)]
    d = W.RefDB(7, {k: (v, s) for k, v, s in recs})
    assert d.bump_version(7) is None  # the same version: a Flush with nothing pending
    d.save(C.KC, b"c", 3)
    kind, data = d.bump_version(7)
    assert kind == "append" and data == R.serialize_record(C.KC, b"c", 3)
    d.save(C.KC, b"c2", 3)
    assert d.uncompacted == 4 and d.pending
    kind, data = d.bump_version(8)  # another version: compact, pending dropped
    assert kind == "replace" and d.version == 8 and d.pending is None and d.uncompacted == 3
    assert R.deserialize_db(data) == (8, {C.KA: (b"a", 1), C.KB: (b"", 2), C.KC: (b"c2", 3)}, 3, R.EOF)


# ---- syzsig_deflate_host against zlib ----

def stored_bound(n):
    return n + 5 * -(-n // 65535)


@functools.lru_cache(maxsize=None)
def program_records(n=2000):
    """the live values of scripts/time_db.py's synthetic corpus.db"""
    from scripts import time_db

    _, records, _, _ = R.deserialize_db(time_db.corpus_db(n))
    return [v for v, _ in records.values()]


@functools.lru_cache(maxsize=None)
def deflate_inputs():
    """name -> value: the shapes the compressor can go wrong on"""
    rng = np.random.default_rng(5)
    rnd = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))  # noqa: E731
    text = b"".join(b"r%d = openat$dir(0xffffffffffffff9c, &(0x7f0000000%03x)='./file%d\\x00', 0x%x, 0x0)\n" % (i, i * 8, i % 5, i)
                    for i in range(40))
    cases = {}
    for n in range(301):
        cases["random_%d" % n] = rnd(n)
        cases["byte_%d" % n] = b"z" * n
        for p in (2, 3, 7):
            cases["period%d_%d" % (p, n)] = (bytes(range(65, 65 + p)) * (n // p + 1))[:n]
    # the stored chunk seam and the wrap of the 16-bit positions
    for n in list(range(65534, 65539)) + list(range(131070, 131076)):
        cases["seam_random_%d" % n] = rnd(n)
        cases["seam_repeat_%d" % n] = (text * (n // len(text) + 1))[:n]
    # a block repeated at distance exactly 32768 and at 32769, with nothing else to match in between:
    # zlib with wbits = -15 rejects a distance of 32769
    block = rnd(300)
    for dist in (MAX_DIST, MAX_DIST + 1):
        cases["far_%d" % dist] = block + b"\0" * (dist - 300) + block
    cases["match_to_the_end"] = rnd(50) + text[:100] + rnd(20) + text[:100]
    base = rnd(259)
    for n in (257, 258, 259):
        cases["match_%d" % n] = base[:n] + b"--" + base[:n] + b"."
    cases["text"] = text
    for i, v in enumerate(program_records()):
        cases["prog_%d" % i] = v
    for i in range(200):
        cases["binary_%d" % i] = rnd(int(rng.integers(1, 2000)))
    return cases


@functools.lru_cache(maxsize=None)
def host_streams():
    return {name: db.deflate_host(v) for name, v in deflate_inputs().items()}


def test_streams_inflate_back_and_keep_the_stored_bound():
    for name, v in deflate_inputs().items():
        s = host_streams()[name]
        if not v:
            assert s == b"", name  # valLen = 0 and no stream (db.go:158-159)
            continue
        assert R.inflate_class(s) == (R.OK, v), name
        assert len(s) <= stored_bound(len(v)), name


def test_stream_shapes():
    """one final block: fixed for what compresses, stored chunks of at most 65535 for what does not"""
    s = host_streams()
    assert s["text"][0] & 7 == 0b011 and len(s["text"]) < len(deflate_inputs()["text"]) // 2
    r = s["random_300"]
    assert r[:5] == b"\x01" + struct.pack("<HH", 300, 300 ^ 0xFFFF) and len(r) == 305
    big = s["seam_random_65536"]
    assert len(big) == 65536 + 10 and big[:5] == b"\x00\xff\xff\x00\x00" and big[65540:65545] == b"\x01\x01\x00\xfe\xff"
    assert len(s["seam_random_65535"]) == 65535 + 5 and s["seam_random_65535"][0] == 1
    # the far block: found at 32768 (its second copy costs a few bytes), not at 32769 (300 literals again)
    assert len(s["far_32769"]) - len(s["far_32768"]) > 250
    # 258 is the longest match: 1 + 2 * 258 equal bytes are a literal and two matches at distance 1,
    # 3 + 8 + 2 * (8 + 5) + 7 = 44 bits; one byte more is one literal more, 52 bits; a run that ends in a
    # match of 3 (7 + 5 bits) has 56
    assert [len(db.deflate_host(b"z" * n)) for n in (517, 518, 520)] == [6, 7, 7]


def test_determinism_and_independence_of_the_neighbourhood():
    """the bytes depend on the value alone: not on what the buffer holds around it"""
    v = deflate_inputs()["text"]
    L = _lib.lib()
    want = host_streams()["text"]
    for lead, tail in ((0, b""), (1, v[:64]), (3, v), (7, b"\xff" * 9)):
        buf = ctypes.create_string_buffer(b"\x5a" * lead + v + tail)
        src = ctypes.cast(ctypes.addressof(buf) + lead, ctypes.c_void_p)
        n = ctypes.c_uint64()
        out = ctypes.create_string_buffer(len(want) + 8)
        assert L.syzsig_deflate_host(src, len(v), out, len(want), ctypes.byref(n)) == 0
        assert out.raw[: n.value] == want and out.raw[n.value:] == b"\0" * 8


def test_ratio_beats_huffman_only_on_program_records():
    vals = program_records()
    assert len(vals) > 1500
    raw = sum(len(v) for v in vals)
    ours = sum(len(host_streams()["prog_%d" % i]) for i in range(len(vals)))

    def z(v):
        c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        return len(c.compress(v) + c.flush())

    huff = sum(z(v) for v in vals)
    print("raw %d, deflate_host %d (%.3f), Z_HUFFMAN_ONLY %d (%.3f)" % (raw, ours, ours / raw, huff, huff / raw))
    assert ours < huff


def test_host_entry_arguments():
    L = _lib.lib()
    v = b"abcabcabcabcabcabc"
    src = ctypes.create_string_buffer(v)
    n = ctypes.c_uint64(99)
    assert L.syzsig_deflate_host(src, len(v), None, 0, ctypes.byref(n)) == 0 and 0 < n.value < len(v)
    need = n.value
    out = ctypes.create_string_buffer(b"\xcd" * 64)
    n.value = 99
    assert L.syzsig_deflate_host(src, len(v), out, need - 1, ctypes.byref(n)) == _lib.SYZSIG_ERANGE
    assert n.value == need and out.raw[:64] == b"\xcd" * 64 and b"deflate_host" in L.syzsig_last_error()
    assert L.syzsig_deflate_host(src, len(v), out, need, ctypes.byref(n)) == 0
    assert out.raw[need:64] == b"\xcd" * (64 - need) and R.inflate_class(out.raw[:need]) == (R.OK, v)
    assert L.syzsig_deflate_host(src, len(v), out, need, None) == _lib.SYZSIG_EINVAL
    assert L.syzsig_deflate_host(None, len(v), out, need, ctypes.byref(n)) == _lib.SYZSIG_EINVAL
    assert L.syzsig_deflate_host(src, len(v), None, need, ctypes.byref(n)) == _lib.SYZSIG_EINVAL
    assert L.syzsig_deflate_host(None, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert L.syzsig_deflate_host(src, _lib.SYZSIG_INFLATE_MAX_OUT + 1, None, 0, ctypes.byref(n)) == _lib.SYZSIG_ERANGE


def test_constants_match_header():
    txt = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    assert f"#define SYZSIG_DEFLATE_LONG {_lib.SYZSIG_DEFLATE_LONG}\n" in txt


# ---- csrc/deflate_core.h and the write side's argument checks on the CPU, under ASan + UBSan ----

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dbw_driver") / "dbw_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "dbw_driver.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "0 failures" in r.stdout
    return r.stdout.splitlines()


def test_argument_checks_under_sanitizer(driver):
    run_driver(driver, "args")


def test_deflate_core_under_sanitizer(driver, tmp_path):
    """Every prefix of a 600-byte program, and the other shapes up to the first
    stored seam, from exact-size heap blocks; the driver inflates each stream
    back with inflate_core.h and prints its size, which is the library's."""
    prog = program_records()[0]
    prog = (prog * (600 // len(prog) + 1))[:600]
    names = [n for n, v in deflate_inputs().items() if not n.startswith(("prog_", "binary_")) and len(v) <= 70000]
    vals = [prog[:k] for k in range(601)] + [deflate_inputs()[n] for n in names]
    blob = struct.pack("<I", len(vals)) + b"".join(struct.pack("<I", len(v)) + v for v in vals)
    p = tmp_path / "values.bin"
    p.write_bytes(blob)
    out = run_driver(driver, "deflate", str(p))
    want = [len(db.deflate_host(v)) for v in vals[:601]] + [len(host_streams()[n]) for n in names]
    assert [int(x) for x in out[: len(vals)]] == want
