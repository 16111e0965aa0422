"""CPU: pkg/db's replay restated (tests/db_ref.py) on the hand-derived files of
tests/db_cases.py, its reader against its writer, and the host-compilable halves
of csrc/db.hip -- db_args.h (the frame walk of syzsig_db_scan, the argument
checks) and inflate_core.h (the decoder of syzsig_inflate_dev) -- in
tests/db_driver.cc under ASan + UBSan, against zlib."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from syzkaller_amd import _lib
from tests import db_cases as C
from tests import db_ref as R
from tests.conftest import ROOT

END_CODE = {R.EOF: _lib.SYZSIG_DB_END_EOF, R.BAD_HEADER: _lib.SYZSIG_DB_END_BAD_HEADER,
            R.BAD_MAGIC: _lib.SYZSIG_DB_END_BAD_MAGIC, R.TRUNCATED: _lib.SYZSIG_DB_END_TRUNCATED}


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_hand_cases(name):
    data, version, records, uncompacted, ended = C.CASES[name]
    assert R.deserialize_db(data) == (version, records, uncompacted, ended)


def test_nonhex_hand_case():
    assert R.deserialize_db(C.NONHEX[0]) == C.NONHEX[1:]


@pytest.mark.parametrize("unc,n,want", [(10, 9, False), (11, 9, False), (20, 18, False), (20, 17, True), (0, 0, True),
                                        (9, 1, False), (10, 8, True)])
def test_needs_compact_boundary(unc, n, want):
    """db.go:49: uncompacted/10*9 > len(Records), in integer arithmetic."""
    assert R.needs_compact(n, unc) is want
    # ... and on a file: n keys, then unc - n overwrites of the first
    recs = [(b"%040x" % i, b"v%d" % i, i) for i in range(n)] + [(b"%040x" % 0, b"w", 100 + i) for i in range(unc - n)]
    _, got, u, _ = R.deserialize_db(R.serialize_db(1, recs, stream=R.stored_stream))
    assert (len(got), u) == (n, unc) and R.needs_compact(len(got), u) is want


def random_db(rng, nkeys, nops, stream=R.go_stream):
    keys = [bytes(rng.integers(0, 256, 20, dtype=np.uint8)).hex().encode() for _ in range(nkeys)]
    recs, model = [], {}
    for i in range(nops):
        k = keys[int(rng.integers(nkeys))]
        if rng.random() < 0.2:
            recs.append((k, None, R.SEQ_DELETED))
            model.pop(k, None)
        else:
            v = bytes(rng.integers(97, 101, int(rng.integers(0, 400)), dtype=np.uint8))
            recs.append((k, v, i))
            model[k] = (v, i)
    return recs, model


def test_reader_against_writer_on_random_databases():
    rng = np.random.default_rng(1)
    for _ in range(20):
        recs, model = random_db(rng, 12, 60)
        version = int(rng.integers(0, 1 << 62))
        assert R.deserialize_db(R.serialize_db(version, recs)) == (version, model, len(recs), R.EOF)


def test_go_stream_shape():
    """Write + Flush + Close: ends with the two empty stored blocks; zlib reads
    it to eof with nothing left over, for each block type."""
    text = b"mmap(&(0x7f0000000000/0x1000)=nil, 0x1000, 0x3, 0x32, 0xffffffffffffffff, 0x0)\n" * 8
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY)):
        s = R.go_stream(text, level, strategy)
        assert s.endswith(b"\x00\x00\xff\xff\x01\x00\x00\xff\xff")
        assert R.inflate_class(s) == (R.OK, text)
        assert R.inflate_class(s[:-1])[0] == R.S_TRUNCATED and R.inflate_class(s + b"\x00")[0] == R.S_TRAILING
    assert R.inflate_class(R.stored_stream(text)) == (R.OK, text)


TWO = C.HDR2 + C.A1 + C.B2  # 16 + 78 + 66 bytes


def test_every_prefix_of_a_two_record_file():
    bounds = {len(C.HDR2): 0, len(C.HDR2 + C.A1): 1, len(TWO): 2}
    for n in range(len(TWO) + 1):
        version, recs, unc, ended = R.deserialize_db(TWO[:n])
        if n == 0:
            assert (version, recs, unc, ended) == (0, {}, 0, R.EOF)
        elif n < 16:
            assert (version, recs, unc, ended) == (0, {}, 0, R.BAD_HEADER)
        else:
            assert version == 7 and unc == max(v for k, v in bounds.items() if k <= n)
            assert ended == (R.EOF if n in bounds else R.TRUNCATED)
            assert recs == dict(list({C.KA: (b"abc", 1), C.KB: (b"q", 2)}.items())[:unc])


# ---- syzsig_db_scan through the library (host only: no context, no device) ----

def lib_scan(data, cap=None):
    L = _lib.lib()
    buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    ver, n, ended = ctypes.c_uint64(99), ctypes.c_uint64(99), ctypes.c_uint32(99)
    rc = L.syzsig_db_scan(buf, len(data), 0, ctypes.byref(ver), ctypes.byref(n), ctypes.byref(ended), None, None, None,
                          None, None)
    assert rc == (_lib.SYZSIG_ERANGE if n.value else _lib.SYZSIG_OK)
    cap = n.value if cap is None else cap
    ko, sq, vo = (np.full(cap + 1, 0xAB, np.uint64) for _ in range(3))
    kl, vl = (np.full(cap + 1, 0xAB, np.uint32) for _ in range(2))
    ver2, n2, ended2 = ctypes.c_uint64(99), ctypes.c_uint64(99), ctypes.c_uint32(99)
    rc = L.syzsig_db_scan(buf, len(data), cap, ctypes.byref(ver2), ctypes.byref(n2), ctypes.byref(ended2),
                          ko.ctypes.data, kl.ctypes.data, sq.ctypes.data, vo.ctypes.data, vl.ctypes.data)
    return rc, ver2.value, n2.value, ended2.value, (ko, kl, sq, vo, vl)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_scan_frames_the_hand_cases(name):
    data, version, _, uncompacted, ended = C.CASES[name]
    rc, ver, n, end, (ko, kl, sq, vo, vl) = lib_scan(data)
    assert rc == 0 and ver == version
    # the scan frames every record; the replay stops at a bad value, which the scan does not read
    assert n >= uncompacted and (n == uncompacted) == (ended in END_CODE)
    if ended in END_CODE:
        assert end == END_CODE[ended]
    for a in (ko, kl, sq, vo, vl):
        assert a[n] == 0xAB, "wrote past n"
    # the frames give back the reference's records
    records = {}
    for i in range(n):
        key = data[int(ko[i]):int(ko[i]) + int(kl[i])]
        if int(sq[i]) == R.SEQ_DELETED:
            assert vo[i] == 0 and vl[i] == 0
            records.pop(key, None)
            continue
        cls, val = R.inflate_class(data[int(vo[i]):int(vo[i]) + int(vl[i])]) if vl[i] else (R.OK, b"")
        if cls != R.OK:
            break
        records[key] = (val, int(sq[i]))
    assert records == C.CASES[name][2]


def test_scan_capacity_and_null_arguments():
    data = C.CASES["three_keys"][0]
    rc, ver, n, end, arrays = lib_scan(data, cap=2)
    assert rc == _lib.SYZSIG_ERANGE and n == 3 and ver == 99 and end == 99  # n set, nothing else written
    assert all((a == 0xAB).all() for a in arrays)
    assert b"db_scan" in _lib.lib().syzsig_last_error()
    L = _lib.lib()
    n = ctypes.c_uint64()
    assert L.syzsig_db_scan(None, 5, 0, None, ctypes.byref(n), None, None, None, None, None, None) == _lib.SYZSIG_EINVAL


# ---- csrc/db_args.h and csrc/inflate_core.h on the CPU, under ASan + UBSan ----

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("db_driver") / "db_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "db_driver.cc")], capture_output=True, text=True, timeout=300)
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


def test_scan_every_prefix_and_hostile_lengths_under_sanitizer(driver, tmp_path):
    p = tmp_path / "two.db"
    p.write_bytes(TWO)
    out = run_driver(driver, "scan", str(p))
    for n in range(len(TWO) + 1):
        version, _, unc, ended = R.deserialize_db(TWO[:n])  # (stored values: every framed record replays)
        assert out[n].split() == [str(unc), str(END_CODE[ended]), str(version)], n


def make_streams():
    """(stream, zlib's class, zlib's bytes) over the block types, the stream
    shapes, the match shapes and one-bit corruptions of them."""
    rng = np.random.default_rng(7)
    text = b"".join(b"r%d = openat$dir(0xffffffffffffff9c, &(0x7f0000000%03x)='./file%d\\x00', 0x0, 0x0)\n" % (i, i * 8, i % 5)
                    for i in range(40))
    noise = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    datas = [b"", b"a", b"abc", text, text[:100], noise, b"a" * 1000, b"abc" * 400, bytes(range(256)) * 2 + b"\x00",
             bytes(rng.integers(0, 256, 257, dtype=np.uint8)) * 5, b"\x00" * 70000, noise[:700] + text + noise[:700]]
    far = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    datas += [far + far[:300], far[:32767] + far[:300]]
    good = []
    for d in datas:
        for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY),
                                (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
            good.append(R.go_stream(d, level, strategy))
        c = zlib.compressobj(9, zlib.DEFLATED, -15)
        good.append(c.compress(d) + c.flush())  # one final block, no Flush / Close blocks
    # three sync-flushed segments of different types (byte-aligned, no shared history) + the final block
    seg = lambda d, lv, st: (lambda c: c.compress(d) + c.flush(zlib.Z_SYNC_FLUSH))(zlib.compressobj(lv, zlib.DEFLATED, -15, 9, st))  # noqa: E731
    good.append(seg(text, 0, 0) + seg(b"tiny", 9, zlib.Z_FIXED) + seg(text, 9, 0) + b"\x01\x00\x00\xff\xff")
    good.append(b"\x00\x00\x00\xff\xff" + seg(text, 9, 0) + b"\x00\x00\x00\xff\xff" * 2 + b"\x01\x00\x00\xff\xff")
    streams = list(good)
    for s in good:
        if len(s) > 40000:
            continue
        for cut in (1, 2, 5, 6, len(s) // 2):
            streams.append(s[:-cut] if cut < len(s) else b"")
        streams.append(s + b"\x00")
        for _ in range(12):
            at = int(rng.integers(len(s) * 8))
            streams.append(s[:at >> 3] + bytes([s[at >> 3] ^ (1 << (at & 7))]) + s[(at >> 3) + 1:])
    streams += HAND_STREAMS
    return [(s,) + R.inflate_class(s) for s in streams]


def bits(*fields):
    """(value, nbits) fields, LSB first, into bytes"""
    acc = n = 0
    for v, k in fields:
        acc |= v << n
        n += k
    return acc.to_bytes((n + 7) // 8, "little")


def dyn_header(cl_lens, hlit=0, hdist=0):
    """a final dynamic block's header with the given 19 code-length-code lengths (in RFC order of symbols)"""
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    return [(1, 1), (2, 2), (hlit, 5), (hdist, 5), (15, 4)] + [(cl_lens.get(s, 0), 3) for s in order]


def h(code, n):
    """a Huffman code of n bits (they go most significant bit first)"""
    return int(format(code, "0%db" % n)[::-1], 2), n


FIXED = [(1, 1), (1, 2)]  # a final fixed block's header
LIT_A, LEN3, EOB = h(0x30 + ord("a"), 8), h(1, 7), h(0, 7)
# hand-built streams: each one's class is whatever zlib says (make_streams asks it)
HAND_STREAMS = [
    b"\x07",                                           # final, block type 3
    b"\x01\x03\x00\xfc\xfe" + b"abc",                  # LEN != ~NLEN
    b"\x01\x03\x00\xfc\xff" + b"ab",                   # a stored block cut short
    b"\x01\x03\x00\xfc",                               # ... inside LEN / NLEN
    bits(*FIXED, LEN3, h(0, 5), EOB),                  # a match (length 3, distance 1) as the very first symbol
    bits(*FIXED, LIT_A, LEN3, h(1, 5), EOB),           # 'a', then distance 2: one byte too far
    bits(*FIXED, LIT_A, LEN3, h(0, 5), EOB),           # 'a', then distance 1: fine, "aaaa"
    bits(*FIXED, h(0xC0 + 6, 8), EOB),                 # literal/length symbol 286
    bits(*FIXED, LIT_A, LEN3, h(30, 5), EOB),          # distance symbol 30
    bits(*dyn_header({0: 1, 1: 1, 2: 1})),             # code-length code over-subscribed
    bits(*dyn_header({0: 2, 1: 2})),                   # ... incomplete
    bits(*dyn_header({0: 1})),                         # ... a single one-bit code: incomplete too
    bits(*dyn_header({})),                             # ... empty: lengths read as zeros, then no end-of-block
    bits(*dyn_header({}), (0, 300)),                   # ... with enough bits for all of them
    bits(*dyn_header({0: 1, 16: 1}), (1, 1), (0, 2), (0, 16)),  # a repeat (16 = code 1) with nothing to repeat
    bits(*dyn_header({0: 1, 18: 1}), (1, 1), (127, 7), (1, 1), (127, 7), (0, 16)),  # 138 + 138 zeros: past HLIT + HDIST
    bits(*dyn_header({1: 1, 18: 1}), (0, 1), (1, 1), (127, 7), (1, 1), (108, 7), (0, 40)),  # lens[0] = 1, no end-of-block
    bits(*dyn_header({1: 1, 18: 1}), (1, 1), (127, 7), (1, 1), (107, 7), (0, 1), (0, 1), (1, 1), (0, 40)),  # one-bit codes: EOB
    bits(*dyn_header({0: 1, 1: 1}, hlit=30), (0, 16)),  # HLIT = 287
    bits(*dyn_header({0: 1, 1: 1}, hdist=30), (0, 16)),  # HDIST = 31
    bits(*FIXED),                                      # a fixed block with no symbol at all
    bits((0, 1), (1, 2), EOB),                         # a non-final empty fixed block, then nothing
    b"",
]


def test_inflate_core_against_zlib_under_sanitizer(driver, tmp_path):
    cases = make_streams()
    classes = {c for _, c, _ in cases}
    assert classes == {R.OK, R.S_TRUNCATED, R.S_INVALID, R.S_TRAILING}
    blob = struct.pack("<II", len(cases), _lib.SYZSIG_INFLATE_MAX_OUT)
    for s, cls, out in cases:
        blob += struct.pack("<III", len(s), cls, len(out)) + s + out
    p = tmp_path / "cases.bin"
    p.write_bytes(blob)
    out = run_driver(driver, "inflate", str(p))
    got = [int(line.split()[0]) for line in out[:len(cases)]]
    assert got == [c for _, c, _ in cases]
    # the block counts of three known shapes
    shapes = {tuple(int(x) for x in line.split()[1:]) for line in out[:len(cases)]}
    assert {(3, 0, 0), (2, 1, 0), (2, 0, 1)} <= shapes  # stored / fixed / dynamic, each + Flush + Close


def test_inflate_core_too_long(driver, tmp_path):
    """The cap is the caller's: with 1000 in place of SYZSIG_INFLATE_MAX_OUT, 1000 bytes pass and 1001 do not."""
    cases = []
    for n, cls in ((1000, R.OK), (1001, R.S_TOO_LONG)):
        for level, strategy in ((0, 0), (9, zlib.Z_FIXED), (9, 0)):
            d = (b"abcdefg" * 200)[:n]
            cases.append((R.go_stream(d, level, strategy), cls, d if cls == R.OK else b""))
    blob = struct.pack("<II", len(cases), 1000)
    for s, cls, out in cases:
        blob += struct.pack("<III", len(s), cls, len(out)) + s + out
    p = tmp_path / "long.bin"
    p.write_bytes(blob)
    run_driver(driver, "inflate", str(p))


def test_constants_match_header():
    txt = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    for name in ("SYZSIG_DB_END_EOF", "SYZSIG_DB_END_BAD_HEADER", "SYZSIG_DB_END_BAD_MAGIC", "SYZSIG_DB_END_TRUNCATED",
                 "SYZSIG_INFLATE_OK", "SYZSIG_INFLATE_TRUNCATED", "SYZSIG_INFLATE_INVALID", "SYZSIG_INFLATE_TRAILING",
                 "SYZSIG_INFLATE_TOO_LONG", "SYZSIG_INFLATE_LONG"):
        assert f"#define {name} {getattr(_lib, name)}\n" in txt, name
    assert "#define SYZSIG_INFLATE_MAX_OUT SYZSIG_HASH_MAX_MSG\n" in txt
    assert _lib.SYZSIG_INFLATE_MAX_OUT == _lib.SYZSIG_HASH_MAX_MSG
    assert [R.OK, R.S_TRUNCATED, R.S_INVALID, R.S_TRAILING, R.S_TOO_LONG] == list(range(5))
