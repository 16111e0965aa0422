"""CPU: the reference of the device hashing and Sig sets (tests/hash_ref.py)
against the FIPS 180 vectors and hand-derived cases of the three loops; the
host-side hex forms of syzkaller_amd.hashing; and the host-compilable halves of
csrc/sigs.hip -- csrc/sha1.h (the SHA-1 and both of the kernels' readers) and
csrc/sigs_args.h (the entry points' argument checks) -- in tests/sigs_driver.cc,
a stand-alone program built under ASan + UBSan."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from syzkaller_amd import _lib, hashing
from tests import hash_ref as R
from tests.conftest import ROOT

PAD_EDGES = (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 129)


def S(x):
    """a hand-made Sig: x repeated"""
    return bytes([x]) * 20


def test_fips_vectors_against_hashlib():
    for msg, hexd in R.FIPS_VECTORS:
        assert hashlib.sha1(msg).hexdigest() == hexd
        assert R.hash_string(msg) == hexd
        assert R.hash_sig(msg).hex() == hexd
    assert R.hash_sig(b"ab", b"", b"c") == R.hash_sig(b"abc")  # Hash(pieces...) = the concatenation's
    data, off = R.pack([m for m, _ in R.FIPS_VECTORS[:3]], lead=3)
    assert [s.hex() for s in R.as_sigs(R.hash_messages(data, off))] == [h for _, h in R.FIPS_VECTORS[:3]]


def test_add_inputs_hand_cases():
    h = set()
    # a duplicate inside a batch: only its first row is appended
    np.testing.assert_array_equal(R.add_inputs(h, [S(1), S(2), S(1), S(3), S(2)]), [1, 1, 0, 1, 0])
    assert h == {S(1), S(2), S(3)}
    # a Sig already present
    np.testing.assert_array_equal(R.add_inputs(h, [S(3), S(4)]), [0, 1])
    assert h == {S(1), S(2), S(3), S(4)}
    np.testing.assert_array_equal(R.add_inputs(h, []), [])


def test_hub_sync_hand_cases():
    hub, sent = R.hub_connect([S(5), S(2), S(5)])
    assert hub == {S(2), S(5)} and sent.tolist() == [1, 1, 1]  # Connect sends every program
    # corpus gained 7 (twice) and 1, lost 5 and 2... and kept 9 that the hub never had
    hub = {S(2), S(5), S(8)}
    add, dels = R.hub_sync(hub, [S(7), S(8), S(7), S(1)])
    assert add.tolist() == [1, 0, 0, 1]
    assert dels == [S(2), S(5)]  # Del in ascending order
    assert hub == {S(1), S(7), S(8)}
    add, dels = R.hub_sync(hub, [])
    assert add.tolist() == [] and dels == [S(1), S(7), S(8)] and hub == set()


def test_number_sigs_hand_cases():
    key, first, known, n = R.number_sigs([S(9), S(3), S(9), S(1), S(3)], known={S(3), S(4)})
    assert key.tolist() == [0, 1, 0, 2, 1] and first == [0, 1, 3] and known == [0, 1, 0] and n == 3
    assert R.number_sigs([])[3] == 0


def test_sig_string_round_trip_and_bad_length():
    sig = R.hash_sig(b"abc")
    s = hashing.to_string(sig)
    assert s == "a9993e364706816aba3e25717850c26c9cd0d89d"
    assert hashing.from_string(s) == sig
    assert hashing.to_string(np.frombuffer(sig, np.uint8)) == s
    for bad in (s[:-2], s + "00", "", s[:-1], "zz" * 20, s[:20] + " " + s[20:]):
        with pytest.raises(ValueError):
            hashing.from_string(bad)
    with pytest.raises(ValueError):
        hashing.to_string(sig[:19])
    assert hashing.SIG_BYTES == _lib.SYZSIG_SIG_BYTES == hashlib.sha1().digest_size


def test_constants_match_header():
    txt = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    for name in ("SYZSIG_SIG_BYTES", "SYZSIG_HASH_STAGE", "SYZSIG_HASH_LONG", "SYZSIG_SIGSET_TILE"):
        assert f"#define {name} {getattr(_lib, name)}\n" in txt, name
    assert "#define SYZSIG_HASH_MAX_MSG (1ull << 28)" in txt and _lib.SYZSIG_HASH_MAX_MSG == 1 << 28


# ---- csrc/sha1.h and csrc/sigs_args.h on the CPU, under ASan + UBSan ----

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sigs_driver") / "sigs_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "sigs_driver.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "0 failures" in r.stdout
    return r.stdout.split()


def test_argument_checks_under_sanitizer(driver):
    run_driver(driver, "args")


def hash_file(tmp_path, msgs, shift):
    data, off = R.pack(msgs)
    p = tmp_path / f"msgs_{shift}.bin"
    p.write_bytes(struct.pack("<II", len(msgs), shift) + off.astype("<u8").tobytes() + data.tobytes())
    return str(p)


def test_sha1_readers_under_sanitizer(driver, tmp_path):
    rng = np.random.default_rng(5)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in PAD_EDGES + (2, 3, 4, 5, 200, 4095, 4097)]
    exp = [hashlib.sha1(m).hexdigest() for m in msgs]
    for shift in range(16):
        out = run_driver(driver, "hash", hash_file(tmp_path, msgs, shift))
        assert out[: len(msgs)] == exp, shift
        assert "staged" in out  # the span fits: the staging reader ran too and agreed
    # the FIPS vectors; the long one from memory only
    out = run_driver(driver, "hash", hash_file(tmp_path, [m for m, _ in R.FIPS_VECTORS], 1))
    assert out[:4] == [h for _, h in R.FIPS_VECTORS] and "staged" not in out
