"""CPU: the restated heads of program-text lines (tests/progtext_ref.py) against
hand-derived cases (tests/progtext_cases.py), the agreement of the two modes on
head-grammar lines, and csrc/calls_core.h + calls_args.h under ASan + UBSan."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import calltab_keys as K
from tests import progtext_cases as C
from tests import progtext_ref as R
from tests.conftest import ROOT

TABLE = R.table_of(C.NAMES)


def _check(case):
    name, text, des, cs = case
    st, el, ids, dis = R.prog_calls(text, TABLE)
    assert (st, el, ids) == des and dis == 0, name
    st, el, ids, sup, unk = R.call_set(text, TABLE)
    assert (st, el, ids, unk) == cs, name
    assert sup == int(st == R.OK and not unk), name


@pytest.mark.parametrize("case", C.CASES, ids=[c[0] for c in C.CASES])
def test_hand_cases(case):
    _check(case)


def test_long_line_boundary():
    for case in C.long_line_cases():
        _check(case)


def test_lines():
    assert R.lines(b"") == []
    assert R.lines(b"a") == [(b"a", 1)]
    assert R.lines(b"a\n") == [(b"a", 1)]
    assert R.lines(b"a\n\n") == [(b"a", 1), (b"", 0)]
    assert R.lines(b"\n") == [(b"", 0)]
    assert R.lines(b"a\r\nb\r") == [(b"a", 2), (b"b", 2)]
    assert R.lines(b"a\r\r\n") == [(b"a\r", 3)]  # one "\r" is dropped, not all
    assert R.lines(b"a\n\r") == [(b"a", 1), (b"", 1)]  # a last run of "\r" is a line (empty after the drop)


def test_enabled_flags():
    en = [1] * len(C.NAMES)
    en[C.OPEN] = 0
    assert R.prog_calls(C.SIX, TABLE, en) == (R.OK, 0, [C.GETPID, C.OPEN, C.GETPID, C.CLOSE_FOO], 1)
    assert R.prog_calls(b"getpid()\n", TABLE, en)[3] == 0
    assert R.call_set(C.SIX, TABLE, en)[3:] == (0, 0)
    assert R.call_set(b"getpid()\nnosuch()\n", TABLE, en)[3:] == (0, 1)
    assert R.call_set(b"getpid()\n", TABLE, en)[3:] == (1, 0)
    assert R.prog_calls(b"open()\nfoo\n", TABLE, en) == (R.BAD_HEAD, 2, [], 0)  # defined only for OK programs
    assert R.load_corpus([b"getpid()\n", b"open()\n", b"(\n", b""], C.NAMES, en) == ([2], [1], [0, 3])


def test_modes_agree_on_head_grammar_lines():
    """On a line that matches I W* ('=' W* I W*)? '(' the Deserialize name is the
    CallSet span stripped of W at both ends: 10^4 random lines."""
    rng = np.random.default_rng(20181015)
    ident = b"abcXYZ019_$"
    ws = [b"", b" ", b"\t", b"  ", b" \t", b"\t "]

    def I():
        return bytes(ident[int(k)] for k in rng.integers(0, len(ident), int(rng.integers(1, 9))))

    def W():
        return ws[int(rng.integers(0, len(ws)))]

    for _ in range(10000):
        name = I()
        ln = name + W()
        if rng.integers(0, 2):
            name = I()
            ln = I() + W() + b"=" + W() + name + W()
        ln += b"(" + [b"", b")", b"0x0, r1=x)", b" = ("][int(rng.integers(0, 4))]
        st, got = R.head_deserialize(ln)
        assert (st, got) == (R.OK, name), ln
        st, span = R.head_callset(ln)
        assert st == R.OK and span.strip(b" \t") == name, ln


def test_calltab_keys():
    assert K.name_hash(b"") == K.fmix64(0xCBF29CE484222325)
    assert K.slots_for(1) == 2 and K.slots_for(64) == 128 and K.slots_for(65) == 256 and K.slots_for(5000) == 16384
    names = K.colliding_names(64, 128, slot=5)
    assert len(set(names)) == 64 and all(K.home(n, 128) == 5 for n in names)
    a = K.absent_name(names, 128, slot=5)
    assert a not in names and K.home(a, 128) == 5


# ---- csrc/calls_core.h and calls_args.h on the CPU, under ASan + UBSan ----

def _pack_cases(cases, names):
    out = [struct.pack("<I", len(names))]
    for n in names:
        out.append(struct.pack("<I", len(n)) + n)
    out.append(struct.pack("<I", len(cases)))
    for _, text, des, cs in cases:
        out.append(struct.pack("<I", len(text)) + text)
        out.append(struct.pack("<4I", des[0], des[1], 0, len(des[2])) + struct.pack("<%dI" % len(des[2]), *des[2]))
        flag = (int(cs[0] == R.OK and not cs[3]) | cs[3] << 1) if cs[0] == R.OK else 0
        out.append(struct.pack("<4I", cs[0], cs[1], flag, len(cs[2])) + struct.pack("<%dI" % len(cs[2]), *cs[2]))
    return b"".join(out)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("progtext") / "progtext_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "progtext_driver.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "\n0 failures" in "\n" + r.stdout
    return r.stdout


def test_argument_checks_under_sanitizer(driver):
    _run(driver, "args")


def test_core_on_hand_cases_under_sanitizer(driver, tmp_path):
    """Every hand case, the 2^20 boundary, and every prefix of the six-line
    program (expected from the restatement, which the hand cases pin), each from a
    heap block of exactly its size."""
    cases = list(C.CASES) + C.long_line_cases()
    for n in range(len(C.SIX) + 1):
        p = C.SIX[:n]
        d, c = R.prog_calls(p, TABLE), R.call_set(p, TABLE)
        cases.append(("six[:%d]" % n, p, d[:3], (c[0], c[1], c[2], c[4])))
    path = tmp_path / "cases.bin"
    path.write_bytes(_pack_cases(cases, C.NAMES))
    out = _run(driver, "cases", str(path))
    assert "%d cases" % len(cases) in out
