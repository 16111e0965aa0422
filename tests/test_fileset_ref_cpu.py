"""CPU: tests/fileset_ref.py -- fileSet, the line walk, parseFile's line count
and templateFileArray.Less restated in Python -- held to the hand-derived
cases of tests/fileset_cases.py; the closed form of the walk against its loop;
the host helpers of syzkaller_amd.report; and syzsig_file_set_dev's checks in
csrc/report_args.h run as a stand-alone program under ASan + UBSan."""
import os
import random
import subprocess

import pytest

from syzkaller_amd import report
from tests import fileset_cases as C
from tests import fileset_ref as R
from tests.conftest import ROOT


@pytest.mark.parametrize("case", C.FILE_SET, ids=[c[0] for c in C.FILE_SET])
def test_file_set_hand_cases(case):
    _, cov, unc, nlines, want, want_walk = case
    got = R.file_set(cov, unc)
    assert got == want
    assert {f: R.walk(nlines[f], lst) for f, lst in got.items()} == want_walk
    assert {f: R.walk_closed(nlines[f], lst) for f, lst in got.items()} == want_walk


def test_file_set_ignores_order_within_a_list_but_not_between():
    by = {c[0]: c for c in C.FILE_SET}
    _, cov, unc, _, want, _ = by["repeats"]
    assert R.file_set(cov[::-1], unc[::-1]) == want
    # the two lists are not interchangeable: swapped, line 3 is covered and line 1 is not
    assert R.file_set(unc, cov) != want


def test_walk_closed_form_is_the_loop():
    rng = random.Random(1)
    for _ in range(4000):
        nlines = rng.randrange(0, 12)
        lines = sorted(rng.sample(range(-3, 16), rng.randrange(0, 9)))
        lst = [(ln, rng.random() < 0.5) for ln in lines]
        assert R.walk_closed(nlines, lst) == R.walk(nlines, lst), (nlines, lst)


@pytest.mark.parametrize("data,n", [(b"", 0), (b"\n", 1), (b"a", 1), (b"a\n", 1), (b"a\nb", 2), (b"a\nb\n", 2),
                                    (b"\n\n", 2), (b"\n\nx", 3), (b"a\r\nb\r\n", 2)])
def test_parse_file_nlines(data, n):
    assert R.parse_file_nlines(data) == n
    assert report.parse_file_nlines(data) == n


def test_parse_file_nlines_random():
    rng = random.Random(2)
    for _ in range(500):
        data = bytes(rng.choice(b"ab\n") for _ in range(rng.randrange(0, 30)))
        assert report.parse_file_nlines(data) == R.parse_file_nlines(data) == len(data.split(b"\n")) - (
            1 if data.endswith(b"\n") or not data else 0)


@pytest.mark.parametrize("case", C.FILE_ORDER, ids=[str(i) for i in range(len(C.FILE_ORDER))])
def test_file_order_hand_cases(case):
    names, want = case
    assert R.file_order(names) == want
    assert report.file_order(names) == want
    assert all(not R.less(b, a) for a, b in zip(want, want[1:]))


def test_file_order_random():
    rng = random.Random(3)
    alphabet = ["", ".", "a", "/", "z", ".a"]
    for _ in range(300):
        names = list({"".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 4))) for _ in range(8)})
        assert report.file_order(names) == R.file_order(names)


# ---- csrc/report_args.h on the CPU, under ASan + UBSan ----

def test_argument_checks_under_sanitizer(tmp_path):
    exe = str(tmp_path / "fileset_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "fileset_driver.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "0 failures" in r.stdout
