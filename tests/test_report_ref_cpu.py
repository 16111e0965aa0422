"""CPU: tests/report_ref.py -- the manager's coverage-page loops restated in
Python -- held to the hand-derived cases of tests/report_cases.py, and
csrc/report_args.h run as a stand-alone program under ASan + UBSan."""
import os
import subprocess

import pytest

from tests import report_cases as C
from tests import report_ref as R
from tests.conftest import ROOT


@pytest.mark.parametrize("case", C.UNCOVERED, ids=[c[0] for c in C.UNCOVERED])
def test_uncovered_hand_cases(case):
    _, syms, allc, pcs, want = case
    assert R.uncovered_pcs_in_funcs(syms, allc, pcs) == want


def test_two_orders_differ():
    by = {c[0]: c for c in C.UNCOVERED}
    for a, b in (("two_order_ab", "two_order_ba"), ("alias_short_first", "alias_long_first"),
                 ("repeat_after_readd", "repeat_before_readd")):
        assert sorted(by[a][3]) == sorted(by[b][3]) and by[a][1:3] == by[b][1:3]  # the same pcs, another order
        assert by[a][4] != by[b][4]


def test_sort_search_is_gos_probe_sequence():
    # monotone: the first true index, n when none
    assert [R.sort_search(5, lambda i, k=k: i >= k) for k in range(7)] == [0, 1, 2, 3, 4, 5, 5]
    # not monotone: ends (100, 30, 50), pc 25: h=1 true, h=0 true -> 0; pc 60: h=1 false, h=2 false -> 3
    ends = [100, 30, 50]
    probes = []
    assert R.sort_search(3, lambda i: probes.append(i) or 25 < ends[i]) == 0 and probes == [1, 0]
    probes.clear()
    assert R.sort_search(3, lambda i: probes.append(i) or 60 < ends[i]) == 3 and probes == [1, 2]
    assert R.sort_search(0, lambda i: True) == 0


@pytest.mark.parametrize("case", C.REPORT_PCS, ids=[c[0] for c in C.REPORT_PCS])
def test_report_pcs_hand_cases(case):
    _, arch, base, pcs, order, srt = case
    assert R.report_pcs(pcs, base, arch) == (order, srt)


def test_report_pcs_unknown_arch_and_text():
    with pytest.raises(RuntimeError):
        R.report_pcs([1], 0, "mips")
    assert R.raw_cover_text([0x1006, 0x1009, 0x1005], 0, "arm") == "0x1002\n0x1002\n0x1006\n"
    assert R.raw_cover_text([3, 10], 0, "amd64") == "0x5\n0xfffffffffffffffe\n"


def test_syscall_info_hand_case():
    got = R.collect_syscall_info(C.CORPUS)
    assert {k: (v[0], len(v[1])) for k, v in got.items()} == C.SYSCALL_INFO
    assert "open" not in got  # a call without inputs is no key of the Go map
    assert got["write"] == [1, set()]  # an input with an empty cover still counts


def test_http_cover_selection():
    assert R.http_cover(C.CORPUS) == {1, 2, 3, 9}
    assert R.http_cover(C.CORPUS, call="read") == {1, 2, 3}
    assert R.http_cover(C.CORPUS, call="write") == set()  # merged into, but empty: "No coverage data available"
    assert R.http_cover(C.CORPUS, call="open") is None  # nil: no input matched
    assert R.http_cover(C.CORPUS, input="d") == {1, 9}
    assert R.http_cover(C.CORPUS, input="a", call="mmap") == {1, 2}  # input wins over call
    with pytest.raises(KeyError):
        R.http_cover(C.CORPUS, input="zz")


# ---- csrc/report_args.h on the CPU, under ASan + UBSan ----

def test_argument_checks_under_sanitizer(tmp_path):
    exe = str(tmp_path / "report_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "report_driver.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "0 failures" in r.stdout
