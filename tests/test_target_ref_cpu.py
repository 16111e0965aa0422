"""CPU: tests/target_ref.py, the restatement of write_coverage_signal<cover_t>
for the three KCOV targets, held to what exists to hold it to:

  - CHECK_X86 word for word to the compiled oracle and to every
    tests/golden/executor_*.npz (the reference executor's own output), which
    pins every line the three targets share;
  - PC32 and 0 to the same goldens through the low-word identity: hash, dedup
    and write_output take uint32 (executor.h:677, :693, :206), so on a trace
    whose PCs all pass the x86 check the signals are a function of the PCs' low
    words, whatever the width and the upper words;
  - the lines that differ (cover_check, the order and equality of the cover
    sort) to cases derived by hand in the comments below.

Then syzkaller_amd/targets.py's table, and csrc/edge_args.h as a stand-alone
program under ASan + UBSan (tests/edge_driver.cc)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_traces as ET
from tests import target_ref as TR
from tests.conftest import ROOT, golden_names, load_golden

X86_LO, X86_HI = 0xffffffff80000000, 0xffffffffff000000
H = TR.hash32


def _golden(name):
    fx = load_golden(name)
    return (fx["pcs"], fx["call_start"], fx["call_len"], fx["prog_call"]), (fx["exp_sigs"], fx["exp_cnt"],
                                                                              fx["exp_completed"])


def _same(got, exp, call_start, prog_call=None, x86_only=False):
    """(sigs, sig_cnt, completed) equal, signals compared inside each call's
    count.  x86_only: `exp` is the x86-checked result and `got` an unchecked
    target's, which agree on what the check lets through -- every call before
    a program's aborting call (the table went through the same signals up to
    there), and `completed` of the programs that did not abort."""
    sigs, cnt, comp = got
    esigs, ecnt, ecomp = exp
    calls = np.ones(len(call_start), bool)
    if x86_only:
        whole = ecomp == np.diff(np.asarray(prog_call, np.int64))
        calls[:] = False
        for p in range(len(ecomp)):
            calls[int(prog_call[p]):int(prog_call[p]) + int(ecomp[p])] = True
        comp, ecomp = comp[whole], ecomp[whole]
    np.testing.assert_array_equal(comp, ecomp)
    np.testing.assert_array_equal(cnt[calls], ecnt[calls])
    for c in np.flatnonzero(calls):
        s, n = int(call_start[c]), int(ecnt[c])
        np.testing.assert_array_equal(sigs[s:s + n], esigs[s:s + n], err_msg=f"call {c}")


def scramble_upper(pcs, seed=7):
    """The PCs' low words under random upper words (some zero, some all-ones)."""
    rng = np.random.default_rng(seed)
    up = rng.integers(0, 1 << 32, pcs.size, dtype=np.uint64)
    up[rng.random(pcs.size) < 0.1] = 0
    up[rng.random(pcs.size) < 0.1] = 0xFFFFFFFF
    return (up << np.uint64(32)) | (pcs & np.uint64(0xFFFFFFFF))


# ---- CHECK_X86 held to the compiled reference ----

@pytest.mark.parametrize("name", golden_names())
def test_check_x86_equals_reference_executor_goldens(name):
    tr, exp = _golden(name)
    _same(TR.exec_batch(*tr, TR.CHECK_X86), exp, tr[1])


def _trace_sets():
    out = {f"dense_{n}": lambda n=n: ET.flat(ET.dense_set(n)) for n in sorted(ET.HOME_SETS)}
    out["geometry"] = lambda: ET.flat(*ET.geometry_programs())
    out["abort_positions"] = lambda: ET.flat(*ET.abort_position_programs()[:2])
    out["stride"] = lambda: ET.flat(ET.stride_batch()[0])
    out["dup_heavy"] = ET.dup_heavy_batch
    return out


@pytest.mark.parametrize("name", sorted(_trace_sets()))
def test_check_x86_equals_oracle_on_edge_traces(name):
    tr = _trace_sets()[name]()
    _same(TR.exec_batch(*tr, TR.CHECK_X86), O.exec_batch(*tr), tr[1])


# ---- the low-word identity ----

def _identity(tr, exp):
    pcs = tr[0]
    _same(TR.exec_batch((pcs & np.uint64(0xFFFFFFFF)).astype(np.uint32), *tr[1:], TR.PC32), exp, tr[1], tr[3], True)
    _same(TR.exec_batch(scramble_upper(pcs), *tr[1:], 0), exp, tr[1], tr[3], True)


@pytest.mark.parametrize("name", golden_names())
def test_low_word_identity_on_goldens(name):
    _identity(*_golden(name))


@pytest.mark.parametrize("name", sorted(_trace_sets()))
def test_low_word_identity_on_edge_traces(name):
    tr = _trace_sets()[name]()
    _identity(tr, O.exec_batch(*tr))


# ---- hand-derived cases ----

def _one(pcs, target, table=None):
    pc32, check = TR.flags_of(target)
    r = TR.write_coverage_signal(pcs, pc32, check, table)
    return None if r is None else r[0]


def test_first_pc_zero_is_a_duplicate_of_the_empty_slot():
    """First PC 0: sig = 0 ^ prev(0) = 0, and dedup(0) finds table[0] == 0 ==
    sig at its first probe (:697), so the signal counts as a duplicate of the
    EMPTY slot and nothing is emitted.  Unreachable under the x86 check (PC 0
    fails it); new with the unchecked targets."""
    h0 = H(0)
    assert h0 != 0 and h0 % 8192 not in (0, 1, 2, 3)
    for t in (0, TR.PC32):
        assert _one([0], t) == []
        # [0, 0, x]: PC 1 = 0 has sig = 0 ^ hash(0) = h0, new at its home; PC 2 = x has
        # sig = x ^ hash(0) again (prev is hash of the PC, not of the signal)
        assert _one([0, 0, 0x1000], t) == [h0, 0x1000 ^ h0]
        # [0x2000, 0]: sig 0x2000 fills slot 0 (0x2000 % 8192 == 0); the zero PC's
        # signal is 0 ^ hash(0x2000), an ordinary nonzero signal
        assert _one([0x2000, 0], t) == [0x2000, H(0x2000)]
    assert _one([0], TR.CHECK_X86) is None


def test_zero_signal_against_a_filled_slot_zero():
    """One program, calls of one PC each (prev = 0, so sig = pc) on one table:
    0x2000, 0x2001, 0x2002, 0x2003 fill slots 0..3 (x % 8192 = 0..3).
      - with slot 0 alone filled, sig 0 probes slot 0 (0x2000: no match, not
        empty), then slot 1, which is empty == sig: a duplicate (:697);
      - with slots 0..3 filled no probe matches or is empty: the forced
        overwrite stores 0 at slot 0 (:704) and the signal 0 is emitted;
      - after that slot 0 holds 0 == sig: a duplicate again."""
    for t in (0, TR.PC32):
        table = [0] * 8192
        assert _one([0x2000], t, table) == [0x2000] and table[0] == 0x2000
        assert _one([0], t, table) == []
        for k in (1, 2, 3):
            assert _one([0x2000 + k], t, table) == [0x2000 + k]
        assert table[:4] == [0x2000, 0x2001, 0x2002, 0x2003]
        assert _one([0], t, table) == [0] and table[0] == 0
        assert _one([0], t, table) == []
    # the batch wrapper shares the table between a program's calls and starts the next program fresh
    pcs = np.array([0x2000, 0, 0x2001, 0x2002, 0x2003, 0, 0, 0], np.uint32)
    sigs, cnt, comp = TR.exec_batch(pcs, np.arange(8), np.ones(8, np.uint32), [0, 7, 8], TR.PC32)
    assert cnt.tolist() == [1, 0, 1, 1, 1, 1, 0, 0] and comp.tolist() == [7, 1]
    assert sigs.tolist() == [0x2000, 0, 0x2001, 0x2002, 0x2003, 0, 0, 0]


def test_pc_0x1000_first():
    """0x1000 < 0xffffffff80000000: doexit(0) under CHECK_X86; under PC32 and 0
    sig = 0x1000 ^ 0, home 0x1000 of an empty table: emitted."""
    assert _one([0x1000], TR.CHECK_X86) is None
    assert _one([0x1000], TR.PC32) == [0x1000]
    assert _one([0x1000], 0) == [0x1000]


def test_x86_range_boundaries():
    """The range is [0xffffffff80000000, 0xffffffffff000000): a call holding the
    upper bound aborts the program there under CHECK_X86 (completed = calls
    before it) and is an ordinary PC under 0."""
    k = 0xffffffff81000000
    pcs = np.array([k, k + 5, X86_HI, k + 10], np.uint64)
    cs, cl, pc = [0, 1, 3], [1, 2, 1], [0, 3]
    sigs, cnt, comp = TR.exec_batch(pcs, cs, cl, pc, TR.CHECK_X86)
    assert comp.tolist() == [1] and cnt.tolist() == [1, 0, 0]
    sigs, cnt, comp = TR.exec_batch(pcs, cs, cl, pc, 0)
    assert comp.tolist() == [3] and cnt.tolist() == [1, 2, 1]
    # call 1: (u32)(k + 5) ^ 0, then (u32)X86_HI ^ hash((u32)(k + 5)); call 2 starts from prev = 0
    lo = lambda x: x & 0xFFFFFFFF  # noqa: E731
    assert sigs.tolist() == [lo(k), lo(k + 5), lo(X86_HI) ^ H(lo(k + 5)), lo(k + 10)]
    for pc_, ok in ((X86_LO, True), (X86_LO - 1, False), (X86_HI - 1, True), (X86_HI, False), (2**64 - 1, False)):
        assert TR.cover_check(pc_, False, True) is ok
        assert TR.cover_check(pc_, False, False) is True
    assert TR.cover_check(0, True, False) is True


def _cover(pcs, target, dedup):
    pc32, check = TR.flags_of(target)
    return TR.write_coverage_signal(pcs, pc32, check, None, True, dedup)[1]


def test_cover_sorts_cover_t_then_truncates():
    """Target 0 with dedup: std::sort + std::unique on u64 (:520-521), then the
    truncation (:525-526).
      [0x1_00000009, 0x2_00000003]: already ascending as u64 -> low words [9, 3]
      (a sort of the low words would give [3, 9]);
      [0x2_00000005, 5, 0x1_00000005, 5]: sorted [5, 5, 0x1_00000005,
      0x2_00000005], unique drops one 5 -> low words [5, 5, 5] (a unique of the
      low words would leave [5]).
    The same traces as a 32-bit kernel writes them (their low words) under PC32:
    [9, 3] -> [3, 9]; [5, 5, 5, 5] -> [5]."""
    a = [0x100000009, 0x200000003]
    b = [0x200000005, 5, 0x100000005, 5]
    assert _cover(a, 0, True) == [9, 3]
    assert _cover(b, 0, True) == [5, 5, 5]
    assert _cover([x & 0xFFFFFFFF for x in a], TR.PC32, True) == [3, 9]
    assert _cover([x & 0xFFFFFFFF for x in b], TR.PC32, True) == [5]
    # without dedup: the truncation in trace order, for every target
    assert _cover(a, 0, False) == [9, 3] and _cover(b, 0, False) == [5, 5, 5, 5]
    assert _cover([9, 3], TR.PC32, False) == [9, 3] and _cover([5, 5, 5, 5], TR.PC32, False) == [5, 5, 5, 5]
    k = [0xffffffff81000010, 0xffffffff81000005, 0xffffffff81000010]
    assert _cover(k, TR.CHECK_X86, False) == [0x81000010, 0x81000005, 0x81000010]
    assert _cover(k, TR.CHECK_X86, True) == [0x81000005, 0x81000010]
    assert _cover(k, 0, True) == [0x81000005, 0x81000010]  # one upper word: the two orders agree


def test_cover_check_x86_equals_cover_ref_on_goldens():
    """The cover half under CHECK_X86 against tests/cover_ref.py, which the
    compiled reference pins (tests/golden/cover)."""
    from tests import cover_ref as CR

    for name in ("executor_abort", "executor_zero2"):
        tr, exp = _golden(name)
        for dedup in (True, False):
            got = TR.edge_cover(*tr, exp[2], TR.CHECK_X86, dedup, fill=7)
            want = CR.edge_cover(*tr, exp[2], dedup, fill=7)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])


# ---- syzkaller_amd/targets.py ----

def test_for_kernel_table():
    from syzkaller_amd import targets as T

    assert (T.PC32, T.CHECK_X86, T.LINUX_AMD64) == (1, 2, 2)
    assert T.for_kernel("linux", "amd64") == T.CHECK_X86
    assert T.for_kernel("linux", "386") == T.CHECK_X86
    assert T.for_kernel("linux", "386", kernel_64_bit=True) == T.CHECK_X86
    assert T.for_kernel("linux", "386", kernel_64_bit=False) == T.PC32
    assert T.for_kernel("linux", "arm") == T.PC32
    assert T.for_kernel("linux", "arm", kernel_64_bit=False) == T.PC32
    assert T.for_kernel("linux", "arm64") == 0
    assert T.for_kernel("linux", "ppc64le") == 0
    for os_ in ("freebsd", "netbsd", "fuchsia", "akaros", "windows"):
        assert T.for_kernel(os_, "amd64") == 0
    for os_, arch in (("linux", "mips64le"), ("darwin", "amd64"), ("freebsd", "386"), ("", "")):
        with pytest.raises(ValueError):
            T.for_kernel(os_, arch)
    with pytest.raises(ValueError):
        T.for_kernel("linux", "amd64", kernel_64_bit=False)  # no executor of the reference runs there
    assert [T.is_valid(t) for t in range(8)] == [True, True, True] + [False] * 5


# ---- csrc/edge_args.h on the CPU, under ASan + UBSan ----

def test_argument_checks_under_sanitizer(tmp_path):
    exe = str(tmp_path / "edge_driver")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra",
                        "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "edge_driver.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "0 failures" in r.stdout
