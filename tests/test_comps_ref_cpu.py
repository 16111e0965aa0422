"""CPU: tests/comps_ref.py, the restatement that checks the comparison-hints
kernels, held to cases worked out by hand from the reference lines it cites
(executor.h:576-593 / :823-875, executor_linux.cc:221-253, ipc.go:420-465,
hints.go:164-218); and the three entry points are bound."""
import numpy as np

from syzkaller_amd import _lib
from tests import comps_ref as R

OUT = 0x7f0000000000  # an output_data address
KM0, KM1 = 0xffff880000000000, 0xffff890000000000


def test_entry_points_bound():
    for n in ("syzsig_exec_comps_dev", "syzsig_comp_map_dev", "syzsig_shrink_expand_dev"):
        assert n in _lib.SIGNATURES


def test_sort_compares_type_as_u64_and_writes_its_low_word():
    # both types are SIZE2 in their low word; operator< orders the full u64
    w, n = R.call_comps([(0x100000002, 5, 6, 0), (2, 7, 8, 0)], OUT)
    assert (w, n) == ([2, 7, 8, 2, 5, 6], 2)


def test_duplicates_differing_in_pc_collapse():
    w, n = R.call_comps([(4, 10, 11, 1), (4, 10, 11, 2), (4, 10, 11, 1)], OUT)
    assert (w, n) == ([4, 10, 11], 1)


def test_unique_precedes_sign_extension():
    w, n = R.call_comps([(0, 0x1fe, 1, 0), (0, 0xfe, 1, 0)], OUT)
    assert (w, n) == ([0, 0xfffffffe, 1, 0, 0xfffffffe, 1], 2)


def test_write_sign_extends_from_the_size_and_orders_size8_lo_hi():
    assert R.write_comp(2, 0x8000, 0x7fff) == [2, 0xffff8000, 0x7fff]
    assert R.write_comp(4, 0x180000000, 1) == [4, 0x80000000, 1]
    assert R.write_comp(1, 0x17f, 0x80) == [1, 0x7f, 0xffffff80]  # SIZE1 | CONST
    assert R.write_comp(6, 0x1122334455667788, 0x99aabbccddeeff00) == [6, 0x55667788, 0x11223344, 0xddeeff00,
                                                                        0x99aabbcc]


def test_ignore_zero_branch():
    assert R.ignore(0, 0, 0, OUT)          # arg1 == 0 && arg2 == 0
    assert R.ignore(1, 0, 5, OUT)          # arg1 == 0 && const
    assert not R.ignore(0, 0, 5, OUT)      # not const, arg2 != 0
    assert not R.ignore(1, 5, 0, OUT)      # arg1 != 0
    assert R.ignore(7, 0, 5, OUT)          # SIZE8 | CONST


def test_ignore_output_region_inclusive_bounds_size8_only():
    end = OUT + (16 << 20)
    assert R.ignore(6, OUT, 1, OUT) and R.ignore(6, end, 1, OUT)
    assert not R.ignore(6, OUT - 1, 1, OUT) and not R.ignore(6, end + 1, 1, OUT)
    assert R.ignore(6, 1, OUT, OUT) and R.ignore(6, 1, end, OUT)
    assert not R.ignore(6, 1, end + 1, OUT)
    assert not R.ignore(4, OUT, 1, OUT)    # SIZE4: never a pointer


def test_ignore_kernel_pointer_branches():
    assert R.ignore(6, KM0, KM1, OUT)                    # both ends inclusive
    assert not R.ignore(6, KM0 - 1, KM1, OUT)            # only arg2 a kernel pointer, arg1 != 0
    assert not R.ignore(6, KM0, KM1 + 1, OUT)
    assert R.ignore(6, KM0, 0, OUT)                      # kptr1 && arg2 == 0
    assert R.ignore(6, 0, KM1, OUT)                      # kptr2 && arg1 == 0
    assert not R.ignore(6, KM1 + 1, 0, OUT)
    assert not R.ignore(2, KM0, KM1, OUT)                # SIZE2


def test_call_comps_skips_ignored_after_unique():
    recs = [(6, KM0, 0, 0), (0, 0, 0, 0), (2, 9, 3, 0), (6, OUT + 5, 1, 0)]
    assert R.call_comps(recs, OUT) == ([2, 9, 3], 1)
    assert R.call_comps([], OUT) == ([], 0)


def test_exec_comps_layout():
    comps = np.array([[2, 9, 3, 0], [2, 9, 3, 1], [6, 1, 2, 0], [0, 0, 0, 0]], np.uint64)
    out, nw, cnt = R.exec_comps(comps, [0, 2, 4], [2, 2, 0], OUT, fill=0xdead)
    assert out.tolist() == [2, 9, 3] + [0xdead] * 7 + [6, 1, 0, 2, 0] + [0xdead] * 5
    assert nw.tolist() == [3, 5, 0] and cnt.tolist() == [1, 1, 0]


def test_parse_zero_extends_small_operands():
    st, m = R.parse_comps([0, 0xfffffffe, 1], 0, 1)
    assert st == R.INGEST_OK and m == {1: {0xfffffffe}, 0xfffffffe: {1}}


def test_parse_size8_equal_dropped_and_const_bit():
    st, m = R.parse_comps([6, 0x55667788, 0x11223344, 2, 0, 0, 7, 7, 1, 3, 9], 0, 3)
    assert st == R.INGEST_OK
    assert m == {2: {0x1122334455667788}, 0x1122334455667788: {2}, 9: {3}}  # [0,7,7] dropped; const: only op2 -> op1


def test_parse_statuses():
    assert R.parse_comps([0, 1, 2], 0, 2) == (R.INGEST_ECOMPS, {})        # no type word for record 1
    assert R.parse_comps([6, 1, 0, 2], 0, 1) == (R.INGEST_ECOMPS, {})     # SIZE8 with three operand words
    assert R.parse_comps([0, 1], 0, 1) == (R.INGEST_ECOMPS, {})
    assert R.parse_comps([0, 1, 2, 8, 1, 2], 0, 2) == (R.INGEST_ECOMPTYPE, {})
    assert R.parse_comps([0, 1, 2, 0, 3, 4], 0, 2, end=5) == (R.INGEST_ECOMPS, {})  # the region ends first
    st, off, pairs, _ = R.comp_map([0, 1, 2, 8], [0, 3], [1, 1])
    assert st.tolist() == [0, R.INGEST_ECOMPTYPE] and off.tolist() == [0, 2, 2]
    assert pairs.tolist() == [[1, 2], [2, 1]]


def test_swap_int_truncates():
    assert R.swap_int(0xffffffffffff8001, 2) == 0x0180
    assert R.swap_int(0x11223344, 4) == 0x44332211
    assert R.swap_int(0x1122334455667788, 8) == 0x8877665544332211
    assert R.swap_int(0xabc, 1) == 0xabc


def test_shrink_expand_width8_mask():
    v = 0x1122334455667788
    assert R.shrink_expand(v, {v: {0xdeadbeefcafef00d}}) == [0xdeadbeefcafef00d]


def test_shrink_expand_shrink_matches():
    assert R.shrink_expand(0x1234, {0x34: {0xab}}) == [0x12ab]                 # width 1
    assert R.shrink_expand(0xaa1234, {0x3412: {0xcdab}}) == [0xaaabcd]         # width 2, big-endian
    assert R.shrink_expand(0x1234, {0x34: {0x1ab}}) == []                      # the other operand is wider
    assert R.shrink_expand(0x1234, {0x34: {0xffffffffffffff80}}) == [0x1280]   # ... unless its high part is all ones


def test_shrink_expand_expand_matches():
    m64 = (1 << 64) - 1
    assert R.shrink_expand(0xff, {m64: {0x05}}) == [0x05]                      # width -1: 0xff | ^0xff
    assert R.shrink_expand(0xff, {m64: {m64 - 1}}) == [0xfe]
    # width -2 big-endian: swapInt truncates the expanded mutant to 0x8001 first;
    # width 2 big-endian meets the same key: one replacer
    assert R.shrink_expand(0x8001, {0x0180: {0x2211}}) == [0x1122]
    assert R.shrink_expand(0x8001, {0x0180ffffffffffff: {0x2211}}) == []


def test_shrink_expand_special_ints_and_dedup():
    assert R.shrink_expand(0x1234, {0x34: {0x40}}, [0x40]) == []
    assert R.shrink_expand(0x1234, {0x34: {0x40}}, [0x41]) == [0x1240]
    assert R.shrink_expand(0x34, {0x34: {0xab}}) == [0xab]                     # widths 8, 4, 2, 1 agree
    assert R.shrink_expand(0x34, {0x34: {0x34}}) == [0x34]                     # equal to v: not excluded
    off, rep = R.shrink_expand_batch([{0x34: {0xab, 0xcd}}, {}], [0, 1, 0], [0x1234, 0x1234, 0x34])
    assert off.tolist() == [0, 2, 2, 4] and rep.tolist() == [0x12ab, 0x12cd, 0xab, 0xcd]
