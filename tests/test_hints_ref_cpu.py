"""CPU: tests/hints_ref.py (checkConstArg / checkDataArg, prog/hints.go:105-132)
held to outcomes worked out by hand from the cited lines, and the pieces of
syzsig_hint_mutants_dev that need no GPU (the exported symbols, the binding,
the header's constants, apply_mutant)."""
import os
import re
import subprocess

import pytest

from syzkaller_amd import _lib
from syzkaller_amd.hints import apply_mutant
from tests import hints_ref as H
from tests.conftest import ROOT

M64 = (1 << 64) - 1
SPECIAL = (0x40, 0x100)  # one list for every case: the device test runs them as one batch


def blob(n, **at):
    """n zero bytes with byte k set to v for every b<k>=v"""
    b = bytearray(n)
    for k, v in at.items():
        b[int(k[1:])] = v
    return bytes(b)


# (name, arg: an int = ConstArg.Val / bytes = DataArg.Data(), map, [(at, nb, replacer)], [the mutated bytes])
HAND = [
    # :107-109: one shrinkExpand of Val; width 1 of 0x1234 finds 0x34
    ("const_one", 0x1234, {0x34: {0xab}}, [(0, 8, 0x12ab)], None),
    # the replacers of one key, ascending
    ("const_several", 0x1234, {0x34: {0xab, 0xcd, 0x05}}, [(0, 8, 0x1205), (0, 8, 0x12ab), (0, 8, 0x12cd)], None),
    # :202-204: 0x40 is in the list, 0x41 is not
    ("const_special", 0x1234, {0x34: {0x40, 0x41}}, [(0, 8, 0x1241)], None),
    # window 0 of an 8-byte blob is 0x8877665544332211; its low 1, 2, 4 and 8 bytes are keys; no other window's are
    ("data_widths", bytes.fromhex("1122334455667788"),
     {0x11: {0xa1}, 0x2211: {0xb2b1}, 0x44332211: {0xc4c3c2c1}, 0x8877665544332211: {0xd8d7d6d5d4d3d2d1}},
     [(0, 8, 0x88776655443322a1), (0, 8, 0x887766554433b2b1), (0, 8, 0x88776655c4c3c2c1), (0, 8, 0xd8d7d6d5d4d3d2d1)],
     ["a122334455667788", "b1b2334455667788", "c1c2c3c455667788", "d1d2d3d4d5d6d7d8"]),
    # nine bytes 0x5a: width 1 finds the key at every offset; window i holds min(8, 9 - i) bytes (:122-124), and the
    # last one is 0x5a at widths 8, 4, 2 and 1: one replacer
    ("data_every_offset", b"\x5a" * 9, {0x5a: {0x7e}},
     [(0, 8, 0x5a5a5a5a5a5a5a7e), (1, 8, 0x5a5a5a5a5a5a5a7e), (2, 7, 0x5a5a5a5a5a5a7e), (3, 6, 0x5a5a5a5a5a7e),
      (4, 5, 0x5a5a5a5a7e), (5, 4, 0x5a5a5a7e), (6, 3, 0x5a5a7e), (7, 2, 0x5a7e), (8, 1, 0x7e)],
     ["7e" + "5a" * 8, "5a7e" + "5a" * 7, "5a5a7e" + "5a" * 6, "5a" * 3 + "7e" + "5a" * 5, "5a" * 4 + "7e" + "5a" * 4,
      "5a" * 5 + "7e" + "5a" * 3, "5a" * 6 + "7e5a5a", "5a" * 7 + "7e5a", "5a" * 8 + "7e"]),
    # window 2 is 0xfe; -1 expands it to 0xff..fe (:175), the key of a comparison -2 == -5 whose other operand
    # has an all-ones high part (:196) and leaves 0xfb; the zero windows find no key 0
    ("data_expand_middle", bytes.fromhex("0000fe0000"), {M64 - 1: {M64 - 4}}, [(2, 3, 0xfb)], ["0000fb0000"]),
    # window 0 is 0x78563412: big-endian at width 4 it is 0x12345678 (:190), and the value comes back swapped
    # (:199-201); at width 2 it is 0x1234, whose value 0x0001 swaps to the special 0x0100 and 0x00aa to 0xaa00.
    # (The big-endian expands -4 and -2 reach the same keys, swapInt truncates: the same replacers.)
    ("data_big_endian", bytes.fromhex("12345678"), {0x12345678: {0xcafebabe}, 0x1234: {0x0001, 0x00aa}},
     [(0, 4, 0x7856aa00), (0, 4, 0xbebafeca)], ["00aa5678", "cafebabe"]),
    # the last window of three bytes is 0xc3 zero-padded: width 8 accepts the full-width value, widths 4, 2, 1
    # find the key too and drop the value for its high part (:196); one byte of the replacer is written (:127)
    ("data_last_window", bytes.fromhex("0102c3"), {0xc3: {0x1122334455667788}}, [(2, 1, 0x1122334455667788)],
     ["010288"]),
    # 101 bytes: window 99 reads bytes 99 and 100 (the pad comes from the length, :123); byte 100 alone (0xe2) is
    # a key, but the loop ends at maxDataLength (:118-121)
    ("data_101", blob(101, b99=0xe1, b100=0xe2), {0xe2e1: {0x0b0a}, 0xe2: {0x99}}, [(99, 2, 0x0b0a)],
     [blob(101, b99=0x0a, b100=0x0b).hex()]),
    # 108 bytes: window 99 is the full 8 bytes 99 .. 106; window 100 (bytes 100 .. 107) would match, and is not run
    ("data_108", blob(108, b99=0xf1, b100=0xf2, b101=0xf3, b102=0xf4, b103=0xf5, b104=0xf6, b105=0xf7, b106=0xf8),
     {0xf8f7f6f5f4f3f2f1: {0x0102030405060708}, 0x00f8f7f6f5f4f3f2: {0x77}}, [(99, 8, 0x0102030405060708)],
     [blob(108, b99=8, b100=7, b101=6, b102=5, b103=4, b104=3, b105=2, b106=1).hex()]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_restatement_hand_cases(case):
    _, arg, m, exp, applied = case
    if isinstance(arg, int):
        assert H.check_const_arg(arg, m, SPECIAL) == exp
        return
    got = H.check_data_arg(arg, m, SPECIAL)
    assert got == exp
    assert [H.apply(arg, *g).hex() for g in got] == applied
    assert [apply_mutant(arg, *g).hex() for g in got] == applied


def test_special_list_decides():
    assert H.check_const_arg(0x1234, {0x34: {0x40, 0x41}}, ()) == [(0, 8, 0x1240), (0, 8, 0x1241)]
    assert H.check_data_arg(bytes.fromhex("12345678"), {0x1234: {0x0001}}, ()) == [(0, 4, 0x78560100)]


def test_window_cap_and_no_window_100():
    m = {0x5a: {0x7e}}
    for n in (99, 100, 101, 108, 300):
        r = H.check_data_arg(b"\x5a" * n, m)
        assert [x[0] for x in r] == list(range(min(n, 100)))
        assert [x[1] for x in r] == [min(8, n - i) for i in range(min(n, 100))]
    assert H.check_data_arg(b"", m) == []


def test_batch_form_orders_args_windows_replacers():
    maps = [{0x34: {0xab, 0x05}}, {}, {0x5a: {0x7e}}]
    off, at, nb, rep = H.hint_mutants(maps, [2, 0, 1, 0], [1, 0, 0, 1], [0, 0x1234, 0x1234, 0], [0, 2, 2, 2, 3],
                                      b"\x5a\x5a\x34")
    assert off.tolist() == [0, 2, 4, 4, 6]
    assert at.tolist() == [0, 1, 0, 0, 0, 0] and nb.tolist() == [2, 1, 8, 8, 1, 1]
    assert rep.tolist() == [0x5a7e, 0x7e, 0x1205, 0x12ab, 0x05, 0xab]


def test_apply_mutant_truncates_and_checks():
    assert apply_mutant(b"\x01\x02\x03", 1, 2, 0x1122334455667788) == b"\x01\x88\x77"
    assert apply_mutant(b"", 0, 0, 5) == b""
    with pytest.raises(ValueError):
        apply_mutant(b"\x01\x02", 1, 2, 0)


def test_library_exports_and_binds_hint_mutants():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (syzsig_\w+)", out))
    assert {"syzsig_hint_mutants_dev", "syzsig_hint_mutants_stats"} <= exported
    assert {"syzsig_hint_mutants_dev", "syzsig_hint_mutants_stats"} <= set(_lib.SIGNATURES)
    assert _lib.lib().syzsig_hint_mutants_dev is not None
    hdr = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    assert int(re.search(r"#define SYZSIG_HINT_LIST (\d+)", hdr).group(1)) == _lib.SYZSIG_HINT_LIST
    assert int(re.search(r"#define SYZSIG_HINT_MAX_DATA (\d+)", hdr).group(1)) == _lib.SYZSIG_HINT_MAX_DATA == H.MAX_DATA_LENGTH
