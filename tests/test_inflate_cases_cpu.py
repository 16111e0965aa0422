"""CPU: the hand-written DEFLATE streams of tests/inflate_cases.py.  First the
writer's own check -- zlib reads every base stream to eof with nothing left over
and returns the bytes that the token lists spell (tests/deflate_writer.spell reads
tokens, never bits) -- then csrc/inflate_core.h over the whole case list in
tests/db_driver.cc, a stand-alone program under ASan + UBSan, against zlib."""
import struct
import zlib

import numpy as np
import pytest

from syzkaller_amd import _lib
from tests import db_ref as R
from tests import deflate_writer as W
from tests import inflate_cases as IC
from tests.test_db_ref_cpu import driver, run_driver  # noqa: F401  (driver: the fixture)


def zlib_exact(stream):
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data and not d.unconsumed_tail
    return out


# ---- the writer ----

def test_bit_sink_orders_and_repeat():
    w = W.BitWriter()
    w.bits(0b1, 1)
    w.bits(0b10, 2)       # LSB first: bit 1 = 0, bit 2 = 1
    w.huff(0b110, 3)      # MSB first: bits 3, 4, 5 = 1, 1, 0
    w.bits(0b01, 2)
    assert w.getvalue() == bytes([0b01011101])
    for k, v in ((2, 1), (3, 5), (5, 19), (8, 200), (7, 1)):
        for lead in range(8):
            for count in (0, 1, 7, 8, 9, 100):
                a, b = W.BitWriter(), W.BitWriter()
                a.bits(0, lead)
                b.bits(0, lead)
                a.repeat(v, k, count)
                for _ in range(count):
                    b.bits(v, k)
                assert (a.getvalue(), a.n) == (b.getvalue(), b.n)


def test_canonical_is_the_rfc_example():
    # RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111
    assert W.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]
    assert W.canonical([0, 1, 0]) == [None, 0, None]
    assert W.canonical(W.FIXED_LL)[0] == 0b00110000 and W.canonical(W.FIXED_LL)[256] == 0


def test_random_complete_lengths():
    rng = np.random.default_rng(3)
    for nsym in (2, 3, 19, 30, 257, 286):
        for maxlen in (9, 15):
            lens = W.random_complete_lengths(rng, nsym, maxlen)
            assert len(lens) == nsym and W.kraft(lens) == 1 << 15 and 1 <= min(lens) and max(lens) <= maxlen
    assert W.random_complete_lengths(rng, 1) == [1]
    assert max(max(W.random_complete_lengths(rng, 286)) for _ in range(20)) == 15


def test_rle_ops_spell_their_lengths():
    rng = np.random.default_rng(4)
    for _ in range(50):
        lens = [int(x) for x in rng.choice([0, 0, 0, 5, 5, 9], int(rng.integers(1, 400)))]
        for kw in ({}, {"zeros": False}, {"rep16": False}):
            assert W.expand_ops(W.rle_ops(lens, **kw)) == lens


@pytest.mark.parametrize("name", [c.name for c in IC.base_cases()])
def test_writer_against_zlib(name):
    case = {c.name: c for c in IC.base_cases()}[name]
    for s, blocks in ((case.short, IC.form_blocks(case, "short")), (case.long, IC.form_blocks(case, "long"))):
        if s is None:
            continue
        if not case.valid:
            assert R.inflate_class(s)[0] == R.S_INVALID
            continue
        assert zlib_exact(s) == IC.spelled(blocks)


def test_base_cases_are_what_their_names_say():
    by = {c.name: c for c in IC.base_cases()}
    dyn = lambda name: by[name].blocks[0][2]  # noqa: E731
    assert sorted(set(dyn("deep_all")["ll_lens"])) == [1, 2, 3, 4, 5, 6, 14, 15] and len(dyn("deep_all")["ll_lens"]) == 286
    assert max(dyn("deep_all")["d_lens"]) == 15 and len(dyn("deep_all")["d_lens"]) == 30
    assert 60000 < len(by["deep_all"].long) < 70000 and by["deep_all"].short is None
    assert any(s == 16 for s, _ in dyn("rle16")["cl_ops"])
    assert dyn("single_dist")["d_lens"] == [1] and dyn("no_dist")["d_lens"] == [0]
    assert len(IC.spelled(by["len284_31"].blocks)) == 259
    assert len(IC.spelled(by["bomb"].blocks)) == 1032001 and len(by["bomb"].short) < 1100
    assert [b[0] for b in by["fixed_reuse"].blocks] == ["fixed", "fixed", "stored", "fixed", "dynamic", "fixed", "dynamic",
                                                       "fixed"]
    assert len(by["alternating"].blocks) == 40 and IC.counts(by["alternating"].blocks) == (13, 13, 14)
    for i, (ops, at) in enumerate(((dyn("zeros_cross")["cl_ops"], 286), (dyn("rep16_cross")["cl_ops"], 259))):
        # one run starts below the nlen | ndist boundary and ends above it
        have, crossing = 0, []
        for s, e in ops:
            n = 1 if s < 16 else 3 + e if s < 18 else 11 + e
            if have < at < have + n:
                crossing.append(s)
            have += n
        assert crossing == [(18, 16)[i]]


def test_wave64_streams():
    w = IC.wave64(1)
    assert len(w) == 64 and len({s for s, _ in w}) == 64
    for s, spelled in w:
        assert len(s) <= IC.LONG and zlib_exact(s) == spelled
    hdr = lambda s: ((s[0] >> 3) + 257, (s[1] & 31) + 1)  # noqa: E731  (HLIT, HDIST of a first dynamic block)
    assert hdr(w[0][0]) == (286, 30) and hdr(w[1][0]) == (257, 1)
    assert len({hdr(s) for s, _ in w}) > 40


def test_cap_streams_against_zlib():
    """the four streams around SYZSIG_INFLATE_MAX_OUT: zlib reads each to eof and gives the length the blocks spell"""
    assert IC.MAX_OUT == _lib.SYZSIG_INFLATE_MAX_OUT and IC.LONG == _lib.SYZSIG_INFLATE_LONG
    for name, (s, n) in IC.cap_streams().items():
        assert 250000 < len(s) < 270000
        assert IC.zlib_length(s) == (True, n), name
    lens = {k: n - IC.MAX_OUT for k, (_, n) in IC.cap_streams().items()}
    assert lens == {"exact": 0, "literal_over": 1, "match_over": 158, "stored_over": 100}


# ---- csrc/inflate_core.h in tests/db_driver.cc under ASan + UBSan ----

def blob_of(cases, max_out):
    parts = [struct.pack("<II", len(cases), max_out)]
    for s, cls, out in cases:
        parts += [struct.pack("<III", len(s), cls, len(out)), s, out]
    return b"".join(parts)


def test_case_list_covers_every_class():
    cases = IC.all_cases()
    assert {c for _, _, c, _ in cases} == {R.OK, R.S_TRUNCATED, R.S_INVALID, R.S_TRAILING}
    for c in IC.base_cases():
        for s in (c.short, c.long):
            if s is not None:
                assert (R.inflate_class(s)[0] == R.OK) == (c.name != "no_dist_needed"), c.name


def test_inflate_core_on_the_case_list_under_sanitizer(driver, tmp_path):  # noqa: F811
    cases = IC.all_cases()
    p = tmp_path / "cases.bin"
    p.write_bytes(blob_of([c[1:] for c in cases], _lib.SYZSIG_INFLATE_MAX_OUT))
    out = run_driver(driver, "inflate", str(p))
    assert len(out) == len(cases) + 1
    got = [tuple(int(x) for x in line.split()) for line in out[:len(cases)]]
    assert [g[0] for g in got] == [c[2] for c in cases]
    # the block counts of the base streams, from the token lists
    at = {label: i for i, (label, _, _, _) in enumerate(cases)}
    for c in IC.base_cases():
        if not c.valid:
            continue
        if c.short is not None:
            assert got[at[c.name + "/short/0"]][1:] == IC.counts(c.blocks), c.name
        if c.long is not None:
            assert got[at[c.name + "/long/0"]][1:] == IC.counts(IC.form_blocks(c, "long")), c.name


def test_inflate_core_at_the_real_cap_under_sanitizer(driver, tmp_path):  # noqa: F811
    """With max_out = SYZSIG_INFLATE_MAX_OUT itself: a literal, a match and a stored
    block that cross 2^28 are TOO_LONG (counting decodes: no output is held)."""
    cases = [(s, R.S_TOO_LONG, b"") for name, (s, n) in IC.cap_streams().items() if n > IC.MAX_OUT]
    assert len(cases) == 3
    p = tmp_path / "cap.bin"
    p.write_bytes(blob_of(cases, _lib.SYZSIG_INFLATE_MAX_OUT))
    run_driver(driver, "inflate", str(p))
