"""CPU: tests/launch_caps.py against the sources it was read from and against the
plain reference loops.

The caps: each constant is held to the literal default or launch expression it
came from, so that a later change of a cap fails here instead of letting
tests/test_gpu_launch_caps.py quietly stop crossing it.  The helpers: the
pool-and-take expectations against tests/progtext_ref.py, tests/db_ref.py and
hashlib run element by element over a few thousand mixed elements, on every
output array; the whole-batch restatements of the keyed operations against the
plain loops, tests/dbw_ref.py's RefDB and the hand cases of tests/dbw_cases.py."""
import hashlib
import os
import re

import numpy as np
import pytest

from syzkaller_amd import db
from tests import db_ref as R
from tests import dbw_cases as C
from tests import dbw_ref as W
from tests import launch_caps as L
from tests import progtext_cases as PC
from tests import progtext_ref as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "syzkaller_amd", "csrc")


def squeeze(text):
    return " ".join(text.split())


def source(name):
    return squeeze(open(os.path.join(CSRC, name)).read())


# ---- the caps ----

def test_caps_match_the_sources():
    for name, text in L.SOURCES:
        assert squeeze(text) in source(name), (name, text)
    assert L.CAP_GRID_FOR == 2048 * 256 == 524288
    assert L.CAP_PC_WAVES == (1 << 16) * 4 == 262144
    assert L.CAP_PC_LONG == 1024 * 64 == L.CAP_SU_GATHER == L.CAP_REC_WRITE == 65536


@pytest.mark.parametrize("name", ["calls.hip", "db.hip", "sigs.hip"])
def test_every_grid_for_launch_is_256_threads_and_the_default_cap(name):
    """grid_for(rows, 256) with no third argument, on 256 threads: an element per thread and 2048 workgroups"""
    src = source(name)
    calls = re.findall(r"(k_\w+)(?:<[^<>]*>)?<<<grid_for\((.*?)\), (\w+), 0,", src)
    assert calls and len(calls) == src.count("grid_for(")
    for kernel, args, threads in calls:
        assert args.endswith(", 256") and threads == "256", kernel
        depth = 0
        for ch in args[: -len(", 256")]:  # (the row count may hold a comma inside brackets, none outside)
            depth += (ch == "(") - (ch == ")")
            assert not (ch == "," and depth == 0), kernel
    launched = {k for k, _, _ in calls}
    assert set(L.GRID_FOR_KERNELS.get(name, [])) <= launched
    for kernel in launched:  # ... and each of them strides by the whole grid
        body = src[src.index("void " + kernel + "("):]
        assert "const uint64_t T = (uint64_t)gridDim.x * blockDim.x" in body[:1500], kernel


def test_a_changed_cap_is_noticed(tmp_path):
    """the same check over a copy of a source with one literal edited"""
    for name, old, new in (("internal.h", "max_blocks = 2048", "max_blocks = 4096"),
                           ("calls.hip", "(nprog + 3) / 4, 1u << 16", "(nprog + 3) / 4, 1u << 17"),
                           ("calls.hip", "/ 64, 1024)", "/ 64, 2048)"),
                           ("calls.hip", "grid_cap(nprog, 1u << 16)", "grid_cap(nprog, 1u << 18)"),
                           ("db.hip", "grid_cap(n, 1u << 16)", "grid_cap(n)")):
        text = open(os.path.join(CSRC, name)).read()
        assert old in text
        (tmp_path / name).write_text(text.replace(old, new))
        edited = squeeze((tmp_path / name).read_text())
        assert any(squeeze(t) not in edited for f, t in L.SOURCES if f == name), (name, old)


# ---- placement ----

def test_place_keeps_the_rule_and_the_rare_spots():
    for n, nclass, caps, rare in ((L.CAP_PC_WAVES + 5, 7, (L.CAP_PC_WAVES, L.CAP_SU_GATHER), (2, 3, 4, 5, 6)),
                                  (L.CAP_GRID_FOR + 3, 4, (L.CAP_GRID_FOR,), (0, 3)),
                                  (L.CAP_GRID_FOR + 3, 6, (L.CAP_GRID_FOR,), (0, 1)),
                                  (L.CAP_REC_WRITE + 3, 4, (L.CAP_REC_WRITE,), (0, 1))):
        kind = L.place(n, nclass, caps, rare)
        for c in caps:
            assert L.crosses(kind, c)
            assert all(int(kind[at]) in rare for at in (c - 1, c, c + 1, n - 1))
        assert np.bincount(kind).min() > n // nclass - 8
    assert not L.crosses(np.arange(20) % 5, 10) and L.crosses(np.arange(20) % 3, 10) and not L.crosses(np.arange(10), 10)


def test_ragged_take():
    items = [b"abc", b"", b"z", b"0123456789"]
    rng = np.random.default_rng(1)
    kind = rng.integers(0, 4, 3000)
    flat, off = L.ragged_take(items, kind)
    assert flat.tobytes() == b"".join(items[k] for k in kind)
    assert off.tolist() == [0] + np.cumsum([len(items[k]) for k in kind]).tolist()
    flat, off = L.ragged_take([[], [7], [1, 2]], [2, 0, 1, 2], np.int32)
    assert flat.dtype == np.int32 and flat.tolist() == [1, 2, 7, 1, 2] and off.tolist() == [0, 2, 2, 3, 5]
    flat, off = L.ragged_take([b"", b""], [0, 1, 0])
    assert flat.size == 0 and off.tolist() == [0, 0, 0, 0]


# ---- program text ----

WIN = 256
TEXT_POOL = [b"getpid()\n", b"open()\nclose()\n", b"nosuch()\n", b"read()\n", b"foo", b"", b"#c\n", b"r0 = open(0x0)\r\nopen()",
             b"\n\n", b"n" * WIN + b"()\n", b"u" * WIN + b"()\n", b"#" + b"x" * (WIN + 1) + b"\n", b"n" * (WIN + 2) + b"\n",
             b"getpid" + b" " * (WIN - 6) + b"()\n"]
TEXT_NAMES = PC.NAMES + [b"n" * WIN]


@pytest.mark.parametrize("mode", [0, 1])
def test_prog_calls_expect_against_the_plain_loop(mode):
    rng = np.random.default_rng(mode)
    kind = rng.integers(0, len(TEXT_POOL), 4000)
    enabled = [1] * len(TEXT_NAMES)
    enabled[PC.READ] = 0
    e = L.prog_calls_expect(TEXT_POOL, kind, TEXT_NAMES, mode, enabled, WIN)
    progs = [TEXT_POOL[k] for k in kind]
    off, ids, status, err, flag = P.batch(progs, TEXT_NAMES, mode, enabled)
    assert e["blob"].tobytes() == b"".join(progs)
    assert e["off"].tolist() == [0] + np.cumsum([len(p) for p in progs]).tolist()
    assert (e["call_off"].tolist(), e["ids"].tolist()) == (off, ids)
    assert (e["status"].tolist(), e["err_line"].tolist(), e["flag"].tolist()) == (status, err, flag)
    lns = [ln for p in progs for ln, _ in P.lines(p)]
    nskip = sum(P.skipped(ln) for ln in lns)
    nlist = sum(len(ln) >= WIN and not P.skipped(ln) for ln in lns)  # (the pool's long lines all have their '(' past the window)
    assert e["stats"] == (len(lns), nskip, len(lns) - nskip - nlist, nlist) and nlist > 500
    assert len(set(status)) >= 3 and {0, 1} <= set(flag)


def test_listed_takes_the_two_forms_only():
    assert not L.listed(b"getpid()", WIN) and not L.listed(b"#" + b"x" * 1000, WIN) and not L.listed(b"", WIN)
    assert not L.listed(b"a" * (WIN - 2), WIN)
    assert L.listed(b"a" * WIN + b"()", WIN) and L.listed(b"a" + b" " * WIN + b"()", WIN) and L.listed(b"a" * WIN, WIN)
    for ln in (b"a" * (WIN - 1), b"a(" + b"x" * WIN, b"a = b" + b" " * WIN):
        with pytest.raises(ValueError):
            L.listed(ln, WIN)


# ---- streams, frames, hashes ----

VALS = [b"", b"q", b"abcabcabcabcabcabcabcabc", bytes(np.random.default_rng(7).integers(0, 256, 80, dtype=np.uint8)),
        b"r0 = openat$dir(0xffffffffffffff9c, &(0x7f0000000000)='./file0\\x00', 0x0, 0x0)\n" * 3]


@pytest.mark.parametrize("stream", [R.go_stream, db.deflate_host])
def test_deflate_and_records_expect_against_the_plain_loop(stream):
    rng = np.random.default_rng(2)
    n = 3000
    kind = rng.integers(0, len(VALS) + 1, n)  # len(VALS): a delete
    e = L.deflate_expect(VALS, kind[kind < len(VALS)], stream)
    vals = [VALS[k] for k in kind if k < len(VALS)]
    streams = [stream(v) if v else b"" for v in vals]
    assert e["src"].tobytes() == b"".join(vals) and e["out"].tobytes() == b"".join(streams)
    assert e["src_off"].tolist() == np.cumsum([0] + [len(v) for v in vals])[:-1].tolist()
    assert e["src_len"].tolist() == [len(v) for v in vals]
    assert e["out_off"].tolist() == np.cumsum([0] + [len(s) for s in streams]).tolist()
    forms = [L.stream_form(s) for s in streams if s]
    assert e["stats"] == (len(forms), 0, forms.count("stored"), forms.count("fixed"))
    assert L.deflate_expect(VALS, kind[kind < len(VALS)], stream, long_bytes=30)["stats"][:2] == \
        (sum(0 < len(v) <= 30 for v in vals), sum(len(v) > 30 for v in vals))
    # the frames
    sigs = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    seqs = rng.integers(0, 1 << 62, n, dtype=np.uint64) * np.uint64(2) + (np.arange(n) & 1).astype(np.uint64)
    seqs[kind == len(VALS)] = np.uint64(L.DEL)
    data, off = L.records_expect(VALS, kind, sigs, seqs, stream)
    want = [R.serialize_record(bytes(s).hex().encode(), VALS[k] if k < len(VALS) else None, int(q), stream)
            for s, k, q in zip(sigs, kind, seqs)]
    assert data.tobytes() == b"".join(want) and off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    sdata, soff = L.stream_pair(VALS, kind, stream)
    every = [stream(VALS[k]) if k < len(VALS) and VALS[k] else b"" for k in kind]
    assert sdata.tobytes() == b"".join(every) and soff.tolist() == np.cumsum([0] + [len(s) for s in every]).tolist()


def test_host_streams_of_the_pool_have_the_forms_their_names_say():
    """one byte and a short repeat go out as a fixed block, 80 bytes of noise stored"""
    assert [L.stream_form(db.deflate_host(v)) for v in VALS[1:4]] == ["fixed", "fixed", "stored"]


def test_hash_expect_against_the_plain_loop():
    rng = np.random.default_rng(3)
    base = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in (0, 1, 55, 56, 64, 65)]
    kind = rng.integers(0, 6, 5000)
    counter = (kind >= 2) & (rng.random(5000) < 0.5)
    data, off, dig = L.hash_expect(base, kind, counter)
    msgs = [(i.to_bytes(4, "little") + base[k][4:]) if c else base[k] for i, (k, c) in enumerate(zip(kind, counter))]
    assert data.tobytes() == b"".join(msgs) and off.tolist() == np.cumsum([0] + [len(m) for m in msgs]).tolist()
    assert dig.tobytes() == b"".join(hashlib.sha1(m).digest() for m in msgs)


# ---- the keyed operations ----

def rand_sigs(rng, n, distinct, unique=False):
    """n Sigs out of `distinct`, which differ in one byte next to a seam of the three sort words or in the last"""
    pool = np.full((distinct, 20), 0x55, np.uint8)
    pool[np.arange(distinct), np.array([0, 7, 8, 15, 16, 19])[np.arange(distinct) % 6]] = rng.integers(0, 256, distinct)
    pool[:, 3] = np.arange(distinct) // 6
    out = pool[rng.integers(0, distinct, n)]
    return np.unique(out, axis=0) if unique and n else out


def test_set_restatements_against_the_loops():
    rng = np.random.default_rng(4)
    for n, m in ((0, 0), (1, 0), (700, 0), (900, 300), (2000, 50)):
        sigs, have = rand_sigs(rng, n, 200), rand_sigs(rng, m, 200, unique=True)
        held = {bytes(s) for s in have}
        seen = set(held)
        is_new, key, first, known = [], [], [], []
        numbered = {}
        for i, s in enumerate(bytes(x) for x in sigs):
            if s not in numbered:
                numbered[s] = len(numbered)
                first.append(i)
                known.append(s in held)
            key.append(numbered[s])
            is_new.append(s not in seen)
            seen.add(s)
        got_new, size = L.sigset_add(have, sigs)
        assert got_new.tolist() == is_new and size == len(seen)
        assert L.member(sigs, have).tolist() == [bytes(s) in held for s in sigs]
        k, f, kn = L.number_sigs(sigs, have)
        assert (k.tolist(), f.tolist(), kn.tolist()) == (key, first, known)
        # the order is memcmp's
        order, _ = L.sig_runs(sigs)
        assert [(bytes(sigs[i]), int(i)) for i in order] == sorted((bytes(s), i) for i, s in enumerate(sigs))


def test_db_live_against_the_replay():
    rng = np.random.default_rng(5)
    for n, nvalid in ((0, 0), (1, 1), (500, 500), (500, 431), (3000, 2999)):
        sigs = rand_sigs(rng, n, 120)
        seqs = rng.integers(0, 4, n).astype(np.uint64)
        seqs[rng.random(n) < 0.3] = np.uint64(L.DEL)
        last = {}
        for i in range(nvalid):  # db.go:185-200
            last.pop(bytes(sigs[i]), None)
            if int(seqs[i]) != L.DEL:
                last[bytes(sigs[i])] = i
        live = L.db_live(sigs, seqs, nvalid)
        assert np.flatnonzero(live).tolist() == sorted(last.values())


def apply_by_ref(live, ops):
    """(written, keep_live, keep_op, the RefDB afterwards) by tests/dbw_ref.RefDB, op by op"""
    ref = W.RefDB(3, {k: (v, s) for k, v, s in live}, stream=lambda v: b"\x03\x00")
    written, owner = [], {k: ("live", i) for i, (k, _, _) in enumerate(live)}
    for j, op in enumerate(ops):
        before = len(ref.log)
        ref.apply([op])
        written.append(len(ref.log) > before)
        if written[-1]:
            owner[op[0]] = ("op", j)
    kept = {owner[k] for k in ref.records}
    return written, [("live", i) in kept for i in range(len(live))], [("op", j) in kept for j in range(len(ops))], ref


def restated(live, ops):
    lv, ov = L.value_ids([v for _, v, _ in live], [v for _, v, _ in ops])
    sig = lambda rows: L.sigs_of_keys([k for k, _, _ in rows]) if rows else np.zeros((0, 20), np.uint8)  # noqa: E731
    return L.db_apply(sig(live), [s for _, _, s in live], lv, sig(ops), [s for _, _, s in ops], ov)


@pytest.mark.parametrize("name", sorted(C.APPLY))
def test_db_apply_restatement_on_the_hand_cases(name):
    live, ops, written, after = C.APPLY[name]
    w, kl, ko = restated(live, ops)
    assert np.flatnonzero(w).tolist() == written
    rows = [live[i] for i in np.flatnonzero(kl)] + [ops[j] for j in np.flatnonzero(ko)]
    assert [(k, v or b"", s) for k, v, s in rows] == after


def test_db_apply_restatement_against_refdb():
    rng = np.random.default_rng(6)
    keys = sorted({bytes(s).hex().encode() for s in rand_sigs(rng, 400, 400)})
    vals = [b"", b"a", b"ab", b"prog one\n", b"prog two\n"]
    for nl, m in ((0, 1), (1, 0), (150, 0), (0, 900), (150, 300), (150, 3000)):
        live = [(keys[i], vals[i % 5], int(i % 3)) for i in rng.permutation(len(keys))[:nl]]
        ops = []
        for _ in range(m):
            k = keys[int(rng.integers(len(keys)))]
            ops.append((k, None, L.DEL) if rng.random() < 0.3 else (k, vals[int(rng.integers(5))], int(rng.integers(3))))
        written, keep_live, keep_op, ref = apply_by_ref(live, ops)
        w, kl, ko = restated(live, ops)
        assert (w.tolist(), kl.tolist(), ko.tolist()) == (written, keep_live, keep_op)
        rows = [live[i] for i in np.flatnonzero(kl)] + [ops[j] for j in np.flatnonzero(ko)]
        assert [(k, (v or b"", s)) for k, v, s in rows] == list(ref.records.items())
        if m == 300:
            assert 0 < sum(written) < m and any(keep_live) and not all(keep_live)
