"""GPU: syzsig_prog_calls_dev and syzkaller_amd.progtext against tests/progtext_ref.py
(prog/encoding.go's line heads restated), exactly, on every output.  Every
expected value comes from the restatement or is written out by hand
(tests/progtext_cases.py), none from the device; output buffers are pre-filled so
that an unwritten or overwritten entry shows; the paths taken are asserted from
syzsig_prog_calls_stats.  W = the window, T = the tile of text per workgroup, S =
the sort tile of CallSet's dedup."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, db, prio, progtext
from tests import calltab_keys as K
from tests import db_ref
from tests import prio_ref
from tests import progtext_cases as C
from tests import progtext_ref as R
from tests.test_gpu_prio import assert_same

pytestmark = pytest.mark.gpu

W, T, S = progtext.WINDOW, progtext.TILE, progtext.SORT_TILE
DES, CS = progtext.DESERIALIZE, progtext.CALLSET
FILL = 0xCD
BIG = [b"sys_%d" % i for i in range(5000)]


@pytest.fixture(scope="module")
def tab(gpu):
    return progtext.CallTable(gpu, C.NAMES)


@pytest.fixture(scope="module")
def bigtab(gpu):
    return progtext.CallTable(gpu, BIG)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def raw(gpu, tab_h, blob, off, mode, enabled=None, cap=None, null_ids=False, need=0):
    """One call with every output pre-filled: -> (rc, total, coff, ids, status, err_line, flag) as numpy."""
    n = len(off) - 1
    data = (torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(gpu.dev) if blob
            else torch.empty(0, dtype=torch.uint8, device=gpu.dev))
    d_off = torch.from_numpy(np.asarray(off, np.int64)).to(gpu.dev)
    cap = need if cap is None else cap
    coff = torch.full((n + 2,), -1, dtype=torch.int64, device=gpu.dev)
    ids = torch.full((cap + 1,), -1, dtype=torch.int32, device=gpu.dev)
    status = torch.full((n + 1,), FILL, dtype=torch.uint8, device=gpu.dev)
    err = torch.full((n + 1,), -1, dtype=torch.int32, device=gpu.dev)
    flag = torch.full((n + 1,), FILL, dtype=torch.uint8, device=gpu.dev)
    en = None if enabled is None else torch.from_numpy(np.asarray(enabled, np.uint8)).to(gpu.dev)
    total = ctypes.c_uint64(12345)
    torch.cuda.synchronize()
    rc = gpu.L.syzsig_prog_calls_dev(gpu.eng.h, tab_h, _p(data), len(blob), _p(d_off), n, mode, _p(en), _p(coff),
                                     None if null_ids else ctypes.c_void_p(ids.data_ptr()), 0 if null_ids else cap,
                                     _p(status), _p(err), _p(flag), ctypes.byref(total))
    return (rc, total.value, coff.cpu().numpy(), ids.cpu().numpy(), status.cpu().numpy(), err.cpu().numpy(),
            flag.cpu().numpy())


def check(gpu, table, names, progs, mode, enabled=None, blob=None, off=None):
    """The batch against the restatement on every output, sentinels intact; -> stats."""
    if blob is None:
        blob = b"".join(progs)
        off = np.concatenate([[0], np.cumsum([len(p) for p in progs])]).astype(np.int64)
    else:
        progs = [blob[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    eoff, eids, est, eerr, eflag = R.batch(progs, names, mode, enabled)
    n = len(progs)
    rc, total, coff, ids, status, err, flag = raw(gpu, table.h, blob, off, mode, enabled, need=len(eids))
    assert rc == 0, gpu.L.syzsig_last_error()
    assert total == len(eids)
    assert status[:n].tolist() == est and status[n] == FILL
    assert err[:n].tolist() == eerr and err[n] == -1
    assert coff[: n + 1].tolist() == eoff and coff[n + 1] == -1
    assert ids[:total].tolist() == eids and ids[total] == -1, "ids differ or written past total"
    assert flag[:n].tolist() == eflag and flag[n] == FILL
    st = progtext.stats(gpu)
    nlines = sum(len(R.lines(p)) for p in progs)
    assert st[0] == nlines
    return st


# ---- the hand cases ----

@pytest.mark.parametrize("mode", [DES, CS])
def test_hand_cases_each_alone_and_as_one_batch(gpu, tab, mode):
    for name, text, des, cs in C.CASES:
        rc, total, coff, ids, status, err, flag = raw(gpu, tab.h, text, [0, len(text)], mode, need=8)
        exp = des if mode == DES else cs
        assert rc == 0 and (status[0], err[0], ids[:total].tolist()) == exp[:3], name
        if mode == CS:
            assert flag[0] == ((int(not cs[3]) | cs[3] << 1) if cs[0] == R.OK else 0), name
        else:
            assert flag[0] == 0, name
    # back to back: a program without a final newline is followed directly by the next one's bytes
    check(gpu, tab, C.NAMES, [c[1] for c in C.CASES], mode)


@pytest.mark.parametrize("mode", [DES, CS])
def test_the_2_20_boundary_and_a_megabyte_line_between_neighbours(gpu, tab, mode):
    cases = C.long_line_cases()
    for name, text, des, cs in cases[:6]:
        rc, total, coff, ids, status, err, flag = raw(gpu, tab.h, text, [0, len(text)], mode, need=8)
        exp = des if mode == DES else cs
        assert rc == 0 and (status[0], err[0], ids[:total].tolist()) == exp[:3], name
    st = check(gpu, tab, C.NAMES, [b"getpid()\n"] + [c[1] for c in cases[5:]] + [b"open()"], mode)
    if mode == CS:
        assert st[3] >= 1  # " " * 2^20 has no '(' in its window: listed, and not scanned


# ---- the window ----

@pytest.mark.parametrize("mode", [DES, CS])
def test_bracket_and_name_at_the_window_edge(gpu, mode):
    lens = (W - 1, W, W + 1)
    names = [b"getpid"] + [b"n" * k for k in lens]
    table = progtext.CallTable(gpu, names)
    for o in lens:  # '(' at line offset o: the head ends inside the window iff o < W
        prog = b"getpid" + b" " * (o - 6) + b"()\n"
        st = check(gpu, table, names, [b"#c\n" + prog + b"getpid()\n"], mode)
        assert st == (3, 1, 2 - (o >= W), int(o >= W))
    for k in lens:  # a name of k bytes has its '(' at offset k
        st = check(gpu, table, names, [b"n" * k + b"(0x0)\n", b"r0 = " + b"n" * k + b"()"], mode)
        assert st == (2, 0, 0 if k >= W else 1, 2 if k >= W else 1)
    # a '\r' as the window's last byte is undecided: it may be the line's end
    st = check(gpu, table, names, [b"getpid" + b" " * (W - 7) + b"\r\nopen()\n", b"#" + b"x" * 3 * W + b"\n"], mode)
    assert st[3] == 1
    table.free()


# ---- tile seams ----

def _filler(n):
    """a comment line of exactly n bytes, newline included (n >= 2)"""
    return b"#" + b"x" * (n - 2) + b"\n"


@pytest.mark.parametrize("mode", [DES, CS])
def test_tile_seams(gpu, tab, mode):
    # a '\n' as the last byte of a tile = a line start as the first byte of the next
    p = _filler(T) + b"getpid()\n" + _filler(T - 13) + b"open"  # "open" ends tile 1: its line ends with the program
    assert len(p) == 2 * T
    check(gpu, tab, C.NAMES, [p, b"(0x0)\n"], mode)
    # "\r\n" split across two tiles: a line that is just "\r", and one that ends in it
    check(gpu, tab, C.NAMES, [_filler(T - 1) + b"\r\ngetpid()\n"], mode)
    check(gpu, tab, C.NAMES, [_filler(T - 4) + b"foo\r\ngetpid()\n"], mode)
    check(gpu, tab, C.NAMES, [_filler(T - 9) + b"getpid()\r", b"\nopen()\n"], mode)  # the '\n' is the next program's
    # a head that crosses the seam, and one whose window ends in the next tile
    check(gpu, tab, C.NAMES, [_filler(T - 3) + b"r0 = close$foo(0x0)\n", _filler(T - 23 - 100) + b"getpid" + b" " * 150 + b"()"],
          mode)


@pytest.mark.parametrize("mode", [DES, CS])
def test_program_boundary_at_every_byte_alignment(gpu, tab, mode):
    """The previous program lacks a final newline and the next starts with a
    valid head: the line stops at off[i + 1] ("getpid" is BAD_HEAD / NO_BRACKET;
    run on, it would read "getpidgetpid2()")."""
    progs, at = [], 0
    for a, mod in [(x, 16) for x in range(16)] + [(T - 1, T), (0, T), (1, T)]:
        pad = (a - at - 6) % mod
        pad += mod if pad < 2 else 0
        prev = _filler(pad) + b"getpid"
        progs += [prev, b"getpid2()\n"]
        at += len(prev) + 10
    off = np.concatenate([[0], np.cumsum([len(p) for p in progs])])
    ends = {int(o) % 16 for o in off[1::2][:16]}
    assert ends == set(range(16)) and {int(o) % T for o in off[1::2][16:]} == {T - 1, 0, 1}
    check(gpu, tab, C.NAMES, progs, mode)
    # the text does not start at data[0] and does not end at nbytes: the bytes outside belong to no program
    blob = b"getpid()\nopen(" + b"".join(progs) + b")\nclose()\n"
    check(gpu, tab, C.NAMES, None, mode, blob=blob, off=off + 14)


# ---- batch shapes ----

@pytest.mark.parametrize("mode", [DES, CS])
def test_batch_shapes(gpu, tab, mode):
    rc, total, coff, ids, status, err, flag = raw(gpu, tab.h, b"", [0], mode)
    assert rc == 0 and total == 0 and coff[0] == 0 and coff[1] == -1 and status[0] == FILL
    check(gpu, tab, C.NAMES, [b"getpid()\n"], mode)
    check(gpu, tab, C.NAMES, [b"", b"", b"getpid()\n", b"", b"open()", b"", b"", b"close()\n", b""], mode)
    check(gpu, tab, C.NAMES, [b""] * 700, mode)
    rng = np.random.default_rng(3)
    one = [[b"getpid()\n", b"r0 = open(0x0)\n", b"nosuch()\n", b"#c\n", b"\n", b"close$foo()"][int(k)]
           for k in rng.integers(0, 6, 4000)]
    st = check(gpu, tab, C.NAMES, one, mode)
    assert st[3] == 0
    lines = [[b"getpid()\n", b"r0 = open(0x0, 0x1)\n", b"#c\n", b"\n", b"close$foo(r0)\n"][int(k)]
             for k in rng.integers(0, 5, 5000)]
    check(gpu, tab, C.NAMES, [b"open()\n", b"".join(lines), b"close()\n"], mode)
    bad = list(lines)
    bad[4321] = b"foo\n"
    check(gpu, tab, C.NAMES, [b"".join(bad)], mode)


# ---- the table ----

def test_table_lookups(gpu, bigtab):
    nslots = K.slots_for(64)
    names = K.colliding_names(64, nslots, slot=7)
    table = progtext.CallTable(gpu, names)
    assert len(table) == 64
    absent = K.absent_name(names, nslots, slot=7)
    progs = [n + b"()\n" for n in names] + [absent + b"()\n", b"".join(n + b"(0x0)\n" for n in reversed(names))]
    for mode in (DES, CS):
        check(gpu, table, names, progs, mode)
    table.free()
    one = progtext.CallTable(gpu, [b"x"])
    for mode in (DES, CS):
        check(gpu, one, [b"x"], [b"x()\n", b"y()\n", b"xx()\n", b"r0 = x()"], mode)
    one.free()
    rng = np.random.default_rng(5)
    progs = [b"".join(BIG[int(k)] + b"(0x1)\n" for k in rng.integers(0, 5000, 12)) for _ in range(300)]
    progs.append(b"sys_5000()\n")
    progs.append(b"".join(n + b"()\n" for n in BIG))
    for mode in (DES, CS):
        check(gpu, bigtab, BIG, progs, mode)
    for bad in ([b"a", b""], [b"a", b"b", b"a"], []):
        with pytest.raises(_lib.SyzsigError) as e:
            progtext.CallTable(gpu, bad)
        assert e.value.code == _lib.SYZSIG_EINVAL


def test_callset_dedup_around_the_sort_tile(gpu, bigtab):
    rng = np.random.default_rng(7)
    progs = []
    for k in (S - 1, S, S + 1, 2 * S + 3):
        order = rng.permutation(k)
        order = np.concatenate([order, order[: k // 3]])  # a third of them twice
        progs.append(b"".join(BIG[int(i)] + b"()\n" for i in order))
    progs.append(b"sys_77(0x0)\n" * 10000)
    progs.append(b"sys_3()\nsys_1()\nsys_3()\n")
    check(gpu, bigtab, BIG, progs, CS)
    check(gpu, bigtab, BIG, progs, DES)


@pytest.mark.parametrize("mode", [DES, CS])
def test_enabled(gpu, tab, mode):
    progs = [C.SIX, b"getpid()\n", b"open()\nnosuch()\n", b"", b"foo\n", b"close()\nclose$foo()\n"]
    n = len(C.NAMES)
    one_off = [1] * n
    one_off[C.OPEN] = 0
    for en in (None, [1] * n, [0] * n, one_off):
        check(gpu, tab, C.NAMES, progs, mode, enabled=en)
    with pytest.raises(ValueError):
        progtext.prog_calls(gpu, tab, progs, enabled=[1] * (n - 1))


# ---- capacity and errors ----

@pytest.mark.parametrize("mode", [DES, CS])
def test_capacity(gpu, tab, mode):
    progs = [C.SIX, b"getpid()\nopen()\n", b"foo\n"]
    blob, off = b"".join(progs), np.concatenate([[0], np.cumsum([len(p) for p in progs])])
    eoff, eids, est, eerr, eflag = R.batch(progs, C.NAMES, mode)
    need = len(eids)
    # the sizing call: everything but the ids
    rc, total, coff, ids, status, err, flag = raw(gpu, tab.h, blob, off, mode, null_ids=True)
    assert rc == 0 and total == need and coff[:4].tolist() == eoff and status[:3].tolist() == est
    assert err[:3].tolist() == eerr and flag[:3].tolist() == eflag and (ids == -1).all()
    # one short: the needed count, and nothing written
    rc, total, coff, ids, status, err, flag = raw(gpu, tab.h, blob, off, mode, cap=need - 1)
    assert rc == _lib.SYZSIG_ERANGE and total == need
    assert (coff == -1).all() and (ids == -1).all() and (status == FILL).all() and (err == -1).all() and (flag == FILL).all()
    # exact
    rc, total, coff, ids, status, err, flag = raw(gpu, tab.h, blob, off, mode, cap=need)
    assert rc == 0 and ids[:need].tolist() == eids and ids[need] == -1


def test_error_paths(gpu, tab):
    blob = b"getpid()\nopen()\n"
    for off in ([0, 9, 8], [0, 9, 17], [5, 3, 16], [0, 1 << 40, 16]):
        rc, total, coff, ids, status, err, flag = raw(gpu, tab.h, blob, off, DES, need=4)
        assert rc == _lib.SYZSIG_EINVAL, off
        assert (coff == -1).all() and (ids == -1).all() and (status == FILL).all()
    assert raw(gpu, tab.h, blob, [0, 9, 16], 2, need=4)[0] == _lib.SYZSIG_EINVAL
    assert raw(gpu, None, blob, [0, 9, 16], DES, need=4)[0] == _lib.SYZSIG_EINVAL
    assert raw(gpu, tab.h, blob, [0, 9, 16], DES, need=4)[0] == 0


# ---- a random batch ----

@pytest.mark.parametrize("mode", [DES, CS])
def test_random_batch_with_corrupted_lines(gpu, bigtab, mode):
    rng = np.random.default_rng(20181015 + mode)
    en = (rng.random(5000) < 0.9).astype(np.uint8)
    progs = []
    for _ in range(20000):
        lines = R.gen_program(rng, BIG, int(rng.integers(2, 9))).split(b"\n")[:-1]
        for k in np.flatnonzero(rng.random(len(lines)) < 0.02):
            ln = bytearray(lines[k])
            ln[int(rng.integers(0, len(ln)))] = int(rng.integers(0, 256))
            lines[k] = bytes(ln)
        progs.append(b"\n".join(lines) + (b"\n" if rng.random() < 0.9 else b""))
    check(gpu, bigtab, BIG, progs, mode, enabled=en.tolist())


# ---- corpus.db bytes -> priorities -> choice table ----

def test_chain_from_corpus_db_to_choice_table(gpu):
    rng = np.random.default_rng(9)
    names = [b"sys_%d" % i for i in range(40)]
    ncalls = len(names)
    table = progtext.CallTable(gpu, names)
    enabled = np.ones(ncalls, np.uint8)
    enabled[[3, 17]] = 0
    vals = [R.gen_program(rng, names, int(rng.integers(1, 12))) for _ in range(120)]
    for k in (5, 50, 90):
        vals[k] = vals[k] + b"nosuch$call(0x0)\n"  # broken
    vals[60] = b"sys_1(\nsys_2 junk\n"
    recs = [(hashlib.sha1(v).hexdigest().encode(), v, i) for i, v in enumerate(vals)]
    d = db.open_db(gpu, db_ref.serialize_db(7, recs))
    assert d.ended == "eof" and d.Len() == len({r[0] for r in recs})
    got_vals = [v for v, _ in (d.records()[bytes(k).hex().encode()] for k in d.keys.cpu().numpy())]
    broken, disabled, cand = progtext.load_corpus(gpu, table, d, enabled)
    eb, ed, ec = R.load_corpus(got_vals, names, enabled.tolist())
    assert (broken.tolist(), disabled.tolist(), cand.tolist()) == (eb, ed, ec)
    assert len(eb) >= 4 and len(ed) >= 1 and len(ec) >= 1
    # disabledHashes: the keys of the disabled records are hash.String of their values
    keys = d.keys.cpu().numpy()
    assert [bytes(keys[i]).hex() for i in ed] == [hashlib.sha1(got_vals[i]).hexdigest() for i in ed]
    # Connect: the ids of every corpus program -> CalculatePriorities -> BuildChoiceTable
    off, ids, status, _, _ = progtext.prog_calls(gpu, table, d.vals, enabled)
    corpus = [R.prog_calls(v, R.table_of(names))[2] for v in got_vals]
    assert ids.cpu().tolist() == [i for c in corpus for i in c]
    prios = prio.calculate_priorities(gpu, (off, ids), ncalls)
    exp = prio_ref.calculate_priorities(corpus, ncalls)
    assert_same(prios.cpu().numpy(), exp)
    ct = prio.ChoiceTable.build(gpu, prios, enabled, ncalls)
    assert np.array_equal(ct.run.cpu().numpy(), prio_ref.build_choice_table(exp, enabled.tolist(), ncalls))
    table.free()
