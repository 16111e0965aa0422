"""GPU: batches one sweep past the launch caps of syzsig_prog_calls_dev, the
pkg/db entry points, syzsig_hash_dev and the Sig sets (tests/launch_caps.py names
the caps and where they were read).  Past its cap a workgroup, a wave or a lane
serves a second element: the place where state kept in registers or LDS is not
reset, where the stride is computed in the wrong width, or where the sweep stops.

Each batch is cap + a few of the smallest elements that still take every
branch, laid out from a small pool so that the element served second never has
the outcome class of the one served first (asserted here, on the CPU side of
each test); the rare classes stand at cap - 1, cap, cap + 1 and at the end.  No
expected value comes from the device: the references run once per distinct
element (tests/launch_caps.py, held to the plain loops by
tests/test_launch_caps_cpu.py).  Outputs are pre-filled so that an unwritten or
overwritten entry shows, and the element after the last must stay untouched."""
import ctypes

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, db, hashing, progtext
from tests import db_ref as R
from tests import launch_caps as L
from tests import progtext_cases as C

pytestmark = pytest.mark.gpu

FILL = 0xCD
W = progtext.WINDOW
DES, CS = progtext.DESERIALIZE, progtext.CALLSET
LONG = _lib.SYZSIG_DEFLATE_LONG
GF, PW, PL, SG, RW = L.CAP_GRID_FOR, L.CAP_PC_WAVES, L.CAP_PC_LONG, L.CAP_SU_GATHER, L.CAP_REC_WRITE
DEL = L.DEL


def p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def dev(gpu, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a).to(gpu.dev) if a.size else torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=gpu.dev)


def full(gpu, n, value, dtype):
    return torch.full((n,), value, dtype=dtype, device=gpu.dev)


def room(nbytes):
    """the device memory a test is about to ask for, worked out from its own sizes: well under 1 GB, and there"""
    assert nbytes < 1 << 30, nbytes
    assert torch.cuda.mem_get_info()[0] > nbytes
    return nbytes


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1)) if got.size else np.zeros(0, np.int64)
    assert bad.size == 0, "%s: %d differ, the first at %s: %s, expected %s" % (
        what, bad.size, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


# ---- program text ----

NAMES = C.NAMES + [b"n" * W]
ENABLED = np.ones(len(NAMES), np.uint8)
ENABLED[C.READ] = 0
# OK with one call, OK with two, an unknown call, a disabled call, BAD_HEAD without a newline, empty, a comment alone
SHORT_POOL = [b"getpid()\n", b"open()\nclose()\n", b"nosuch()\n", b"read()\n", b"foo", b"", b"#c\n"]
SHORT_RARE = (2, 3, 4, 5, 6)
# a known call, an unknown call, a comment longer than the window, a head with no bracket (each of them with nothing
# decided in its first W bytes unless it is a comment), a short comment
LONG_POOL = [b"n" * W + b"()\n", b"u" * W + b"()\n", b"#" + b"x" * (W + 1) + b"\n", b"n" * (W + 2) + b"\n", b"#c\n"]


@pytest.fixture(scope="module")
def tab(gpu):
    t = progtext.CallTable(gpu, NAMES)
    yield t
    t.free()


def run_calls(gpu, tab, e, mode, off=None):
    """one call over the batch e, every output pre-filled; -> (rc, total, coff, ids, status, err_line, flag)"""
    n, cap = e["off"].size - 1, e["ids"].size
    room(2 * e["blob"].size + 128 * n + 32 * e["stats"][0] + 16 * cap)
    data, d_off, en = dev(gpu, e["blob"]), dev(gpu, e["off"] if off is None else off), dev(gpu, ENABLED)
    coff, ids = full(gpu, n + 2, -1, torch.int64), full(gpu, cap + 1, -1, torch.int32)
    status, flag = full(gpu, n + 1, FILL, torch.uint8), full(gpu, n + 1, FILL, torch.uint8)
    err = full(gpu, n + 1, -1, torch.int32)
    total = ctypes.c_uint64(12345)
    torch.cuda.synchronize()
    rc = gpu.L.syzsig_prog_calls_dev(gpu.eng.h, tab.h, p(data), data.numel(), p(d_off), n, mode, p(en), p(coff),
                                     ctypes.c_void_p(ids.data_ptr()), cap, p(status), p(err), p(flag), ctypes.byref(total))
    return (rc, total.value) + tuple(t.cpu().numpy() for t in (coff, ids, status, err, flag))


def check_calls(gpu, tab, e, mode):
    n, cap = e["off"].size - 1, e["ids"].size
    rc, total, coff, ids, status, err, flag = run_calls(gpu, tab, e, mode)
    assert rc == 0, gpu.L.syzsig_last_error()  # (SYZSIG_EIO would be "a listed head was left undecided")
    assert total == cap
    same(status[:n], e["status"], "status")
    same(err[:n], e["err_line"], "err_line")
    same(flag[:n], e["flag"], "flag")
    same(coff[: n + 1], e["call_off"], "call_off")
    same(ids[:cap], e["ids"], "ids")
    assert status[n] == FILL and err[n] == -1 and flag[n] == FILL and coff[n + 1] == -1 and ids[cap] == -1
    assert progtext.stats(gpu) == e["stats"]


def untouched(coff, ids, status, err, flag):
    return (coff == -1).all() and (ids == -1).all() and (status == FILL).all() and (err == -1).all() and (flag == FILL).all()


@pytest.mark.parametrize("mode", [DES, CS])
def test_prog_calls_a_wave_serves_a_second_program(gpu, tab, mode):
    """k_pc_reduce and k_pc_write, a wave per program on 65536 workgroups of four: 262144 + 5 programs; in CallSet
    mode k_su_gather too, a workgroup per program on 65536"""
    n = PW + 5
    kind = L.place(n, len(SHORT_POOL), (PW, SG), SHORT_RARE)
    assert n > PW > SG and L.crosses(kind, PW) and L.crosses(kind, SG)
    e = L.prog_calls_expect(SHORT_POOL, kind, NAMES, mode, ENABLED.tolist(), W)
    assert len(set(e["status"].tolist())) >= 3 and e["flag"].any() and e["stats"][3] == 0
    check_calls(gpu, tab, e, mode)


@pytest.mark.parametrize("mode", [DES, CS])
def test_prog_calls_a_lane_serves_a_second_program(gpu, tab, mode):
    """k_pc_prep and k_pc_seglens, a program per thread on 2048 workgroups of 256: 524288 + 3 programs; then one
    decreasing offset in the second sweep, which a k_pc_prep that stopped at the cap would not see"""
    n = GF + 3
    kind = L.place(n, len(SHORT_POOL), (GF, PW, SG), SHORT_RARE)
    assert n > GF and all(L.crosses(kind, c) for c in (GF, PW, SG))
    e = L.prog_calls_expect(SHORT_POOL, kind, NAMES, mode, ENABLED.tolist(), W)
    check_calls(gpu, tab, e, mode)
    off = e["off"].copy()
    assert off[GF] >= 1 and GF + 1 < n
    off[GF + 1] = off[GF] - 1  # program 524288 ends before it starts
    rc, total, *outs = run_calls(gpu, tab, e, mode, off=off)
    assert rc == _lib.SYZSIG_EINVAL and total == 0 and untouched(*outs)


@pytest.mark.parametrize("mode", [DES, CS])
def test_prog_calls_a_lane_serves_a_second_listed_head(gpu, tab, mode):
    """k_pc_long, a listed head per lane on 1024 workgroups of 64: 65536 + a few lines whose head is not decided
    within the window, one line per program, a comment after every three (comments are never listed)"""
    n = 109240
    kind = np.arange(n) % len(LONG_POOL)
    line_listed = np.array([L.listed(p_.rstrip(b"\n"), W) for p_ in LONG_POOL])
    assert line_listed.tolist() == [True, True, False, True, False]
    heads = kind[line_listed[kind]]  # the listed heads in line order (the list's own order is the atomics')
    assert PL < heads.size <= PL + 16 and L.crosses(heads, PL)
    assert n > SG and L.crosses(kind, SG)
    e = L.prog_calls_expect(LONG_POOL, kind, NAMES, mode, ENABLED.tolist(), W)
    assert e["stats"][3] == heads.size and e["stats"][0] == n and e["stats"][2] == 0
    check_calls(gpu, tab, e, mode)
    assert progtext.stats(gpu)[3] == heads.size


# ---- deflate and inflate ----

VALS = [b"", b"q", b"abc" * 8, bytes(np.random.default_rng(7).integers(0, 256, 80, dtype=np.uint8))]
LONG_VAL = (b"r0 = openat$dir(0xffffffffffffff9c, &(0x7f0000000000)='./file0\\x00', 0x0, 0x0)\n" * 60)[: LONG + 1]


@pytest.fixture(scope="module")
def deflate_case():
    """524288 + 3 values: empty, one byte, a short repeat that goes out fixed, short noise that goes out stored"""
    n = GF + 3
    kind = L.place(n, len(VALS), (GF,), (0, 1))
    assert n > GF and L.crosses(kind, GF)
    streams = L.checked_streams(VALS, db.deflate_host)
    assert [L.stream_form(s) for s in streams[1:]] == ["fixed", "fixed", "stored"] and streams[0] == b""
    return kind, L.deflate_expect(VALS, kind, db.deflate_host, LONG)


def run_deflate(gpu, e, src_off=None, src_len=None):
    n, cap = e["src_len"].size, e["out"].size
    room(e["src"].size + 2 * cap + 64 * n)
    src = dev(gpu, e["src"])
    d_off, d_len = dev(gpu, e["src_off"] if src_off is None else src_off), dev(gpu, e["src_len"] if src_len is None else src_len)
    out, off = full(gpu, cap + 32, FILL, torch.uint8), full(gpu, n + 2, -1, torch.int64)
    total = ctypes.c_uint64(12345)
    rc = gpu.L.syzsig_deflate_dev(gpu.eng.h, p(src), src.numel(), p(d_off), p(d_len), n, p(out), cap, p(off),
                                  ctypes.byref(total))
    return rc, total.value, out.cpu().numpy(), off.cpu().numpy()


def check_deflate(gpu, e):
    n, cap = e["src_len"].size, e["out"].size
    rc, total, out, off = run_deflate(gpu, e)
    assert rc == 0, gpu.L.syzsig_last_error()
    assert total == cap
    same(off[: n + 1], e["out_off"], "stream offsets")
    same(out[:cap], e["out"], "stream bytes")
    assert off[n + 1] == -1 and (out[cap:] == FILL).all()
    assert db.deflate_stats(gpu) == e["stats"]


def test_deflate_a_lane_checks_a_second_value(gpu, deflate_case):
    """k_def_prep on 2048 workgroups of 256; then a range past nbytes in the second sweep, then a value of
    SYZSIG_DEFLATE_LONG + 1 bytes there, which the sweep must list"""
    kind, e = deflate_case
    n = kind.size
    assert e["stats"][1] == 0 and e["stats"][2] > n // 5 and e["stats"][3] > n // 3
    check_deflate(gpu, e)
    bad_off, bad_len = e["src_off"].copy(), e["src_len"].copy()
    bad_off[GF + 1], bad_len[GF + 1] = e["src"].size - 4, 5
    rc, total, out, off = run_deflate(gpu, e, bad_off, bad_len)
    assert rc == _lib.SYZSIG_EINVAL and total == 0 and (out == FILL).all() and (off == -1).all()
    kind2 = kind.copy()
    kind2[GF + 2] = len(VALS)
    assert L.crosses(kind2, GF) and R.inflate_class(db.deflate_host(LONG_VAL)) == (R.OK, LONG_VAL)
    e2 = L.deflate_expect(VALS + [LONG_VAL], kind2, db.deflate_host, LONG)
    assert e2["stats"][1] == 1
    check_deflate(gpu, e2)


def test_inflate_a_lane_checks_a_second_stream(gpu, deflate_case):
    """k_inf_prep on 2048 workgroups of 256: the streams of the values above back to the values"""
    kind, e = deflate_case
    n, cap = kind.size, e["src"].size
    room(2 * e["out"].size + 2 * cap + 64 * n)
    src = dev(gpu, e["out"])
    lens = np.diff(e["out_off"]).astype(np.int32)
    for bad in (False, True):
        s_off = e["out_off"][:-1].copy()
        if bad:
            s_off[GF + 1], lens[GF + 1] = e["out"].size - 1, 2
        out, off = full(gpu, cap + 32, FILL, torch.uint8), full(gpu, n + 2, -1, torch.int64)
        status = full(gpu, n + 1, FILL, torch.uint8)
        total = ctypes.c_uint64(12345)
        d_off, d_len = dev(gpu, s_off), dev(gpu, lens)
        rc = gpu.L.syzsig_inflate_dev(gpu.eng.h, p(src), src.numel(), p(d_off), p(d_len), n, p(out), cap, p(off), p(status),
                                      ctypes.byref(total))
        out, off, status = out.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy()
        if bad:
            assert rc == _lib.SYZSIG_EINVAL and total.value == 0
            assert (out == FILL).all() and (off == -1).all() and (status == FILL).all()
            continue
        assert rc == 0, gpu.L.syzsig_last_error()
        assert total.value == cap and not status[:n].any() and status[n] == FILL
        same(off[: n + 1], np.concatenate([e["src_off"], [cap]]), "value offsets")
        same(out[:cap], e["src"], "value bytes")
        assert off[n + 1] == -1 and (out[cap:] == FILL).all()
        st = db.inflate_stats(gpu)
        assert st[0] == int((lens > 0).sum()) and st[1] == 0


# ---- record frames ----

def run_records(gpu, sigs, seqs, sdata, soff, cap):
    n = seqs.size
    room(20 * n + 48 * n + sdata.size + cap + 64)
    d_sig, d_seq, d_sd, d_so = dev(gpu, sigs), dev(gpu, seqs), dev(gpu, sdata), dev(gpu, soff)
    out, off = full(gpu, cap + 32, FILL, torch.uint8), full(gpu, n + 2, -1, torch.int64)
    total = ctypes.c_uint64(12345)
    rc = gpu.L.syzsig_db_records_dev(gpu.eng.h, p(d_sig), p(d_seq), n, p(d_sd), d_sd.numel(), p(d_so), p(out), cap, p(off),
                                     ctypes.byref(total))
    return rc, total.value, out.cpu().numpy(), off.cpu().numpy()


def records_case(n, kind, vals, seed):
    rng = np.random.default_rng(seed)
    sigs = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    seqs = rng.integers(0, 1 << 62, n, dtype=np.uint64) * np.uint64(2) + (np.arange(n) & 1).astype(np.uint64)
    seqs[kind == len(vals)] = np.uint64(DEL)
    return sigs, seqs, L.stream_pair(vals, kind, db.deflate_host), L.records_expect(vals, kind, sigs, seqs, db.deflate_host)


def test_db_records_a_wave_writes_a_second_record(gpu):
    """k_rec_write, a wave per record on 65536 workgroups: 65536 + 3 records -- an empty value (60 bytes), a short
    stream, a stream of more than 64 bytes (the copy loop runs twice), a delete (56 bytes)"""
    vals = [VALS[0], VALS[2], VALS[3]]
    n = RW + 3
    kind = L.place(n, 4, (RW,), (3, 0))
    assert n > RW and L.crosses(kind, RW)
    sigs, seqs, (sdata, soff), (data, off) = records_case(n, kind, vals, 11)
    lens = np.diff(off)
    assert sorted(set(lens.tolist())) == [56, 60, 60 + len(db.deflate_host(vals[1])), 60 + len(db.deflate_host(vals[2]))]
    assert len(db.deflate_host(vals[2])) > 64 > len(db.deflate_host(vals[1]))
    rc, total, out, got_off = run_records(gpu, sigs, seqs, sdata, soff, data.size)
    assert rc == 0, gpu.L.syzsig_last_error()
    assert total == data.size
    same(got_off[: n + 1], off, "record offsets")
    same(out[: data.size], data, "record bytes")
    assert got_off[n + 1] == -1 and (out[data.size:] == FILL).all()


def test_db_records_a_lane_measures_a_second_record(gpu):
    """k_rec_len on 2048 workgroups of 256: 524288 + 3 deletes and empty values; then a delete with a stream in the
    second sweep"""
    n = GF + 3
    i = np.arange(n)
    kind = (i + i // GF + 1) % 2  # 0: an empty value, 1: a delete
    assert n > GF and L.crosses(kind, GF)
    sigs, seqs, (sdata, soff), (data, off) = records_case(n, kind, [b""], 12)
    assert sdata.size == 0 and not soff.any() and set(np.diff(off).tolist()) == {56, 60}
    rc, total, out, got_off = run_records(gpu, sigs, seqs, sdata, soff, data.size)
    assert rc == 0, gpu.L.syzsig_last_error()
    assert total == data.size
    same(got_off[: n + 1], off, "record offsets")
    same(out[: data.size], data, "record bytes")
    assert got_off[n + 1] == -1 and (out[data.size:] == FILL).all()
    at = GF + 1
    assert kind[at] == 1
    soff = soff.copy()
    soff[at + 1:] = 2  # record 524289, a delete, has the stream's two bytes
    rc, total, out, got_off = run_records(gpu, sigs, seqs, np.frombuffer(b"\x03\x00", np.uint8), soff, data.size)
    assert rc == _lib.SYZSIG_EINVAL and b"deleting record with value" in gpu.L.syzsig_last_error()
    assert total == 0 and (out == FILL).all() and (got_off == -1).all()


# ---- hashes ----

PAD_LENS = (0, 1, 55, 56, 64, 65)  # the SHA-1 padding classes


@pytest.fixture(scope="module")
def hash_case():
    """524288 + 3 messages; those long enough carry their index in their first four bytes, so that a kernel that
    hashed message i - cap again shows"""
    n = GF + 3
    rng = np.random.default_rng(13)
    base = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in PAD_LENS]
    kind = L.place(n, len(base), (GF,), (0, 1))
    assert n > GF and L.crosses(kind, GF)
    counter = np.array(PAD_LENS)[kind] >= 4
    data, off, dig = L.hash_expect(base, kind, counter)
    assert np.unique(dig[counter], axis=0).shape[0] == int(counter.sum()) > n // 2
    return kind, counter, data, off, dig


def test_hash_a_lane_checks_a_second_message(gpu, hash_case):
    """k_hash_prep on 2048 workgroups of 256"""
    kind, counter, data, off, dig = hash_case
    n = kind.size
    room(data.size + 8 * n + 20 * n + 64)
    out = torch.full((n + 1, 20), FILL, dtype=torch.uint8, device=gpu.dev)
    got = hashing.hash_batch(gpu, dev(gpu, data), dev(gpu, off), out=out)
    assert got.data_ptr() == out.data_ptr()
    o = out.cpu().numpy()
    same(o[:n], dig, "Sigs")
    assert (o[n] == FILL).all()
    st = hashing.hash_stats(gpu)
    assert sum(st[:3]) == n and st[2] == 0 and st[3] == int(((np.diff(off) + 72) // 64).sum())
    bad = off.copy()
    bad[GF + 1] = bad[GF] - 1
    out.fill_(FILL)
    with pytest.raises(_lib.SyzsigError) as e:
        hashing.hash_batch(gpu, dev(gpu, data), dev(gpu, bad), out=out)
    assert e.value.code == _lib.SYZSIG_EINVAL and (out == FILL).all()


# ---- the Sig sets, db_live and db_apply ----

@pytest.fixture(scope="module")
def keyed_rows(hash_case):
    """524288 + 3 Sigs from the hashes above: a row whose message carries its index has its own Sig; the others, about
    a third, have the Sig of a row half a batch away; and row i >= cap has the Sig of row i - cap"""
    kind, counter, data, off, dig = hash_case
    n = kind.size
    i = np.arange(n)
    far = (i + n // 2) % n
    for _ in range(8):
        far = np.where(counter[far], far, (far + 1) % n)
    assert counter[far].all()
    src = np.where(counter, i, far)
    src[GF:] = src[: n - GF]
    sigs = dig[src]
    dup = ~L.first_rows(sigs)
    assert n // 4 < dup.sum() < n // 2 and dup[GF:].all() and (sigs[GF:] == sigs[: n - GF]).all()
    return sigs


def run_flags(gpu, fn, sigs, *args):
    """a Sig-set entry point that writes a flag per row, into a pre-filled buffer"""
    n = sigs.shape[0]
    d_sig, out = dev(gpu, sigs), full(gpu, n + 1, FILL, torch.uint8)
    rc = fn(gpu.eng.h, *args, p(d_sig), n, p(out))
    assert rc == 0, gpu.L.syzsig_last_error()
    out = out.cpu().numpy()
    assert out[n] == FILL
    return out[:n]


def test_sigsets_a_lane_serves_a_second_row(gpu, keyed_rows):
    """every k_sg_* row kernel behind SigSet.add and contains, on 2048 workgroups of 256"""
    sigs = keyed_rows
    n = sigs.shape[0]
    assert n > GF
    room(20 * n + 2 * 24 * n + 6 * 4 * n + 24 * n + 4096)
    small = sigs[: n // 4]
    s = hashing.SigSet(gpu)
    is_new, size = L.sigset_add(np.zeros((0, 20), np.uint8), small)
    same(run_flags(gpu, gpu.L.syzsig_sigset_add_dev, small, ctypes.byref(s._h)), is_new, "is_new of the first add")
    assert s.Len() == size
    held = small[is_new]
    want = L.member(sigs, held)
    assert want[GF:].any() and 0 < want.sum() < n
    same(run_flags(gpu, gpu.L.syzsig_sigset_contains_dev, sigs, s._h), want, "contains")
    is_new, size = L.sigset_add(held, sigs)
    assert not is_new[GF:].any() and 0 < is_new.sum() < n - held.shape[0]
    same(run_flags(gpu, gpu.L.syzsig_sigset_add_dev, sigs, ctypes.byref(s._h)), is_new, "is_new of the second add")
    assert s.Len() == size == np.unique(sigs, axis=0).shape[0]
    same(run_flags(gpu, gpu.L.syzsig_sigset_contains_dev, sigs, s._h), np.ones(n, bool), "contains everything")


def test_new_input_keys_past_the_cap(gpu, hash_case):
    """hash_batch and numberSigs over 524288 + 3 programs, a third of which are one of two programs"""
    kind, counter, data, off, dig = hash_case
    n = kind.size
    room(data.size + 8 * n + 20 * n + 2 * 24 * n + 9 * 4 * n + 4096)
    corpus_sigs = dig[np.arange(n) % 5 == 0]
    corpus_sigs = corpus_sigs[L.first_rows(corpus_sigs)]
    corpus = hashing.SigSet(gpu)
    corpus.add(corpus_sigs)
    key, first, known = L.number_sigs(dig, corpus_sigs)
    assert known.any() and not known.all() and first.size < n - n // 4
    raw = data.tobytes()
    got = hashing.new_input_keys(gpu, [raw[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist())], corpus)
    same(got["sigs"].cpu().numpy(), dig, "Sigs")
    assert got["nkeys"] == first.size
    same(got["input_key"].astype(np.int64), key, "input_key")
    same(got["first"], first, "first")
    same(got["present"], np.flatnonzero(known), "present")


def test_db_live_a_lane_serves_a_second_record(gpu, keyed_rows):
    """k_sg_last on 2048 workgroups of 256, the last record left out of the replay"""
    sigs = keyed_rows
    n = sigs.shape[0]
    room(20 * n + 8 * n + 2 * 24 * n + 5 * 4 * n + 4096)
    seqs = (np.arange(n) % 3).astype(np.uint64)
    seqs[np.arange(n) % 4 == 1] = np.uint64(DEL)
    seqs[n - 1] = 1
    want = L.db_live(sigs, seqs, n - 1)
    assert n - 1 > GF and want[GF:].any() and not want[n - 1] and 0 < want.sum() < n // 2 + n // 4
    live, nlive, unc = db.db_live(gpu, dev(gpu, sigs), dev(gpu, seqs), n - 1)
    same(live.cpu().numpy(), want, "live")
    assert (nlive, unc) == (int(want.sum()), n - 1)


def test_db_apply_a_lane_serves_a_second_row(gpu, keyed_rows):
    """k_ap_check, k_ap_pack, k_ap_written and k_ap_keep on 2048 workgroups of 256: a third of the rows are the live
    records, the rest the ops, a quarter of them deletes"""
    sigs = keyed_rows
    n = sigs.shape[0]
    nl = n // 3
    i = np.arange(n)
    own = L.first_rows(sigs)
    # a row that repeats a Sig repeats its seq and its value too two times out of three: a Save that changes nothing
    first_of = np.zeros(n, np.int64)
    order, run = L.sig_runs(sigs)
    head = order[np.concatenate([[True], run[1:] != run[:-1]])]
    first_of[order] = head[run]
    seqs = (first_of % 3).astype(np.uint64)
    vk = (first_of % 4).astype(np.int64)
    change = ~own & (i % 3 == 0)
    seqs[change] = (seqs[change] + np.uint64(1)) % np.uint64(3)
    vk[~own & (i % 3 == 1)] = 3 - vk[~own & (i % 3 == 1)]
    seqs[GF:] = (seqs[: n - GF] + np.uint64(1)) % np.uint64(3)  # across the cap: the same Sig, another seq
    dele = (i >= nl) & (i % 4 == 1)
    seqs[dele], vk[dele] = np.uint64(DEL), 0
    assert n > GF and np.unique(sigs[:nl], axis=0).shape[0] == nl
    assert ((seqs[GF:] != seqs[: n - GF]) | (vk[GF:] != vk[: n - GF])).all()
    pool = [b"", b"a", b"prog one\n", b"prog two\n"]
    written, keep_live, keep_op = L.db_apply(sigs[:nl], seqs[:nl], vk[:nl], sigs[nl:], seqs[nl:], vk[nl:])
    saves = ~dele[nl:]
    assert 0 < (saves & ~written).sum() and 0 < (~saves & ~written).sum() and 0 < (~saves & written).sum()
    assert 0 < keep_live.sum() < nl and 0 < keep_op.sum() < written.sum() and written[GF - nl:].any()
    ldata, loff = L.ragged_take(pool, vk[:nl])
    odata, ooff = L.ragged_take(pool, vk[nl:])
    room(20 * n + 8 * n + 8 * n + ldata.size + odata.size + 2 * 24 * n + 6 * 4 * n + 3 * n + 4096)
    w, kl, ko, counts = db.db_apply(gpu, dev(gpu, sigs[:nl]), dev(gpu, seqs[:nl]), (dev(gpu, ldata), dev(gpu, loff)),
                                    dev(gpu, sigs[nl:]), dev(gpu, seqs[nl:]), (dev(gpu, odata), dev(gpu, ooff)))
    same(w.cpu().numpy(), written, "written")
    same(kl.cpu().numpy(), keep_live, "keep_live")
    same(ko.cpu().numpy(), keep_op, "keep_op")
    assert counts == (int(written.sum()), int(keep_live.sum()), int(keep_op.sum()))
