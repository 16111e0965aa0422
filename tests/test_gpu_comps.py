"""GPU: the executor's comps output (executor.h:576-593, syzsig_exec_comps_dev)
and the CompMap parse (ipc.go:420-465, syzsig_comp_map_dev), bit for bit
against tests/comps_ref.py: the hand cases, the one-workgroup LDS sort up to
SYZSIG_COMPS_TILE keys, tiles + merge passes past it."""
import ctypes

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, synth
from syzkaller_amd.hints import CompMap
from tests import comps_ref as R

pytestmark = pytest.mark.gpu

T = _lib.SYZSIG_COMPS_TILE
OUT = 0x7f1200000000
KM0, KM1 = 0xffff880000000000, 0xffff890000000000
SENT = 0x5e5e5e5e


def dev_i64(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(gpu.dev)


def dev_i32(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(gpu.dev)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def run_exec_comps(gpu, comps, call_start, call_len):
    """-> (out, out_words, comps_cnt) as numpy, out prefilled with SENT"""
    comps = np.asarray(comps, np.uint64).reshape(-1, 4)
    out = torch.full((5 * comps.shape[0],), SENT, dtype=torch.int32, device=gpu.dev)
    o, nw, cnt = gpu.exec_comps(dev_i64(gpu, comps), dev_i64(gpu, call_start), dev_i32(gpu, call_len), OUT, out=out)
    return u32(o), u32(nw), u32(cnt)


def check_exec_comps(gpu, comps, call_start, call_len):
    got = run_exec_comps(gpu, comps, call_start, call_len)
    exp = R.exec_comps(comps, call_start, call_len, OUT, fill=SENT)
    for g, e in zip(got[::-1], exp[::-1]):
        np.testing.assert_array_equal(g, e)
    return got


HAND = [  # (records, expected words, expected comps_size): tests/test_comps_ref_cpu.py's cases
    ([(0x100000002, 5, 6, 0), (2, 7, 8, 0)], [2, 7, 8, 2, 5, 6], 2),
    ([(4, 10, 11, 1), (4, 10, 11, 2), (4, 10, 11, 1)], [4, 10, 11], 1),
    ([(0, 0x1fe, 1, 0), (0, 0xfe, 1, 0)], [0, 0xfffffffe, 1, 0, 0xfffffffe, 1], 2),
    ([(2, 0x8000, 0x7fff, 0), (4, 0x180000000, 1, 0), (1, 0x17f, 0x80, 0)],
     [1, 0x7f, 0xffffff80, 2, 0xffff8000, 0x7fff, 4, 0x80000000, 1], 3),
    ([(6, 0x1122334455667788, 0x99aabbccddeeff00, 0)], [6, 0x55667788, 0x11223344, 0xddeeff00, 0x99aabbcc], 1),
    # ignore(): the zero branch
    ([(0, 0, 0, 0), (1, 0, 5, 0), (7, 0, 5, 0), (0, 0, 5, 0), (1, 5, 0, 0)], [0, 0, 5, 1, 5, 0], 2),
    # ... the output region, both ends inclusive, SIZE8 only
    ([(6, OUT, 1, 0), (6, OUT + (16 << 20), 1, 0), (6, 1, OUT, 0), (6, 1, OUT + (16 << 20), 0),
      (6, OUT - 1, 1, 0), (6, OUT + (16 << 20) + 1, 2, 0), (4, OUT, 1, 0)],
     [4, OUT & 0xffffffff, 1,
      6, (OUT - 1) & 0xffffffff, (OUT - 1) >> 32, 1, 0,
      6, (OUT + (16 << 20) + 1) & 0xffffffff, (OUT + (16 << 20) + 1) >> 32, 2, 0], 3),
    # ... kernel pointers
    ([(6, KM0, KM1, 0), (6, KM0, 0, 0), (6, 0, KM1, 0), (6, KM0 - 1, KM1, 0), (6, KM1 + 1, 0, 0), (2, KM0, KM1, 0)],
     [2, 0, 0,
      6, 0xffffffff, 0xffff87ff, 0, 0xffff8900,
      6, 1, 0xffff8900, 0, 0], 3),
    ([], [], 0),
]


def test_exec_comps_hand_cases(gpu):
    lens = [len(r) for r, _, _ in HAND]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    comps = np.array([x for r, _, _ in HAND for x in r], np.uint64)
    out, nw, cnt = check_exec_comps(gpu, comps, starts, lens)
    for i, (_, words, n) in enumerate(HAND):
        s = 5 * int(starts[i])
        assert out[s:s + int(nw[i])].tolist() == words, i
        assert (int(nw[i]), int(cnt[i])) == (len(words), n), i


@pytest.fixture(scope="module")
def ragged():
    """calls of 0 .. 5, T - 1, T, T + 1, 2 T + 3, 3 T (an odd tile count: the
    last run of a merge pass has no partner), 4 T (a full last tile) and 65535
    records; the last drawn from a larger pool, so that most of its triples are
    distinct.  One call: the shorter long calls are copied through the later
    merge passes of the longest."""
    lens = [0, 1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 3, 3 * T, 4 * T, 65535]
    a, _ = synth.comparisons(11, lens[:-1], OUT)
    b, _ = synth.comparisons(12, lens[-1:], OUT, pool=700)
    comps = np.concatenate([a, b])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    ref = R.exec_comps(comps, starts, lens, OUT, fill=SENT)
    return comps, starts, np.array(lens, np.uint32), ref


def test_exec_comps_segment_lengths_and_sentinels(gpu, ragged):
    comps, starts, lens, ref = ragged
    assert set(np.unique(comps[:, 0]).tolist()) == set(range(8))
    got = run_exec_comps(gpu, comps, starts, lens)
    for g, e in zip(got[::-1], ref[::-1]):  # the whole buffer: the words outside the written ranges keep SENT
        np.testing.assert_array_equal(g, e)
    assert ref[2][-1] > T  # the long call's survivors pass the tile


def test_exec_comps_too_many_comparisons_rejected_nothing_written(gpu):
    comps = torch.zeros((65536 + 3, 4), dtype=torch.int64, device=gpu.dev)
    comps[:, 1] = torch.arange(1, 65536 + 4, device=gpu.dev)
    out = torch.full((5 * comps.shape[0],), SENT, dtype=torch.int32, device=gpu.dev)
    nw = torch.full((2,), SENT, dtype=torch.int32, device=gpu.dev)
    cnt = torch.full((2,), SENT, dtype=torch.int32, device=gpu.dev)
    with pytest.raises(_lib.SyzsigError) as e:
        gpu.exec_comps(comps, dev_i64(gpu, [0, 3]), dev_i32(gpu, [3, 65536]), OUT, out=out, out_words=nw,
                       comps_cnt=cnt)
    assert e.value.code == _lib.SYZSIG_EINVAL
    for t in (out, nw, cnt):
        assert bool((t == SENT).all())
    with pytest.raises(_lib.SyzsigError) as e:  # a range past the buffer
        gpu.exec_comps(comps, dev_i64(gpu, [65530]), dev_i32(gpu, [10]), OUT, out=out)
    assert e.value.code == _lib.SYZSIG_EINVAL


def test_exec_comps_one_record_repeated_past_the_tile(gpu):
    n = T + 5
    comps = np.tile(np.array([[4, 0x11223344, 0x80000001, 0]], np.uint64), (n, 1))
    comps[:, 3] = np.arange(n)
    out, nw, cnt = check_exec_comps(gpu, comps, [0], [n])
    assert out[:3].tolist() == [4, 0x11223344, 0x80000001] and (int(nw[0]), int(cnt[0])) == (3, 1)


def check_comp_map(got, exp):
    st, off, pairs = got
    est, eoff, epairs, _ = exp
    np.testing.assert_array_equal(st.cpu().numpy(), est)
    np.testing.assert_array_equal(u64(off), eoff)
    np.testing.assert_array_equal(u64(pairs).reshape(-1, 2), epairs)


def test_comp_map_on_exec_comps_output(gpu, ragged):
    comps, starts, lens, _ = ragged
    words, nw, cnt = gpu.exec_comps(dev_i64(gpu, comps), dev_i64(gpu, starts), dev_i32(gpu, lens), OUT)
    m = CompMap.from_exec_output(gpu, words, dev_i64(gpu, starts), nw, cnt)
    hw, hnw, hcnt = u32(words), u32(nw), u32(cnt)
    exp = R.comp_map(hw, 5 * starts, hcnt, 5 * starts + hnw)
    check_comp_map((m.status, m.off, m.pairs), exp)
    assert int(exp[1][-1] - exp[1][-2]) > T  # the long call's pairs exceed one tile
    key = int(exp[2][-1][0])
    assert m.lookup(len(lens) - 1, key) == sorted(exp[3][-1][key])
    assert m.lookup(0, key) == []


def test_comp_map_hand_cases_and_statuses(gpu):
    calls = [  # (words, comps_size, expected status, expected pairs)
        ([0, 0xfffffffe, 1], 1, 0, [(1, 0xfffffffe), (0xfffffffe, 1)]),  # zero-extended, not 0xff..fe
        ([6, 0x55667788, 0x11223344, 2, 0, 0, 7, 7, 1, 3, 9], 3, 0,
         [(2, 0x1122334455667788), (9, 3), (0x1122334455667788, 2)]),
        ([0, 1, 2, 0, 1, 2, 0, 2, 1], 3, 0, [(1, 2), (2, 1)]),  # the same pair from three records
        ([0, 1, 2], 2, _lib.SYZSIG_INGEST_ECOMPS, []),           # its region ends after record 0
        ([6, 1, 0, 2], 1, _lib.SYZSIG_INGEST_ECOMPS, []),
        ([0, 1, 2, 8, 1, 2], 2, _lib.SYZSIG_INGEST_ECOMPTYPE, []),
        ([], 0, 0, []),
    ]
    words = np.array([w for c in calls for w in c[0]], np.uint32)
    lens = [len(c[0]) for c in calls]
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    end = start + np.array(lens, np.uint64)
    cnt = [c[1] for c in calls]
    st, off, pairs = gpu.comp_map(dev_i32(gpu, words), dev_i64(gpu, start), dev_i32(gpu, cnt), dev_i64(gpu, end))
    check_comp_map((st, off, pairs), R.comp_map(words, start, cnt, end))
    assert st.cpu().tolist() == [c[2] for c in calls]
    o, p = off.cpu().tolist(), u64(pairs).reshape(-1, 2)
    for i, c in enumerate(calls):
        assert [tuple(x) for x in p[o[i]:o[i + 1]].tolist()] == c[3], i
    # without region ends a short record reads on into the next call's words
    # (as one region would): only the buffer's end stops it
    st2, _, _ = gpu.comp_map(dev_i32(gpu, words[:3]), dev_i64(gpu, [0]), dev_i32(gpu, [2]))
    assert st2.cpu().tolist() == [_lib.SYZSIG_INGEST_ECOMPS]


def test_comp_map_from_regions(gpu):
    """regions = headers + signal + cover + the comps words, through the ingest"""
    rng = np.random.default_rng(5)
    cpp, nprog = 3, 4
    lens = rng.integers(0, 300, nprog * cpp).astype(np.uint32)
    lens[4] = 0
    comps, starts = synth.comparisons(21, lens, OUT)
    words, nw, cnt = R.exec_comps(comps, starts, lens, OUT)
    ncalls = nprog * cpp
    per_call = [(words[5 * int(starts[c]):5 * int(starts[c]) + int(nw[c])], int(cnt[c])) for c in range(ncalls)]
    sigs = [rng.integers(0, 1 << 32, int(rng.integers(0, 9)), dtype=np.uint64).astype(np.uint32) for _ in range(ncalls)]
    covers = [rng.integers(0, 1 << 32, int(rng.integers(0, 9)), dtype=np.uint64).astype(np.uint32)
              for _ in range(ncalls)]
    prog_call = synth.prog_call_index(nprog, cpp)
    errno = rng.integers(0, 3, ncalls)
    out, prog_off = synth.frame_exec_output_comps(sigs, covers, per_call, prog_call, errno)
    dout = dev_i32(gpu, out)
    r = gpu.ingest_exec_output(dout, dev_i64(gpu, prog_off), dev_i32(gpu, prog_call),
                               torch.zeros(ncalls, dtype=torch.uint8, device=gpu.dev), want_cover=True)
    assert r["n_failed"] == 0
    m = CompMap.from_regions(gpu, dout, r)
    exp = [R.parse_comps(w, 0, n) for w, n in per_call]
    assert m.status.cpu().tolist() == [0] * ncalls
    off, pairs = m.off.cpu().tolist(), u64(m.pairs).reshape(-1, 2)
    for c in range(ncalls):
        np.testing.assert_array_equal(pairs[off[c]:off[c + 1]], R.map_pairs(exp[c][1]))
    assert off[-1] > 0


def test_comp_map_erange_reports_needed_total_and_writes_nothing(gpu):
    words = np.array([0, 1, 2, 0, 3, 4, 1, 5, 6], np.uint32)  # 2 + 2 + 1 pairs
    dw, ds, dc = dev_i32(gpu, words), dev_i64(gpu, [0]), dev_i32(gpu, [3])
    st = torch.full((1,), SENT, dtype=torch.int32, device=gpu.dev)
    off = torch.full((2,), SENT, dtype=torch.int64, device=gpu.dev)
    pairs = torch.full((4, 2), SENT, dtype=torch.int64, device=gpu.dev)
    n = ctypes.c_uint64()

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    rc = gpu.L.syzsig_comp_map_dev(gpu.eng.h, p(dw), 9, p(ds), p(dc), None, 1, p(st), p(off), p(pairs), 4,
                                   ctypes.byref(n))
    assert rc == _lib.SYZSIG_ERANGE and n.value == 5
    for t in (st, off, pairs):
        assert bool((t == SENT).all())
    with pytest.raises(_lib.SyzsigError) as e:
        gpu.comp_map(dw, ds, dc, pairs=pairs)
    assert e.value.code == _lib.SYZSIG_ERANGE and e.value.needed == 5
    _, off2, pairs2 = gpu.comp_map(dw, ds, dc)
    assert u64(pairs2).reshape(-1, 2).tolist() == [[1, 2], [2, 1], [3, 4], [4, 3], [6, 5]]
    with pytest.raises(_lib.SyzsigError) as e:  # a range outside the buffer
        gpu.comp_map(dw, dev_i64(gpu, [10]), dc)
    assert e.value.code == _lib.SYZSIG_EINVAL
