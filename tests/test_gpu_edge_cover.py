"""GPU: syzsig_edge_cover_dev -- the executor's cover output per call
(executor/executor.h:514-527: std::sort + std::unique over the PCs with
flag_dedup_cover, truncation to u32) -- bit-equal to the restatement
tests/cover_ref.py, on every path of the segmented sort-unique: the LDS sort
up to SYZSIG_COVER_TILE keys, tiles + merge passes past it."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from syzkaller_amd import _lib, synth
from tests import cover_ref as CR

pytestmark = pytest.mark.gpu

T = _lib.SYZSIG_COVER_TILE
HI = np.uint64(0xffffffff00000000)
LO, END = 0x80000000, 0xff000000  # cover_check's range, low words (executor_linux.cc:196-204)
FILL = 0x12345678                 # no PC's low word


def _t(gpu, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)


def _contents(kind, n, rng):
    if kind == "equal":
        low = np.full(n, 0x81000010, np.uint64)
    elif kind == "asc":
        low = LO + 3 * np.arange(n, dtype=np.uint64)
    elif kind == "desc":
        low = END - 1 - 5 * np.arange(n, dtype=np.uint64)
    elif kind == "dups":  # about 70 % duplicates
        low = 0x81000000 + 5 * rng.integers(0, max(1, int(0.3 * n)), n).astype(np.uint64)
    else:  # "span": both ends of the range and everything between
        low = rng.integers(LO, END, n).astype(np.uint64)
        low[: min(n, 2)] = [LO, END - 1][: min(n, 2)]
    return HI | low.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _lengths_batch():
    """Every length class x every content kind in one batch: odd call starts,
    gaps between calls, programs of 5 calls."""
    rng = np.random.default_rng(11)
    lens, starts, chunks, pos = [], [], [], 0
    for n in [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 262143]:
        for kind in ["equal", "asc", "desc", "dups", "span"]:
            gap = int(rng.integers(1, 40))
            gap += (pos + gap + 1) % 2  # an odd start
            chunks.append(HI | np.uint64(0x81000000) + rng.integers(0, 9, gap).astype(np.uint64))
            pos += gap
            starts.append(pos)
            lens.append(n)
            chunks.append(_contents(kind, n, rng))
            pos += n
    pcs = np.concatenate(chunks + [np.full(3, HI | np.uint64(0x81000000), np.uint64)])
    starts, lens = np.array(starts, np.uint64), np.array(lens, np.uint32)
    assert (starts % 2 == 1).all()
    prog_call = np.arange(0, lens.size + 1, 5, dtype=np.uint32)
    completed = np.full(prog_call.size - 1, 5, np.uint32)
    return pcs, starts, lens, prog_call, completed


def _run(gpu, pcs, starts, lens, prog_call, completed, dedup):
    cover = torch.full((pcs.size,), FILL, dtype=torch.int32, device=gpu.dev)
    cnt = torch.full((lens.size,), -1, dtype=torch.int32, device=gpu.dev)
    gpu.edge_cover(_t(gpu, pcs, np.int64), _t(gpu, starts, np.int64), _t(gpu, lens, np.int32),
                   _t(gpu, prog_call, np.int32), completed if torch.is_tensor(completed) else
                   _t(gpu, completed, np.int32), dedup=dedup, cover=cover, cover_cnt=cnt)
    return cover.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("dedup", [True, False])
def test_edge_cover_lengths_and_contents(gpu, dedup):
    pcs, starts, lens, prog_call, completed = _lengths_batch()
    # completed as edge_derive writes it for these traces (every PC passes cover_check)
    _, _, comp = gpu.edge_derive(_t(gpu, pcs, np.int64), _t(gpu, starts, np.int64), _t(gpu, lens, np.int32),
                                 _t(gpu, prog_call, np.int32))
    np.testing.assert_array_equal(comp.cpu().numpy().view(np.uint32), completed)
    cover, cnt = _run(gpu, pcs, starts, lens, prog_call, comp, dedup)
    ecover, ecnt = CR.edge_cover(pcs, starts, lens, prog_call, completed, dedup, fill=FILL)
    np.testing.assert_array_equal(cnt, ecnt)
    # bit-equal, the fill outside [call_start, +cover_cnt) included
    np.testing.assert_array_equal(cover, ecover)


def _one_program(gpu, chunks, dedup=True):
    """the chunks as the calls of one completed program -> (cover, cnt), checked against the restatement"""
    lens = np.array([c.size for c in chunks], np.uint32)
    starts = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    pcs = np.concatenate(chunks)
    prog_call = np.array([0, lens.size], np.uint32)
    completed = np.array([lens.size], np.uint32)
    cover, cnt = _run(gpu, pcs, starts, lens, prog_call, completed, dedup)
    ecover, ecnt = CR.edge_cover(pcs, starts, lens, prog_call, completed, dedup, fill=FILL)
    np.testing.assert_array_equal(cnt, ecnt)
    np.testing.assert_array_equal(cover, ecover)
    return cover, cnt


def test_edge_cover_pad_sizes_and_tile_counts(gpu):
    """3, 4 and 5 keys around the smallest padded sort; 3 T keys: an odd tile
    count, so the last run of a merge pass has no partner; 4 T: a full last
    tile and a power-of-two run count.  One call, so that the shorter long
    segments are copied through the later passes of the longest."""
    rng = np.random.default_rng(23)
    lens = [3, 4, 5, 3 * T, 4 * T]
    _, cnt = _one_program(gpu, [_contents(kind, n, rng) for n, kind in zip(lens, ["desc", "span", "dups", "span", "dups"])])
    assert cnt[0] == 3 and cnt[3] > 2 * T


def test_edge_cover_one_pc_repeated_past_two_tiles(gpu):
    """duplicates across every tile and run boundary: one survivor"""
    cover, cnt = _one_program(gpu, [_contents("equal", 2 * T + 1, None)])
    assert cnt.tolist() == [1] and cover[0] == 0x81000010


def test_edge_cover_aborts(gpu):
    rng = np.random.default_rng(5)
    nprog, cpp = 16, 8
    lens = rng.integers(1, 900, nprog * cpp).astype(np.uint32)
    starts = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    pcs = HI | (0x81000000 + 5 * rng.integers(0, 300, int(lens.sum())).astype(np.uint64))
    bad = rng.integers(0, cpp, nprog)
    for p in range(nprog):
        c = p * cpp + int(bad[p])
        pcs[int(starts[c]) + int(rng.integers(0, lens[c]))] = 0x1000 + p  # fails cover_check
    prog_call = synth.prog_call_index(nprog, cpp)
    d = [_t(gpu, pcs, np.int64), _t(gpu, starts, np.int64), _t(gpu, lens, np.int32), _t(gpu, prog_call, np.int32)]
    _, _, comp = gpu.edge_derive(*d)
    _, _, ocomp = O.exec_batch(pcs, starts, lens, prog_call)
    np.testing.assert_array_equal(comp.cpu().numpy().view(np.uint32), ocomp)
    np.testing.assert_array_equal(ocomp, bad)
    for dedup in (True, False):
        cover, cnt = _run(gpu, pcs, starts, lens, prog_call, comp, dedup)
        ecover, ecnt = CR.edge_cover(pcs, starts, lens, prog_call, ocomp, dedup, fill=FILL)
        np.testing.assert_array_equal(cnt, ecnt)
        np.testing.assert_array_equal(cover, ecover)
        for p in range(nprog):  # the aborting call and the later ones: nothing
            assert not cnt[p * cpp + bad[p]:(p + 1) * cpp].any()


@pytest.mark.parametrize("global_walk", [0, 1])
def test_edge_cover_c1_batch(gpu, global_walk):
    nprog, cpp, n = 64, 32, 2048
    cfg = synth.synth_default(global_walk=global_walk)
    cl = synth.call_lengths(nprog, cpp, n)
    pcs, cs, dcl, _ = gpu.synth_traces(cfg, 0, nprog, cpp, torch.from_numpy(cl.view(np.int32)))
    pidx = _t(gpu, synth.prog_call_index(nprog, cpp), np.int32)
    _, _, comp = gpu.edge_derive(pcs, cs, dcl, pidx)
    cover = torch.full((pcs.numel(),), FILL, dtype=torch.int32, device=gpu.dev)
    cover, cnt = gpu.edge_cover(pcs, cs, dcl, pidx, comp, cover=cover)
    hp = pcs.cpu().numpy().view(np.uint64)
    ecover, ecnt = CR.edge_cover(hp, cs.cpu().numpy(), cl, synth.prog_call_index(nprog, cpp),
                                 comp.cpu().numpy().view(np.uint32), True, fill=FILL)
    cnt = cnt.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(cnt, ecnt)
    np.testing.assert_array_equal(cover.cpu().numpy().view(np.uint32), ecover)
    assert cnt.min() > 0
    if not global_walk:
        assert cnt.max() <= 256  # a call walks one syscall's region of 2^8 blocks


def test_edge_cover_argument_checks(gpu):
    n = 262144 + 16
    pcs = _t(gpu, np.full(n, HI | np.uint64(0x81000000), np.uint64), np.int64)
    pidx = _t(gpu, np.array([0, 2], np.uint32), np.int32)
    comp = _t(gpu, np.array([2], np.uint32), np.int32)

    def rejected(starts, lens, completed):
        cover = torch.full((n,), FILL, dtype=torch.int32, device=gpu.dev)
        cnt = torch.full((2,), -1, dtype=torch.int32, device=gpu.dev)
        with pytest.raises(_lib.SyzsigError) as e:
            gpu.edge_cover(pcs, _t(gpu, np.array(starts, np.uint64), np.int64),
                           _t(gpu, np.array(lens, np.uint32), np.int32), pidx, completed, cover=cover, cover_cnt=cnt)
        assert e.value.code == _lib.SYZSIG_EINVAL
        torch.cuda.synchronize()
        assert bool((cover == FILL).all()) and bool((cnt == -1).all())  # nothing written

    rejected([0, 8], [4, 262144], comp)     # executor_linux.cc:186-187 "too much cover"
    rejected([0, 8], [4, 4], None)          # d_completed is required
    rejected([0, n - 2], [4, 4], comp)      # a range past npc
    rejected([0, 8], [4, 4], _t(gpu, np.array([3], np.uint32), np.int32))  # completed past the program's calls
    # ... and the accepted neighbour of the first: 262143 PCs
    cover, cnt = gpu.edge_cover(pcs, _t(gpu, np.array([0, 8], np.uint64), np.int64),
                                _t(gpu, np.array([4, 262143], np.uint32), np.int32), pidx, comp)
    assert cnt.cpu().tolist() == [1, 1]
