"""GPU: Device.edge_derive / Device.edge_cover with a KCOV target
(syzsig_edge_derive_target_dev, syzsig_edge_cover_target_dev): u32 traces
(PC32) and unchecked u64 PCs (target 0) beside today's x86-checked u64 PCs.
Every result must match exactly:

  - the reference executor's goldens, through the low-word identity (a signal
    depends on the PC's low 32 bits alone, tests/test_target_ref_cpu.py): PC32 is
    fed the low words, target 0 the low words under scrambled upper words;
  - tests/target_ref.py, the restatement, everywhere else.

Both marking modes of K2 are forced through the debug flags, as
tests/test_gpu_edge.py does."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import edge_traces as ET
from tests import target_ref as TR
from tests.conftest import golden_names
from tests.test_target_ref_cpu import _golden, _same, scramble_upper

pytestmark = pytest.mark.gpu

PC32, CHECK_X86 = TR.PC32, TR.CHECK_X86
NEW_TARGETS = [PC32, 0]
MODES = ["markall", "passes"]
M32 = np.uint64(0xFFFFFFFF)
FILL = 0x5EA1ED5E
T = 4096  # SYZSIG_COVER_TILE: the u32 tile's and the u64 tile's size alike (cover_tile.h CvTile64)


@pytest.fixture
def mode(gpu, request):
    from syzkaller_amd._lib import SYZSIG_DEBUG_EDGE_MARKALL, SYZSIG_DEBUG_EDGE_PASSES

    gpu.eng.set_debug({"markall": SYZSIG_DEBUG_EDGE_MARKALL, "passes": SYZSIG_DEBUG_EDGE_PASSES}[request.param])
    yield request.param
    gpu.eng.set_debug(0)


def _t(gpu, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def for_target(pcs, target, seed=7):
    """x86 PCs as the target's kernel would have traced them: their low words as
    u32 (PC32), or under scrambled upper words (0)."""
    pcs = np.asarray(pcs, np.uint64)
    if target == PC32:
        return (pcs & M32).astype(np.uint32)
    return scramble_upper(pcs, seed) if target == 0 else pcs


def _args(gpu, pcs, cs, cl, pc):
    return (_t(gpu, pcs, np.int32 if pcs.dtype == np.uint32 else np.int64), _t(gpu, np.asarray(cs, np.uint64), np.int64),
            _t(gpu, np.asarray(cl, np.uint32), np.int32), _t(gpu, np.asarray(pc, np.uint32), np.int32))


def _derive(gpu, pcs, cs, cl, pc, target, fill=None):
    sigs = None if fill is None else torch.full((pcs.size,), fill, dtype=torch.int32, device=gpu.dev)
    out = gpu.edge_derive(*_args(gpu, pcs, cs, cl, pc), sigs=sigs, target=target)
    torch.cuda.synchronize()
    return tuple(_u32(x) for x in out)


@functools.lru_cache(maxsize=None)
def _golden_case(name, target):
    """(the golden's traces as the target sees them, the restatement's result, the golden's own)"""
    tr, exp = _golden(name)
    tr = (for_target(tr[0], target),) + tr[1:]
    return tr, TR.exec_batch(*tr, target), exp


# ---- goldens on the device ----

@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_linux_amd64_target_is_todays_call(gpu, mode):
    tr, exp = _golden("executor_geometry")
    a = _args(gpu, *tr)
    d = tuple(_u32(x) for x in gpu.edge_derive(*a))
    t = tuple(_u32(x) for x in gpu.edge_derive(*a, target=CHECK_X86))
    for x, y in zip(d, t):
        np.testing.assert_array_equal(x, y)
    _same(t, exp, tr[1])


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("target", NEW_TARGETS)
@pytest.mark.parametrize("name", golden_names())
def test_goldens_under_new_targets(gpu, name, target, mode):
    """Against the golden's own exp_sigs / exp_cnt wherever the x86 check let the
    golden through (every call of a program that did not abort, and the calls
    before an abort), and against the restatement in full: the aborting calls
    of executor_abort / executor_geometry now complete, completed = every call
    (executor_big is the one call of 262143 PCs)."""
    tr, ref, exp = _golden_case(name, target)
    got = _derive(gpu, *tr, target)
    _same(got, exp, tr[1], tr[3], x86_only=True)
    _same(got, ref, tr[1])
    np.testing.assert_array_equal(got[2], np.diff(tr[3].astype(np.int64)))


# ---- seam lengths, alignments ----

SEAMS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]


@functools.lru_cache(maxsize=None)
def _seam_batch(target):
    """One program of one call per (length, alignment): the lane, chunk (256),
    prefetch-group (4 x 256) and double-buffer seams, each starting at
    call_start = 0, 1, 2, 3 modulo 4 (u32 words: every 4-byte alignment modulo
    16), with gap words that belong to no call before and after.  The walks
    repeat edges, so a call holds new signals and duplicates."""
    rng = np.random.default_rng(41)
    parts, cs, cl, pos = [], [], [], 0
    for n in SEAMS:
        for a in range(4):
            gap = (a - pos) % 4 + 4 * int(rng.integers(0, 2))
            parts.append(ET.region_walk(rng, gap, 5, 8))
            pos += gap
            assert pos % 4 == a
            parts.append(ET.region_walk(rng, n, int(rng.integers(0, 1 << 20)), 6))
            cs.append(pos)
            cl.append(n)
            pos += n
    parts.append(ET.region_walk(rng, 3, 5, 8))
    pcs = for_target(np.concatenate(parts), target, seed=43)
    tr = (pcs, np.array(cs, np.uint64), np.array(cl, np.uint32), np.arange(len(cs) + 1, dtype=np.uint32))
    return tr, TR.exec_batch(*tr, target)


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("target", NEW_TARGETS)
def test_seam_lengths_and_alignments(gpu, target, mode):
    tr, ref = _seam_batch(target)
    got = _derive(gpu, *tr, target, fill=FILL)
    _same(got, ref, tr[1])
    own = np.zeros(tr[0].size, bool)
    for s, n in zip(tr[1], tr[2]):
        own[int(s):int(s) + int(n)] = True
    assert (~own).sum() > 0 and (got[0][~own] == FILL).all()  # no word outside a call's range is written


# ---- structure-aimed programs ----

def _structure_sets():
    out = {f"dense_{n}": lambda n=n: ET.flat(ET.dense_set(n)) for n in sorted(ET.HOME_SETS)}
    out["dup_heavy"] = ET.dup_heavy_batch
    out["stride"] = lambda: ET.flat(ET.stride_batch()[0])
    return out


@functools.lru_cache(maxsize=None)
def _structure_case(name):
    tr = _structure_sets()[name]()
    return tr, O.exec_batch(*tr)


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("name", sorted(_structure_sets()))
def test_structure_aimed_programs_as_low_words(gpu, name, mode):
    """Dense conflicts at the bin and mark-word boundaries, a duplicate-heavy
    batch and the grid-stride batch, as a 32-bit kernel would trace them, against
    the compiled oracle on the x86 PCs (no program aborts)."""
    tr, exp = _structure_case(name)
    got = _derive(gpu, for_target(tr[0], PC32), *tr[1:], PC32)
    _same(got, exp, tr[1])


ZERO_AT = [0, 63, 64, 255, 256]  # lane 0, lane 63, a wave seam, the two sides of a chunk seam


@functools.lru_cache(maxsize=None)
def _zero_pc_batch(target):
    """PC 0 -- legal under the unchecked targets alone -- by position: as a
    call's first PC (sig 0 == the empty slot: a duplicate), as [0, 0, x] and as
    a lone zero inside a walk at each of ZERO_AT, and the hand program of
    tests/test_target_ref_cpu.py (slots 0..3 filled, then sig 0 forced into slot
    0, then a duplicate of it)."""
    rng = np.random.default_rng(47)
    progs = []
    for at in ZERO_AT:
        for pat in ([0], [0, 0, 0x1000]):
            w = ET.region_walk(rng, 300, int(rng.integers(0, 1 << 20)), 6)
            w[at:at + len(pat)] = pat
            progs.append([(False, w), (False, w[:at + 3].copy())])
    progs.append([(False, np.array([x], np.uint64)) for x in (0x2000, 0, 0x2001, 0x2002, 0x2003, 0, 0)])
    progs.append([(False, np.array([0], np.uint64))])
    pcs, cs, cl, pc = ET.flat(progs)
    # target 0: upper words over everything but the zero PCs
    tpcs = np.where(pcs == 0, pcs, for_target(pcs, target, seed=49)) if target == 0 else for_target(pcs, target)
    tr = (tpcs, cs, cl, pc)
    return tr, TR.exec_batch(*tr, target)


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("target", NEW_TARGETS)
def test_zero_pcs_by_position(gpu, target, mode):
    tr, ref = _zero_pc_batch(target)
    got = _derive(gpu, *tr, target)
    _same(got, ref, tr[1])
    hand = int(tr[3][-3])  # the hand program's first call
    assert got[1][hand:hand + 7].tolist() == [1, 0, 1, 1, 1, 1, 0] and got[1][-1] == 0
    assert got[0][int(tr[1][hand + 5])] == 0  # the forced zero signal is emitted


# ---- edge_cover ----

COVER_LENS = [T - 1, T, T + 1, 2 * T + 3]


@functools.lru_cache(maxsize=None)
def _cover_batch(target):
    """Per-call lengths around the tile (one workgroup in LDS up to T, the
    tile-sort and rank-merge path past it), low words drawn from a pool half
    the call's size so that duplicates abound; under target 0 a few upper
    words, so that equal low words meet under different upper words; a call
    whose PCs share one low word under distinct upper words; the two hand
    cases; gap words between the calls.  The last program aborts under
    CHECK_X86 in its second call (0x1000) and is an ordinary program under the
    other targets."""
    rng = np.random.default_rng(53)
    calls = []
    for n in COVER_LENS + [1, 3, 5, 257]:
        low = rng.integers(0, max(n // 2, 1), n).astype(np.uint64) * np.uint64(5) + np.uint64(0x81000000)
        up = rng.choice(np.array([0, 1, 2, 0xFFFFFFFF], np.uint64), n) if target == 0 else np.uint64(0xFFFFFFFF)
        calls.append((up << np.uint64(32)) | low)
    calls.append((np.arange(300, dtype=np.uint64) << np.uint64(32)) | np.uint64(5) if target != CHECK_X86
                 else np.full(300, 0xFFFFFFFF81000005, np.uint64))
    if target != CHECK_X86:
        calls.append(np.array([0x100000009, 0x200000003], np.uint64))
        calls.append(np.array([0x200000005, 5, 0x100000005, 5], np.uint64))
    progs = [[(False, c)] for c in calls]
    k = 0xFFFFFFFF81000000
    progs.append([(False, np.array([k + 7, k + 3, k + 7], np.uint64)), (False, np.array([k + 9, 0x1000, k + 1], np.uint64)),
                  (False, np.array([k + 2, k + 2], np.uint64))])
    gaps = {(p, 0): np.array([k + 11] * (1 + p % 3), np.uint64) for p in range(len(progs))}
    pcs, cs, cl, pc = ET.flat(progs, gaps)
    if target == PC32:
        pcs = (pcs & M32).astype(np.uint32)
    return pcs, cs, cl, pc


@pytest.mark.parametrize("dedup", [True, False])
@pytest.mark.parametrize("target", [CHECK_X86, PC32, 0])
def test_edge_cover_by_target(gpu, target, dedup):
    """Against the restatement.  Target 0 with dedup sorts and uniques u64 PCs
    before the truncation: an implementation that reuses the sort of the low
    words fails here on the order ([9, 3], not [3, 9]) and on the repeats
    ([5, 5, 5], not [5]; the shared-low-word call keeps all 300)."""
    tr = _cover_batch(target)
    a = _args(gpu, *tr)
    _, _, comp = gpu.edge_derive(*a, target=target)
    ref_comp = TR.exec_batch(*tr, target)[2]
    np.testing.assert_array_equal(_u32(comp), ref_comp)
    assert ref_comp[-1] == (1 if target == CHECK_X86 else 3)
    cover = torch.full((tr[0].size,), FILL, dtype=torch.int32, device=gpu.dev)
    cover, cnt = gpu.edge_cover(*a, comp, dedup=dedup, cover=cover, target=target)
    torch.cuda.synchronize()
    ecover, ecnt = TR.edge_cover(*tr, ref_comp, target, dedup, fill=FILL)
    np.testing.assert_array_equal(_u32(cnt), ecnt)
    np.testing.assert_array_equal(_u32(cover), ecover)  # (FILL wherever nothing is written: gaps, past a count)
    shared = len(COVER_LENS) + 4
    assert int(ecnt[shared]) == (300 if not dedup or target == 0 else 1)
    if target != CHECK_X86:
        c = _u32(cover)
        s9, s5 = int(tr[1][shared + 1]), int(tr[1][shared + 2])
        if dedup:
            assert c[s9:s9 + 2].tolist() == ([9, 3] if target == 0 else [3, 9])
            assert c[s5:s5 + int(ecnt[shared + 2])].tolist() == ([5, 5, 5] if target == 0 else [5])
        else:
            assert c[s9:s9 + 2].tolist() == [9, 3] and c[s5:s5 + 4].tolist() == [5, 5, 5, 5]
    if target == CHECK_X86:  # today's entry point gives the same
        cover2 = torch.full((tr[0].size,), FILL, dtype=torch.int32, device=gpu.dev)
        cover2, cnt2 = gpu.edge_cover(*a, comp, dedup=dedup, cover=cover2)
        assert torch.equal(cover2, cover) and torch.equal(cnt2, cnt)


# ---- error paths ----

@pytest.mark.parametrize("target", [PC32 | CHECK_X86, 4, 1 << 31])
def test_invalid_target_is_einval_and_writes_nothing(gpu, target):
    from syzkaller_amd._lib import SYZSIG_EINVAL, SyzsigError

    pcs = np.full(16, 0xFFFFFFFF81000000, np.uint64)
    a = _args(gpu, pcs, [0, 8], [8, 8], [0, 1, 2])
    mk = lambda n: torch.full((n,), FILL, dtype=torch.int32, device=gpu.dev)  # noqa: E731
    sigs, cnt, comp = mk(16), mk(2), mk(2)
    with pytest.raises(SyzsigError) as e:
        gpu.edge_derive(*a, sigs=sigs, sig_cnt=cnt, completed=comp, target=target)
    assert e.value.code == SYZSIG_EINVAL
    cover, ccnt = mk(16), mk(2)
    done = _t(gpu, np.array([1, 1], np.uint32), np.int32)
    with pytest.raises(SyzsigError) as e:
        gpu.edge_cover(*a, done, cover=cover, cover_cnt=ccnt, target=target)
    assert e.value.code == SYZSIG_EINVAL
    torch.cuda.synchronize()
    for x in (sigs, cnt, comp, cover, ccnt):
        assert (_u32(x) == FILL).all()


def test_dtype_that_contradicts_the_target(gpu):
    p64 = np.full(8, 0xFFFFFFFF81000000, np.uint64)
    p32 = np.full(8, 0x81000000, np.uint32)
    done = _t(gpu, np.array([1], np.uint32), np.int32)
    for pcs, targets in ((p32, (0, CHECK_X86)), (p64, (PC32,))):
        a = _args(gpu, pcs, [0], [8], [0, 1])
        for t in targets:
            sigs = torch.full((8,), FILL, dtype=torch.int32, device=gpu.dev)
            with pytest.raises(ValueError):
                gpu.edge_derive(*a, sigs=sigs, target=t)
            with pytest.raises(ValueError):
                gpu.edge_cover(*a, done, cover=sigs, target=t)
            assert (_u32(sigs) == FILL).all()


# ---- chain ----

def test_pc32_traces_through_triage_equal_the_widened_x86_traces(gpu):
    """PC32 traces -> edge_derive -> triage flags the same calls as the same
    traces widened to x86 PCs through today's path (the caller's workaround
    this target replaces)."""
    from syzkaller_amd import signal as S
    from syzkaller_amd import synth

    cfg = synth.synth_default()
    nprog, cpp = 8, 8
    cl = synth.call_lengths(nprog, cpp, 0, ragged=(0, 2000), seed=3)
    pcs, cs, prio = synth.traces(cfg, 0, nprog, cpp, cl)
    pidx = synth.prog_call_index(nprog, cpp)
    m0e, m0p = synth.m0(cfg, 64, 20000)
    res = []
    for tpcs, target in ((pcs, None), (for_target(pcs, PC32), PC32)):
        a = _args(gpu, tpcs, cs, cl, pidx)
        sigs, cnt, comp = gpu.edge_derive(*a, target=target)
        ms = S.Serial(m0e, m0p).Deserialize(gpu.eng)
        ns = S.Signal(None, gpu.eng)
        _, cnew, _ = gpu.triage(ms, ns, sigs, a[1], cnt, _t(gpu, prio, np.uint8))
        torch.cuda.synchronize()
        res.append((cnew.cpu().numpy(), _u32(cnt), ns.to_dict()))
    assert res[0][0].sum() > 0
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]
