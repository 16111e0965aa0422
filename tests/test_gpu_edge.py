"""GPU: K1+K2 (edge.hip) bit-exact against the reference executor's own output
(golden vectors) and against the oracle on larger synthetic batches, and on
the traces of tests/edge_traces.py, built for the kernel's own structure
(tests/test_edge_rounds_cpu.py checks on CPU that they have the shape they
were built for).  The one path of the kernel with no test is the epoch wrap
(epoch == kEpochMax): reaching it takes 2^24 - 1 rounds inside one program,
more than 4 * 10^9 PCs."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import edge_traces as ET
from tests.conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

# K2's two marking modes (edge.hip), forced; None = the library's own choice
MODES = [None, "markall", "passes"]


@pytest.fixture
def mode(gpu, request):
    from syzkaller_amd._lib import SYZSIG_DEBUG_EDGE_MARKALL, SYZSIG_DEBUG_EDGE_PASSES

    m = request.param
    gpu.eng.set_debug({None: 0, "markall": SYZSIG_DEBUG_EDGE_MARKALL, "passes": SYZSIG_DEBUG_EDGE_PASSES}[m])
    yield m
    gpu.eng.set_debug(0)


def _run(gpu, pcs, call_start, call_len, prog_call):
    d = gpu.dev
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(d)  # noqa: E731
    sigs, cnt, comp = gpu.edge_derive(t(pcs, np.int64), t(call_start, np.int64), t(call_len, np.int32),
                                      t(prog_call, np.int32))
    torch.cuda.synchronize()
    return (sigs.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32),
            comp.cpu().numpy().view(np.uint32))


def _check(fx_sigs, fx_cnt, fx_comp, call_start, sigs, cnt, comp):
    np.testing.assert_array_equal(comp, fx_comp)
    np.testing.assert_array_equal(cnt, fx_cnt)
    for c in range(len(call_start)):
        s, n = int(call_start[c]), int(fx_cnt[c])
        np.testing.assert_array_equal(sigs[s: s + n], fx_sigs[s: s + n], err_msg=f"call {c}")


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("name", golden_names())
def test_edge_matches_reference_executor_goldens(gpu, name, mode):
    fx = load_golden(name)
    out = _run(gpu, fx["pcs"], fx["call_start"], fx["call_len"], fx["prog_call"])
    _check(fx["exp_sigs"], fx["exp_cnt"], fx["exp_completed"], fx["call_start"], *out)


@pytest.mark.parametrize("over,ragged", [({}, None), ({"region_log2": 12}, (0, 3000)),
                                          ({"bad_pc_ppm": 20}, (0, 4000)), ({"skew": 1}, None),
                                          ({"global_walk": 1}, None)])
@pytest.mark.parametrize("mode", MODES[1:], indirect=True)
def test_edge_c1_batch_vs_oracle(gpu, over, ragged, mode):
    """Config 1 shape: 64 programs x 32 calls x 2k PCs (ragged variants)."""
    from syzkaller_amd import synth

    cfg = synth.synth_default(**over)
    nprog, cpp = 64, 32
    cl = synth.call_lengths(nprog, cpp, 2048, ragged=ragged, seed=1)
    pcs, cs, prio = synth.traces(cfg, 0, nprog, cpp, cl)
    pidx = synth.prog_call_index(nprog, cpp)
    exp = O.exec_batch(pcs, cs, cl, pidx)
    out = _run(gpu, pcs, cs, cl, pidx)
    _check(*exp, cs, *out)


@pytest.mark.parametrize("over", [{"skew": 1}, {"skew": 2, "global_walk": 1}])
def test_device_synth_matches_host(gpu, over):
    from syzkaller_amd import synth

    cfg = synth.synth_default(**over)
    cl = synth.call_lengths(16, 8, 0, ragged=(0, 3000), seed=4)
    pcs, cs, prio = synth.traces(cfg, 5, 16, 8, cl)
    dpcs, dcs, dcl, dprio = gpu.synth_traces(cfg, 5, 16, 8, torch.from_numpy(cl.view(np.int32)))
    np.testing.assert_array_equal(dpcs.cpu().numpy().view(np.uint64), pcs)
    np.testing.assert_array_equal(dprio.cpu().numpy(), prio)
    e, p = synth.m0(cfg, 10, 20000)
    de, dp = gpu.synth_m0(cfg, 10, 20000)
    np.testing.assert_array_equal(de.cpu().numpy().view(np.uint32), e)
    np.testing.assert_array_equal(dp.cpu().numpy(), p)


def test_edge_rejects_oversized_call(gpu):
    from syzkaller_amd._lib import SyzsigError

    n = 262144  # kCoverSize: executor_linux.cc:186-187 fail("too much cover")
    pcs = np.full(n, 0xFFFFFFFF81000000, np.uint64)
    with pytest.raises(SyzsigError):
        _run(gpu, pcs, np.array([0], np.uint64), np.array([n], np.uint32), np.array([0, 1], np.uint32))


@pytest.mark.parametrize("mode", ["markall"], indirect=True)
def test_edge_markall_clear_after_one_round_chunks(gpu, mode):
    """in the mark-all mode a chunk that leaves no lane
    pending after its first round clears its slot marks and returns with no
    barrier behind the clear, while the next chunk of the same prefetch group
    marks with no K1 barrier in front of it.  The trace alternates such chunks
    with chunks of colliding pairs (whose lost marks would let a blocked lane
    write), over 1024 programs so many waves interleave; bit-exact against the
    oracle (which the CPU test pins to the round restatement's shape)."""
    from tests.test_edge_rounds_cpu import clear_race_trace

    pcs, cs, cl, pidx = clear_race_trace(1024, nchunks=16, seed=11)
    exp = O.exec_batch(pcs, cs, cl, pidx)
    for _ in range(3):
        out = _run(gpu, pcs, cs, cl, pidx)
        _check(*exp, cs, *out)


@functools.lru_cache(maxsize=None)
def _with_oracle(build, *args):
    """(pcs, call_start, call_len, prog_call) of a builder and the oracle's
    (sigs, sig_cnt, completed) for it: computed once, shared by the modes."""
    tr = build(*args)
    return tr, O.exec_batch(*tr)


def _dense_draw(name):
    # a larger draw than the executor_dense fixture, fresh seeds
    return ET.flat(ET.dense_set(name, nprog=64, seed=100 + ET.DENSE_FIXTURE_SEEDS[name]))


@pytest.mark.parametrize("mode", MODES[1:], indirect=True)
@pytest.mark.parametrize("home_set", sorted(ET.HOME_SETS))
def test_edge_dense_conflicts_vs_oracle(gpu, home_set, mode):
    """Matches, inserts into empty slots and forced overwrites of a few
    repeated values in one bin inside one chunk, at homes chosen for the
    second-bin stamp, the mark mask's spill into the next fm1/fm2 word, the
    last mark words and the windows that hold slot 0."""
    tr, exp = _with_oracle(_dense_draw, home_set)
    _check(*exp, tr[1], *_run(gpu, *tr))


def _geometry():
    return ET.flat(*ET.geometry_programs())


@pytest.mark.parametrize("mode", MODES[1:], indirect=True)
def test_edge_call_length_geometry(gpu, mode):
    """Call lengths at the edges of a wave, a chunk (256), a prefetch group
    (1024) and the two buffers (2048), contiguous and with gaps between the
    calls.  sigs goes in pre-filled: no word outside a call's range is
    written (inside it, past sig_cnt, the content is unspecified)."""
    (pcs, cs, cl, pc), exp = _with_oracle(_geometry)
    sentinel = 0x5EA1ED5E
    own = np.zeros(pcs.size, bool)
    for c in range(cs.size):
        own[int(cs[c]): int(cs[c]) + int(cl[c])] = True
    assert (~own).sum() > 0
    d = gpu.dev
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(d)  # noqa: E731
    sigs = torch.full((pcs.size,), sentinel, dtype=torch.int32, device=d)
    sigs, cnt, comp = gpu.edge_derive(t(pcs, np.int64), t(cs, np.int64), t(cl, np.int32), t(pc, np.int32), sigs=sigs)
    torch.cuda.synchronize()
    sigs = sigs.cpu().numpy().view(np.uint32)
    _check(*exp, cs, sigs, cnt.cpu().numpy().view(np.uint32), comp.cpu().numpy().view(np.uint32))
    assert (sigs[~own] == sentinel).all()


def _abort_positions():
    progs, gaps, completed = ET.abort_position_programs()
    return ET.flat(progs, gaps)


@pytest.mark.parametrize("mode", MODES[1:], indirect=True)
def test_edge_abort_positions(gpu, mode):
    """A cover_check failure as the only signal of a call's fifth chunk, at
    lane 63 / 64, at the last / first position of a chunk and of a group, as a
    program's first PC; and failing PCs between the calls, which abort
    nothing."""
    (pcs, cs, cl, pc), exp = _with_oracle(_abort_positions)
    completed = ET.abort_position_programs()[2]
    sigs, cnt, comp = _run(gpu, pcs, cs, cl, pc)
    np.testing.assert_array_equal(comp, completed)
    _check(*exp, cs, sigs, cnt, comp)  # exp_cnt bounds the compared words: the published calls' signals
    for p in range(pc.size - 1):
        assert (cnt[int(pc[p]) + int(completed[p]): int(pc[p + 1])] == 0).all(), p


def _stride():
    return ET.flat(ET.stride_batch()[0])


@pytest.mark.parametrize("mode", MODES[1:], indirect=True)
def test_edge_grid_stride_resets_program_state(gpu, mode):
    """One workgroup runs two or three programs: the second run of a program
    starts from the table, stamps and marks its first run left in the same
    workgroup, and must give the same output."""
    (pcs, cs, cl, pc), exp = _with_oracle(_stride)
    origin = ET.stride_batch()[1]
    nprog = pc.size - 1
    assert nprog > 1024  # edge.hip's grid cap (min(nprog, 256 * 4)): program p + 1024 runs after p in p's workgroup
    sigs, cnt, comp = _run(gpu, pcs, cs, cl, pc)
    _check(*exp, cs, sigs, cnt, comp)
    for p in range(1024, nprog):
        o = int(origin[p])
        assert comp[p] == comp[o]
        for c, co in zip(range(int(pc[p]), int(pc[p + 1])), range(int(pc[o]), int(pc[o + 1]))):
            assert cnt[c] == cnt[co]
            np.testing.assert_array_equal(sigs[int(cs[c]): int(cs[c]) + int(cnt[c])],
                                          sigs[int(cs[co]): int(cs[co]) + int(cnt[co])], err_msg=f"program {p}")


def _clear_race16():
    from tests.test_edge_rounds_cpu import clear_race_trace

    return clear_race_trace(16)


def test_edge_mode_choice_follows_previous_launch(gpu):
    """The library's own mode choice (no debug flag): the dense batch after a
    duplicate-heavy launch and after a duplicate-free one, which lie on
    opposite sides of the host's 5 % rule (test_edge_rounds_cpu.py
    test_mode_choice_primers_lie_on_both_sides), so the two dense launches run
    in different modes.  The library does not report which; both are exact."""
    gpu.eng.set_debug(0)
    dense, dexp = _with_oracle(_dense_draw, "bin_edge")
    for primer in (ET.dup_heavy_batch, _clear_race16):
        tr, exp = _with_oracle(primer)
        _check(*exp, tr[1], *_run(gpu, *tr))
        _check(*dexp, dense[1], *_run(gpu, *dense))


def _malformed_cases():
    n = 262144  # kCoverSize
    pcs = ET.region_walk(np.random.default_rng(5), 300, 77, 8)
    u64, u32 = (lambda *a: np.array(a, np.uint64)), (lambda *a: np.array(a, np.uint32))
    big = np.full(100 + n, 0xFFFFFFFF81000000, np.uint64)
    return {
        "prog_call_decreasing": (pcs, u64(0, 100, 200), u32(100, 100, 100), u32(0, 2, 1, 1)),
        "prog_call_past_ncalls": (pcs, u64(0, 100), u32(100, 100), u32(0, 1, 5)),
        "call_start_past_npc": (pcs, u64(0, 305), u32(100, 0), u32(0, 1, 2)),
        "call_end_past_npc": (pcs, u64(0, 290), u32(100, 20), u32(0, 1, 2)),
        "oversized_call_in_second_program": (big, u64(0, 100), u32(100, n), u32(0, 1, 2)),
    }


@pytest.mark.parametrize("case", sorted(_malformed_cases()))
def test_edge_rejects_malformed_ranges(gpu, case):
    from syzkaller_amd._lib import SYZSIG_EINVAL, SyzsigError

    with pytest.raises(SyzsigError) as e:
        _run(gpu, *_malformed_cases()[case])
    assert e.value.code == SYZSIG_EINVAL
    # the engine is usable after the error: a well-formed launch is exact
    tr, exp = _with_oracle(_abort_positions)
    _check(*exp, tr[1], *_run(gpu, *tr))
