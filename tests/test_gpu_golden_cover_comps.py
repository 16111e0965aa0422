"""GPU: Device.edge_cover, Device.exec_comps and the consumers of executor
output regions (ingest -> CompMap, ingest -> triage_cover) against what the
REFERENCE executor itself wrote: the fixtures under tests/golden/cover and
tests/golden/comps (oracle/_ref/ref_harness runs the reference's
handle_completion with flag_collect_cover / flag_collect_comps; generators
tests/golden/make_golden_cover.py, make_golden_comps.py).  Device output is
compared with the reference's words directly, bit for bit; only the fixtures
are read.

shrink_expand is not here: prog/hints.go is Go, which the build machine cannot
compile, so it stays checked against the restatement (tests/test_gpu_hints.py)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from syzkaller_amd import _lib
from syzkaller_amd.hints import CompMap
from tests import comps_ref as R
from tests import cover_ref as CR
from tests import golden_sets as GS

pytestmark = pytest.mark.gpu

FILL = 0x12345678  # no PC's low word (cover_check keeps them in 0x80000000..0xfeffffff); no fixture's comps word


def _t(gpu, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _filled(exp, start, cnt, scale=1):
    """`exp` where a call's list lies (scale * start[c] .. + cnt[c]), FILL everywhere else"""
    out = np.full(exp.size, FILL, np.uint32)
    for s, n in zip(start, cnt):
        s = scale * int(s)
        out[s:s + int(n)] = exp[s:s + int(n)]
    return out


@pytest.mark.parametrize("name", GS.COVER_NAMES)
def test_edge_cover_matches_reference_executor(gpu, name):
    fx = GS.load_cover(name)
    a = [_t(gpu, fx["pcs"], np.int64), _t(gpu, fx["call_start"], np.int64), _t(gpu, fx["call_len"], np.int32),
         _t(gpu, fx["prog_call"], np.int32)]
    _, _, comp = gpu.edge_derive(*a)
    np.testing.assert_array_equal(_u32(comp), fx["exp_completed"])
    cover = torch.full((fx["pcs"].size,), FILL, dtype=torch.int32, device=gpu.dev)
    cnt = torch.full((fx["call_len"].size,), -1, dtype=torch.int32, device=gpu.dev)
    gpu.edge_cover(*a, comp, dedup=bool(fx["dedup"]), cover=cover, cover_cnt=cnt)
    cover, cnt = _u32(cover), _u32(cnt)
    np.testing.assert_array_equal(cnt, fx["exp_cover_cnt"])  # 0 for the calls without a record
    for c in range(cnt.size):
        s, n = int(fx["call_start"][c]), int(cnt[c])
        np.testing.assert_array_equal(cover[s:s + n], fx["exp_cover"][s:s + n], err_msg=f"call {c}")
    # nothing is written outside the lists, so nothing at all for a call without a record
    np.testing.assert_array_equal(cover, _filled(fx["exp_cover"], fx["call_start"], fx["exp_cover_cnt"]))


def _exec_comps(gpu, fx, sel):
    ncmp = fx["comps"].shape[0]
    out = torch.full((5 * ncmp,), FILL, dtype=torch.int32, device=gpu.dev)
    nw = torch.full((sel.size,), FILL, dtype=torch.int32, device=gpu.dev)
    cnt = torch.full((sel.size,), FILL, dtype=torch.int32, device=gpu.dev)
    gpu.exec_comps(_t(gpu, fx["comps"], np.int64), _t(gpu, fx["call_start"][sel], np.int64),
                   _t(gpu, fx["call_len"][sel], np.int32), int(fx["out_start"]), out=out, out_words=nw, comps_cnt=cnt)
    return out, nw, cnt


def _completed(fx):
    return np.array([c for p in range(fx["prog_call"].size - 1)
                     for c in range(int(fx["prog_call"][p]), int(fx["prog_call"][p]) + int(fx["exp_completed"][p]))],
                    np.int64)


@pytest.mark.parametrize("name", GS.COMPS_NAMES)
def test_exec_comps_matches_reference_executor(gpu, name):
    fx = GS.load_comps(name)
    assert FILL not in fx["exp_words"]
    sel = _completed(fx)  # the calls the reference wrote a record for
    out, nw, cnt = (_u32(x) for x in _exec_comps(gpu, fx, sel))
    np.testing.assert_array_equal(nw, fx["exp_out_words"][sel])
    np.testing.assert_array_equal(cnt, fx["exp_comps_cnt"][sel])
    for c in sel:
        s, n = 5 * int(fx["call_start"][c]), int(fx["exp_out_words"][c])
        np.testing.assert_array_equal(out[s:s + n], fx["exp_words"][s:s + n], err_msg=f"call {c}")
    np.testing.assert_array_equal(out, _filled(fx["exp_words"], fx["call_start"][sel], fx["exp_out_words"][sel], 5))


def test_exec_comps_refuses_where_the_reference_fails(gpu):
    """The call the reference's child died in (fail("too many comparisons"),
    exit status 67): 65536 records.  Refused, nothing written; its neighbour of
    65535 records is the `toomany` case of the test above."""
    fx = GS.load_comps("toomany")
    assert fx["exp_status"].tolist() == [GS.K_FAIL_STATUS, 0]
    bad = int(fx["prog_call"][0]) + int(fx["exp_completed"][0])
    assert int(fx["call_len"][bad]) == 65536
    ncmp = fx["comps"].shape[0]
    out = torch.full((5 * ncmp,), FILL, dtype=torch.int32, device=gpu.dev)
    nw = torch.full((2,), FILL, dtype=torch.int32, device=gpu.dev)
    cnt = torch.full((2,), FILL, dtype=torch.int32, device=gpu.dev)
    with pytest.raises(_lib.SyzsigError) as e:
        gpu.exec_comps(_t(gpu, fx["comps"], np.int64), _t(gpu, fx["call_start"][bad - 1:bad + 1], np.int64),
                       _t(gpu, fx["call_len"][bad - 1:bad + 1], np.int32), int(fx["out_start"]), out=out, out_words=nw,
                       comps_cnt=cnt)
    assert e.value.code == _lib.SYZSIG_EINVAL
    torch.cuda.synchronize()
    for t in (out, nw, cnt):
        assert bool((t == FILL).all())


def _ingest(gpu, fx):
    ncalls = np.diff(fx["prog_call"])
    call_num = np.concatenate([np.arange(n) for n in ncalls]).astype(np.uint32)
    dout = _t(gpu, fx["regions"], np.int32)
    ing = gpu.ingest_exec_output(dout, _t(gpu, fx["region_off"], np.int64), _t(gpu, fx["prog_call"], np.int32),
                                 torch.zeros(call_num.size, dtype=torch.uint8, device=gpu.dev),
                                 call_num=_t(gpu, call_num, np.int32), want_cover=True)
    regions = [fx["regions"][int(fx["region_off"][p]):int(fx["region_off"][p + 1])] for p in range(ncalls.size)]
    host = O.ingest_batch(regions, ncalls.tolist(), np.zeros(call_num.size, np.uint8), call_num)
    np.testing.assert_array_equal(ing["prog_status"].cpu().numpy(), host[7])
    np.testing.assert_array_equal(ing["call_errno"].cpu().numpy(), host[6])
    assert ing["n_failed"] == int((host[7] != 0).sum())
    return dout, ing, regions, host


@pytest.mark.parametrize("name", GS.COMPS_NAMES)
def test_reference_written_comps_regions_to_comp_map(gpu, name):
    """regions -> ingest -> CompMap.from_regions, and comp_map on every call's
    framed words, against comps_ref.parse_comps on the same regions (held to
    them by tests/test_golden_cover_comps_cpu.py)."""
    fx = GS.load_comps(name)
    dout, ing, regions, host = _ingest(gpu, fx)
    nprog = fx["prog_call"].size - 1
    frames = {c: (ws, we) for p in range(nprog) for c, ws, we in GS.comps_region_calls(fx, p)}
    ncalls = fx["call_len"].size
    m = CompMap.from_regions(gpu, dout, ing)
    off, pairs = m.off.cpu().tolist(), m.pairs.cpu().numpy().view(np.uint64).reshape(-1, 2)
    st = m.status.cpu().tolist()
    for c in range(ncalls):
        p = int(np.searchsorted(fx["prog_call"], c, side="right")) - 1
        if c in frames and host[7][p] == 0:  # an executed call of a program that parsed
            est, em = R.parse_comps(fx["regions"], frames[c][0], int(fx["exp_comps_cnt"][c]), frames[c][1])
            assert est == R.INGEST_OK
        else:  # Errno = -1: no comparisons
            est, em = R.INGEST_OK, {}
        assert st[c] == est, c
        np.testing.assert_array_equal(pairs[off[c]:off[c + 1]], R.map_pairs(em), err_msg=f"call {c}")
    # ... and per call, the programs that failed the region parse included: the type above 7 is reported
    sel = sorted(frames)
    start = np.array([frames[c][0] for c in sel], np.uint64)
    end = np.array([frames[c][1] for c in sel], np.uint64)
    cnt = fx["exp_comps_cnt"][sel]
    got = gpu.comp_map(dout, _t(gpu, start, np.int64), _t(gpu, cnt, np.int32), _t(gpu, end, np.int64))
    est, eoff, epairs, _ = R.comp_map(fx["regions"], start, cnt, end)
    np.testing.assert_array_equal(got[0].cpu().numpy(), est)
    np.testing.assert_array_equal(got[1].cpu().numpy().view(np.uint64), eoff)
    np.testing.assert_array_equal(got[2].cpu().numpy().view(np.uint64).reshape(-1, 2), epairs)
    if name == "edges":
        bad = [i for i, c in enumerate(sel) if c >= int(fx["prog_call"][1])]
        assert est[bad].tolist() == [R.INGEST_ECOMPTYPE] * 3 and not est[: bad[0]].any()
        assert host[7].tolist() == [O.INGEST_OK, O.INGEST_ECOMPTYPE]
    assert epairs.shape[0] > 0


@pytest.mark.parametrize("name", ["abort_dedup0", "abort_dedup1"])
def test_reference_written_cover_regions_to_triage_cover(gpu, name):
    """regions with the reference's signal and cover lists -> ingest ->
    triage_runs + triage_cover (its "regions" source): every call is a re-run,
    three consecutive calls an item.  Expected: proc.go:107-140 restated
    (cover_ref.triage_cover) over the lists readOutCoverage's restatement takes
    from the same regions."""
    fx = GS.load_cover(name)
    dout, ing, regions, host = _ingest(gpu, fx)
    assert ing["n_failed"] == 0
    words, _, _, cs, cl, _, errno, _ = host
    np.testing.assert_array_equal(ing["call_len"].cpu().numpy().view(np.uint32), cl)
    nruns, runs = cl.size, 3
    nitems = nruns // runs
    assert nitems * runs == nruns
    run_sigs = [words[int(cs[r]):int(cs[r]) + int(cl[r])] for r in range(nruns)]
    run_cover = []
    for p in range(fx["prog_call"].size - 1):
        n = int(fx["prog_call"][p + 1] - fx["prog_call"][p])
        _, info = O.read_out_coverage(regions[p], n, list(range(n)))
        run_cover += [regions[p][i[3]:i[3] + i[4]] if i is not None else np.empty(0, np.uint32) for i in info]
    # the device's ranges are the reference's lists
    dcs, dcl = ing["cover_start"].cpu().numpy(), ing["cover_len"].cpu().numpy()
    for r in range(nruns):
        np.testing.assert_array_equal(fx["regions"][int(dcs[r]):int(dcs[r]) + int(dcl[r])], run_cover[r])
        s = int(fx["call_start"][r])
        np.testing.assert_array_equal(run_cover[r], fx["exp_cover"][s:s + int(fx["exp_cover_cnt"][r])])
    rng = np.random.default_rng(3)
    elems = []
    for i in range(nitems):  # newSignal: the signal of the item's first run that has any
        first = next((s for s in run_sigs[i * runs:(i + 1) * runs] if s.size), np.empty(0, np.uint32))
        elems.append(np.unique(first))
    item_off = np.cumsum([0] + [e.size for e in elems]).astype(np.uint64)
    elems = np.concatenate(elems).astype(np.uint32)
    prios = np.zeros(elems.size, np.int8)
    flags = rng.integers(0, 4, nitems).astype(np.uint8)
    run_off = np.cumsum([0] + [s.size for s in run_sigs]).astype(np.uint64)
    run_prio = np.full(nruns, 3, np.uint8)
    run_exec = (errno != -1).astype(np.uint8)
    run_errno = np.where(errno == -1, 0, errno).astype(np.int32)
    ekeep, ecovers = CR.triage_cover(item_off, elems, prios, flags, runs, run_off, np.concatenate(run_sigs), run_prio,
                                     run_errno, run_exec, run_cover)
    d = dict(flags=_t(gpu, flags, np.uint8), run_off=_t(gpu, run_off, np.int64), run_errno=_t(gpu, run_errno, np.int32),
             run_exec=_t(gpu, run_exec, np.uint8))
    keep, _ = gpu.triage_runs(_t(gpu, item_off, np.int64), _t(gpu, elems, np.int32), _t(gpu, prios, np.int8),
                              d["flags"], runs, d["run_off"], _t(gpu, np.concatenate(run_sigs), np.int32),
                              _t(gpu, run_prio, np.uint8), d["run_errno"], d["run_exec"])
    np.testing.assert_array_equal(keep.cpu().numpy(), ekeep)
    off, cover = gpu.triage_cover(d["flags"], keep, runs, d["run_off"], d["run_errno"], d["run_exec"], dout,
                                  ing["cover_start"], ing["cover_len"])
    np.testing.assert_array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum([c.size for c in ecovers])]))
    np.testing.assert_array_equal(_u32(cover), np.concatenate(ecovers).astype(np.uint32))
    assert 0 < ekeep.sum() < nitems and sum(c.size for c in ecovers) > 0
