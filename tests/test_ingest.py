"""Executor output regions -> triage batch (pkg/ipc/ipc.go:328-468 readOutCoverage).

CPU: the readOutCoverage restatement against the REFERENCE executor's own
regions (oracle/_ref/ref_harness, container only) and the committed fixture.
GPU: k_ingest_exec_output bit-exact against the fixture (well-formed regions
written by the reference executor plus one corrupted region per ipc.go error
branch), then ingest -> checkNewSignal end to end against the oracle.

The regions of tests/ingest_cases.py (written by hand: the accepting and the
rejecting side of every length check, programs of 256 calls and more, 600
programs over three workgroups) are checked on the CPU against their
hand-stated status and on the GPU against the restatement, array by array."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import ingest_cases as IC
from tests.conftest import GOLDEN

FIX = os.path.join(GOLDEN, "ingest", "exec_regions.npz")


def load():
    with np.load(FIX, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def regions_of(fx):
    po = fx["prog_off"].astype(np.int64)
    pc = fx["prog_call"].astype(np.int64)
    regs = [fx["out"][po[p]:po[p + 1]] for p in range(po.size - 1)]
    return regs, np.diff(pc)


def test_fixture_reproduced_by_restatement():
    fx = load()
    regs, ncalls = regions_of(fx)
    out, po, pc, cs, cl, cp, ce, st = O.ingest_batch(regs, ncalls, fx["call_any"], fx["call_num"])
    for k, v in dict(out=out, prog_off=po, prog_call=pc, exp_call_start=cs, exp_call_len=cl, exp_call_prio=cp,
                     exp_call_errno=ce, exp_status=st).items():
        np.testing.assert_array_equal(v, fx[k], err_msg=k)
    # one region per ipc.go error branch is present
    assert set(range(1, 10)) <= set(st.tolist())


@pytest.mark.skipif(not os.path.exists(O.REF_HARNESS), reason="reference executor harness not built (container only)")
def test_restatement_vs_reference_executor_regions():
    from syzkaller_amd import synth

    progs = []
    cfg = synth.synth_default(bad_pc_ppm=200)
    cl = synth.call_lengths(12, 6, 0, ragged=(0, 2500), seed=5)
    pcs, cs, prio = synth.traces(cfg, 900, 12, 6, cl)
    for p in range(12):
        progs.append([(((prio[c] >> 1) & 1) == 0, pcs[cs[c]:cs[c] + cl[c]]) for c in range(p * 6, (p + 1) * 6)])
    regions = O.run_reference_executor(progs, raw=True)
    parsed = O.run_reference_executor(progs)
    for reg, (completed, calls) in zip(regions, parsed):
        st, info = O.read_out_coverage(reg, 6, list(range(6)))
        assert st == 0 and sum(i is not None for i in info) == completed
        for idx, err, sigs in calls:
            e, so, sl, _, _ = info[idx]
            assert e == err
            np.testing.assert_array_equal(reg[so:so + sl], sigs)


def test_frame_exec_output_roundtrip():
    """The synthetic framer writes regions the restatement parses back."""
    from syzkaller_amd import synth

    sigs = np.arange(100, dtype=np.uint32)
    cs = np.array([0, 10, 30, 60], np.uint64)
    cnt = np.array([5, 0, 20, 7], np.uint32)
    out, off = synth.frame_exec_output(sigs, cs, cnt, [2, 1], np.array([0, 2, 4]), np.array([0, -1, 22, 0]),
                                       order_seed=3)
    st0, i0 = O.read_out_coverage(out[off[0]:off[1]], 2)
    st1, i1 = O.read_out_coverage(out[off[1]:off[2]], 2)
    assert st0 == st1 == 0
    assert i0[0][0] == 0 and i0[0][2] == 5 and i0[1][0] == -1 and i0[1][2] == 0
    assert i1[0][0] == 22 and i1[0][2] == 20 and i1[1] is None


def _dev_ingest(gpu, out, po, pc, call_any, call_num, want_cover=False):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu.dev)  # noqa: E731
    r = gpu.ingest_exec_output(t(out, np.int32), t(po, np.int64), t(pc, np.int32), t(call_any, np.uint8),
                               None if call_num is None else t(call_num, np.int32), want_cover=want_cover)
    return t(out, np.int32), r


def _np(x, dt):
    return x.cpu().numpy().view(dt)


@pytest.mark.gpu
def test_ingest_matches_fixture(gpu):
    fx = load()
    _, r = _dev_ingest(gpu, fx["out"], fx["prog_off"], fx["prog_call"], fx["call_any"], fx["call_num"],
                       want_cover=True)
    np.testing.assert_array_equal(_np(r["prog_status"], np.int32), fx["exp_status"])
    np.testing.assert_array_equal(_np(r["call_len"], np.uint32), fx["exp_call_len"])
    np.testing.assert_array_equal(_np(r["call_errno"], np.int32), fx["exp_call_errno"])
    np.testing.assert_array_equal(_np(r["call_prio"], np.uint8), fx["exp_call_prio"])
    np.testing.assert_array_equal(_np(r["call_start"], np.uint64), fx["exp_call_start"])
    assert r["n_failed"] == int((fx["exp_status"] != 0).sum())
    regs, ncalls = regions_of(fx)
    exp_cov = []
    for reg, nc, pst in zip(regs, ncalls, fx["exp_status"]):
        _, info = O.read_out_coverage(reg, int(nc))
        exp_cov += [i[4] if (i is not None and pst == 0) else 0 for i in info]
    np.testing.assert_array_equal(_np(r["cover_len"], np.uint32), exp_cov)
    assert sum(exp_cov) == 1  # the well-formed region with comparisons carries one cover word


@pytest.mark.gpu
def test_ingest_without_call_num_and_empty(gpu):
    fx = load()
    _, r = _dev_ingest(gpu, fx["out"], fx["prog_off"], fx["prog_call"], fx["call_any"], None)
    exp = fx["exp_status"].copy()
    exp[exp == 4] = 0  # the callNum check is skipped without call_num
    np.testing.assert_array_equal(_np(r["prog_status"], np.int32), exp)
    _, r = _dev_ingest(gpu, np.empty(0, np.uint32), np.zeros(1, np.uint64), np.zeros(1, np.uint32),
                       np.empty(0, np.uint8), None)
    assert r["n_failed"] == 0


@pytest.mark.gpu
def test_ingest_rejects_out_of_bounds_offsets(gpu):
    from syzkaller_amd._lib import SyzsigError

    with pytest.raises(SyzsigError):
        _dev_ingest(gpu, np.zeros(4, np.uint32), np.array([0, 9], np.uint64), np.array([0, 1], np.uint32),
                    np.zeros(1, np.uint8), None)


@pytest.mark.gpu
@pytest.mark.parametrize("order_seed", [None, 7])
def test_ingest_then_triage_vs_oracle(gpu, order_seed):
    """64 programs x 32 calls: oracle executor -> executor regions (records in
    call or shuffled completion order) -> device ingest -> batch checkNewSignal,
    against the oracle's checkNewSignal on the same calls."""
    from syzkaller_amd import signal as S
    from syzkaller_amd import synth

    cfg = synth.synth_default(bad_pc_ppm=50)
    nprog, cpp = 64, 32
    cl = synth.call_lengths(nprog, cpp, 0, ragged=(0, 3000), seed=9)
    pcs, cs, prio = synth.traces(cfg, 0, nprog, cpp, cl)
    prog_call = synth.prog_call_index(nprog, cpp)
    sigs, cnt, comp = O.exec_batch(pcs, cs, cl, prog_call)
    rng = np.random.default_rng(1)
    errno = np.where(((prio >> 1) & 1) == 0, rng.integers(1, 40, prio.size), 0).astype(np.int32)
    call_any = ((prio & 1) == 0).astype(np.uint8)
    out, po = synth.frame_exec_output(sigs, cs, cnt, comp, prog_call, errno, order_seed=order_seed)
    dout, r = _dev_ingest(gpu, out, po, prog_call, call_any, np.tile(np.arange(cpp, dtype=np.uint32), nprog))
    assert r["n_failed"] == 0
    # un-published calls (after an abort) have errno -1 -> prio loses the errno bit, like signalPrio on Errno=-1
    exec_ = np.zeros(prio.size, bool)
    for p in range(nprog):
        exec_[prog_call[p]:prog_call[p] + comp[p]] = True
    hprio = np.where(exec_, prio, prio & 1).astype(np.uint8)
    np.testing.assert_array_equal(_np(r["call_prio"], np.uint8), hprio)
    np.testing.assert_array_equal(_np(r["call_len"], np.uint32), np.where(exec_, cnt, 0))
    m0 = synth.m0(cfg, 2048, 200000)
    ms = S.Serial(*m0).Deserialize(gpu.eng)
    ns = S.Signal(None, gpu.eng)
    pairs = torch.full((int(cnt.sum()) + 1,), -1, dtype=torch.int64, device=gpu.dev)
    _, cnew, st = gpu.triage(ms, ns, dout, r["call_start"], r["call_len"], r["call_prio"], new_pairs=pairs)
    oms, ons, obits, ocnew = O.triage_batch(m0[0], m0[1], sigs, cs, cnt, hprio)
    np.testing.assert_array_equal(_np(cnew, np.uint8), ocnew)
    r_ = np.nonzero(np.unpackbits(obits.view(np.uint8), bitorder="little"))[0].astype(np.uint64)
    call = np.searchsorted(cs.astype(np.uint64) + cnt.astype(np.uint64), r_, side="right").astype(np.uint64)
    op = np.unique((call << np.uint64(32)) | sigs[r_].astype(np.uint64))
    assert st["new_pairs"] == op.size
    np.testing.assert_array_equal(np.sort(_np(pairs[:op.size], np.uint64)), op)
    assert ms.to_dict() == oms.to_dict()
    assert ns.to_dict() == ons.to_dict()


def test_bench_frame_regions_parse_back():
    """bench.py's device-side framer (torch ops, run here on CPU) writes regions
    that the readOutCoverage restatement parses back to the batch."""
    import bench
    from syzkaller_amd import synth

    cfg = synth.synth_default(bad_pc_ppm=100)
    P, C = 12, 6
    cl = synth.call_lengths(P, C, 0, ragged=(0, 900), seed=4)
    pcs, cs, prio = synth.traces(cfg, 40, P, C, cl)
    pc = synth.prog_call_index(P, C)
    sigs, cnt, comp = O.exec_batch(pcs, cs, cl, pc)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt))  # noqa: E731
    out, poff, _, done = bench.frame_regions(t(sigs, np.int32), t(cs, np.int64), t(cnt, np.int32),
                                             t(prio, np.uint8), t(comp, np.int32), P, C)
    out, poff, done = out.numpy().view(np.uint32), poff.numpy(), done.numpy()
    assert done.sum() == comp.sum()
    for p in range(P):
        st, info = O.read_out_coverage(out[poff[p]:poff[p + 1]], C, list(range(C)))
        assert st == 0
        for i in range(C):
            c = p * C + i
            if i >= comp[p]:
                assert info[i] is None
                continue
            err, so, sl, _, _ = info[i]
            assert err == (0 if (prio[c] >> 1) & 1 else 22) and sl == cnt[c]
            reg = out[poff[p]:poff[p + 1]]
            np.testing.assert_array_equal(reg[so:so + sl], sigs[cs[c]:cs[c] + cnt[c]])


# ---- regions written by hand (tests/ingest_cases.py) ----
SETS = {"boundaries": IC.boundaries, "long": IC.long_programs, "batch": IC.batch}


@functools.lru_cache(maxsize=None)
def expected(which, with_call_num=True):
    """The restatement's result for a set of hand regions, computed once: the
    inputs and every output array of the kernel, the cover ranges included."""
    regions = SETS[which]()
    regs, ncalls, call_any, nums = IC.arrays(regions, with_call_num)
    out, po, pc, cs, cl, cp, ce, st = O.ingest_batch(regs, ncalls, call_any, nums)
    cov_s, cov_l = cs.copy(), np.zeros(cl.size, np.uint32)
    for p, reg in enumerate(regs):
        c0 = int(pc[p])
        cov_s[c0:int(pc[p + 1])] = po[p]
        if st[p] != 0:
            continue
        _, info = O.read_out_coverage(reg, int(ncalls[p]), None if nums is None else nums[c0:int(pc[p + 1])])
        for i, inf in enumerate(info):
            if inf is not None:
                cov_s[c0 + i], cov_l[c0 + i] = int(po[p]) + inf[3], inf[4]
    r = dict(out=out, prog_off=po, prog_call=pc, call_any=call_any, call_num=nums, call_start=cs, call_len=cl,
             call_prio=cp, call_errno=ce, prog_status=st, cover_start=cov_s, cover_len=cov_l)
    for v in r.values():
        if v is not None:
            v.setflags(write=False)
    return r


@pytest.mark.parametrize("which", ["boundaries", "long"])
def test_hand_status_is_the_restatements(which):
    for r in SETS[which]():
        words = np.array(r.words, np.uint32)
        st, info = O.read_out_coverage(words, r.ncalls, IC.call_nums(r.ncalls))
        assert st == r.status, r.name
        assert O.read_out_coverage(words, r.ncalls)[0] == r.status_nonum, r.name
        assert len(info) == r.ncalls


def test_hand_regions_reach_what_they_are_for():
    by = {r.name: r for r in IC.boundaries() + IC.long_programs()}
    assert len(by) == len(IC.boundaries()) + len(IC.long_programs())
    assert {r.status for r in IC.boundaries()} == set(range(10))  # every ipc.go branch, and success
    # the accepted region and its rejected neighbour differ by one word or by one in one size field
    for ok, bad in [("hdr7", "hdr6"), ("nsig_exact", "nsig_plus1"), ("ncover_exact", "ncover_plus1"),
                    ("comp_type7", "comp_type8"), ("comp8_4left", "comp8_3left"), ("comp4_2left", "comp4_1left"),
                    ("idx_last", "idx_ncalls")]:
        a, b = by[ok], by[bad]
        assert a.status == 0 != b.status and a.ncalls == b.ncalls
        if len(a.words) == len(b.words):
            d = [(x, y) for x, y in zip(a.words, b.words) if x != y]
            assert len(d) == 1 and d[0][1] == d[0][0] + 1, (ok, bad)
        else:
            assert len(a.words) == len(b.words) + 1 and a.words[:len(b.words)] == b.words, (ok, bad)
    # long programs: 256 calls fit the LDS bitmap exactly, 257 and 300 pass it
    assert {r.ncalls for r in IC.long_programs()} == {IC.SEEN_CALLS, IC.SEEN_CALLS + 1, 300}
    for nc in (256, 257, 300):
        st, info = O.read_out_coverage(by[f"long{nc}"].words, nc, IC.call_nums(nc))
        have = [i is not None for i in info]
        assert st == 0 and have[255] and have[nc - 1] and not have[254] and not have[3]
        assert by[f"long{nc}"].words[0] == sum(have)  # ncmd: one record per call that has one
    st, info = O.read_out_coverage(by["long300"].words, 300, IC.call_nums(300))
    assert info[256] is not None and info[258] is None and info[270] is None and info[257] is not None
    # the late failures come after records for calls of 256 and up were accepted
    for name in ("long300_fails_late", "long300_fails_short", "long257_fails_signal", "long300_double256",
                 "long257_double256_empty"):
        st, info = O.read_out_coverage(by[name].words, by[name].ncalls, IC.call_nums(by[name].ncalls))
        assert st != 0 and any(i is not None for i in info[IC.SEEN_CALLS:]), name
    # the batch: three workgroups, long programs and every status in each, neighbours of unlike outcome
    b = IC.batch()
    assert len(b) == IC.NPROG == 600 and -(-len(b) // IC.THREADS) == 3
    assert sum(r.ncalls == 2 for r in b) > len(b) * 3 // 4
    for g in range(3):
        grp = b[g * IC.THREADS:(g + 1) * IC.THREADS]
        assert any(r.ncalls > IC.SEEN_CALLS and r.status == 0 for r in grp)
        assert any(r.ncalls > IC.SEEN_CALLS and r.status != 0 for r in grp)
        assert g == 2 or any(r.ncalls > IC.SEEN_CALLS for r in grp[64:])  # past the first wave of a full group
    assert {r.name for r in b} >= set(by)
    short = [r for r in b if r.name.startswith("short")]
    assert all((r.status == 0) == (int(r.name[5:]) % 2 == 0) for r in short)
    for which in SETS:
        e = expected(which)
        np.testing.assert_array_equal(e["prog_status"], [r.status for r in SETS[which]()])
        np.testing.assert_array_equal(expected(which, False)["prog_status"], [r.status_nonum for r in SETS[which]()])
        assert not (e["call_len"] == IC.NIL_LEN).any()
        failed = np.repeat(e["prog_status"] != 0, np.diff(e["prog_call"].astype(np.int64)))
        assert (e["call_len"][failed] == 0).all() and (e["call_errno"][failed] == -1).all()
        assert 0 < (e["call_len"] > 0).sum() and 0 < (e["cover_len"] > 0).sum()


FILL = 0xAA


def raw_ingest(gpu, e, want_cover):
    """syzsig_ingest_exec_output_dev on call outputs pre-filled with 0xAA"""
    t = lambda a, dt: torch.from_numpy(a.view(dt).copy()).to(gpu.dev)  # noqa: E731
    from syzkaller_amd.device import _p

    ncalls, nprog = e["call_any"].size, e["prog_status"].size
    fill = lambda n, dt: torch.full((n * np.dtype(dt).itemsize,), FILL, dtype=torch.uint8, device=gpu.dev)  # noqa: E731
    o = {"call_start": fill(ncalls, np.uint64), "call_len": fill(ncalls, np.uint32),
         "call_prio": fill(ncalls, np.uint8), "call_errno": fill(ncalls, np.int32),
         "prog_status": fill(nprog, np.int32)}
    if want_cover:
        o["cover_start"], o["cover_len"] = fill(ncalls, np.uint64), fill(ncalls, np.uint32)
    out, po, pc = t(e["out"], np.int32), t(e["prog_off"], np.int64), t(e["prog_call"], np.int32)
    any_, num = t(e["call_any"], np.uint8), None if e["call_num"] is None else t(e["call_num"], np.int32)
    nf = ctypes.c_uint64()
    rc = gpu.L.syzsig_ingest_exec_output_dev(
        gpu.eng.h, _p(out), out.numel(), _p(po), nprog, _p(pc), ncalls, _p(num), _p(any_), _p(o["call_start"]),
        _p(o["call_len"]), _p(o["call_prio"]), _p(o["call_errno"]), _p(o.get("cover_start")),
        _p(o.get("cover_len")), _p(o["prog_status"]), ctypes.byref(nf))
    assert rc == 0
    dts = dict(call_start=np.uint64, call_len=np.uint32, call_prio=np.uint8, call_errno=np.int32,
               prog_status=np.int32, cover_start=np.uint64, cover_len=np.uint32)
    return {k: v.cpu().numpy().view(dts[k]) for k, v in o.items()}, int(nf.value)


def check_ingest(gpu, which, want_cover, with_call_num=True):
    e = expected(which, with_call_num)
    got, n_failed = raw_ingest(gpu, e, want_cover)
    assert not (got["call_len"] == IC.NIL_LEN).any()  # no "Signal == nil" sentinel left behind
    assert set(got) == {"call_start", "call_len", "call_prio", "call_errno", "prog_status"} | (
        {"cover_start", "cover_len"} if want_cover else set())
    for k, v in got.items():
        np.testing.assert_array_equal(v, e[k], err_msg=k)
    assert n_failed == int((e["prog_status"] != 0).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("want_cover", [False, True])
@pytest.mark.parametrize("which", ["boundaries", "long", "batch"])
def test_ingest_hand_regions(gpu, which, want_cover):
    check_ingest(gpu, which, want_cover)


@pytest.mark.gpu
def test_ingest_hand_regions_without_call_num(gpu):
    check_ingest(gpu, "batch", True, with_call_num=False)
    e = expected("batch", False)
    assert (e["prog_status"] != expected("batch")["prog_status"]).any()  # the callNum region now passes
    # and through the wrapper, which allocates the outputs itself
    _, r = _dev_ingest(gpu, e["out"].copy(), e["prog_off"].copy(), e["prog_call"].copy(), e["call_any"].copy(), None,
                       want_cover=True)
    for k, dt in dict(call_start=np.uint64, call_len=np.uint32, call_prio=np.uint8, call_errno=np.int32,
                      prog_status=np.int32, cover_start=np.uint64, cover_len=np.uint32).items():
        np.testing.assert_array_equal(_np(r[k], dt), e[k], err_msg=k)
    assert r["n_failed"] == int((e["prog_status"] != 0).sum())
