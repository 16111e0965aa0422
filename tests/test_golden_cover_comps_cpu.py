"""CPU: the cover and comps restatements (tests/cover_ref.py, tests/comps_ref.py)
and the region parse (oracle.read_out_coverage / ingest_batch, comps_ref.
parse_comps) held word for word to what the REFERENCE executor wrote: the
fixtures under tests/golden/cover and tests/golden/comps come from
oracle/_ref/ref_harness, which #includes the reference's executor_linux.cc and
runs handle_completion with flag_collect_cover / flag_collect_comps on."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from syzkaller_amd import _lib, synth
from tests import comps_ref as R
from tests import cover_ref as CR
from tests import golden_sets as GS

TC, TM = _lib.SYZSIG_COVER_TILE, _lib.SYZSIG_COMPS_TILE
KM0, KM1 = 0xffff880000000000, 0xffff890000000000
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- cover

@pytest.mark.parametrize("name", GS.COVER_NAMES)
def test_cover_restatement_matches_reference_fixtures(name):
    fx = GS.load_cover(name)
    dedup = bool(fx["dedup"])
    # which calls have a record at all: the oracle's signal loop (pinned by the signal goldens) agrees
    _, _, comp = O.exec_batch(fx["pcs"], fx["call_start"], fx["call_len"], fx["prog_call"])
    np.testing.assert_array_equal(comp, fx["exp_completed"])
    cover, cnt = CR.edge_cover(fx["pcs"], fx["call_start"], fx["call_len"], fx["prog_call"], fx["exp_completed"], dedup)
    np.testing.assert_array_equal(cnt, fx["exp_cover_cnt"])
    np.testing.assert_array_equal(cover, fx["exp_cover"])  # zeros outside the lists on both sides
    for c in np.flatnonzero(fx["exp_cover_cnt"]):
        s, n = int(fx["call_start"][c]), int(fx["call_len"][c])
        np.testing.assert_array_equal(CR.call_cover(fx["pcs"][s:s + n], dedup),
                                      fx["exp_cover"][s:s + int(fx["exp_cover_cnt"][c])], err_msg=f"call {c}")


@pytest.mark.parametrize("name", ["abort_dedup0", "abort_dedup1"])
def test_reference_written_cover_regions_parse(name):
    """readOutCoverage over the regions the executor wrote with cover lists:
    inf.Signal and inf.Cover are the reference's words, calls without a record
    have none."""
    fx = GS.load_cover(name)
    sigs, sig_cnt, _ = O.exec_batch(fx["pcs"], fx["call_start"], fx["call_len"], fx["prog_call"])
    for p in range(fx["prog_call"].size - 1):
        reg = fx["regions"][int(fx["region_off"][p]):int(fx["region_off"][p + 1])]
        c0, c1 = int(fx["prog_call"][p]), int(fx["prog_call"][p + 1])
        st, info = O.read_out_coverage(reg, c1 - c0, list(range(c1 - c0)))
        assert st == O.INGEST_OK
        assert [i is not None for i in info] == [k < fx["exp_completed"][p] for k in range(c1 - c0)]
        for k, inf in enumerate(info):
            if inf is None:
                continue
            c, s = c0 + k, int(fx["call_start"][c0 + k])
            err, so, sl, co, cl = inf
            assert err == (22 if fx["call_failed"][c] else 0)
            np.testing.assert_array_equal(reg[so:so + sl], sigs[s:s + int(sig_cnt[c])])
            np.testing.assert_array_equal(reg[co:co + cl], fx["exp_cover"][s:s + int(fx["exp_cover_cnt"][c])])
        assert co + cl == reg.size if fx["exp_completed"][p] else reg.size == 1


def test_cover_fixtures_hold_the_corner_cases():
    for s in GS.COVER_SETS:  # both dedup values over the same traces
        a, b = GS.load_cover(s + "_dedup0"), GS.load_cover(s + "_dedup1")
        assert int(a["dedup"]) == 0 and int(b["dedup"]) == 1
        for k in GS.TRACE_KEYS:
            np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a["exp_completed"], b["exp_completed"])
        done = np.concatenate([np.arange(n) < k for n, k in zip(np.diff(a["prog_call"]), a["exp_completed"])])
        np.testing.assert_array_equal(a["exp_cover_cnt"], np.where(done, a["call_len"], 0))  # no dedup: every PC
        assert (b["exp_cover_cnt"] <= a["exp_cover_cnt"]).all()
    fx = GS.load_cover("lengths_dedup1")
    lens, cnt = fx["call_len"].tolist(), fx["exp_cover_cnt"].tolist()
    assert set(lens) == {0, 1, 2, TC - 1, TC, TC + 1, 2 * TC + 3}
    calls = [fx["pcs"][int(s):int(s) + n] for s, n in zip(fx["call_start"], lens)]
    long_ = [(p, k) for p, k in zip(calls, cnt) if p.size > TC]
    assert any(k == 1 for _, k in long_)                                          # all PCs equal
    assert any((np.diff(p.astype(np.int64)) > 0).all() for p, _ in long_)         # already sorted
    assert any((np.diff(p.astype(np.int64)) < 0).all() for p, _ in long_)         # reverse-sorted
    assert any(1 < k < p.size for p, k in long_)                                  # duplicates among distinct PCs
    assert any(k > TC for _, k in long_)                                          # survivors past one tile
    for bound in (0xffffffff80000000, 0xfffffffffeffffff):                        # both bounds of cover_check
        assert (fx["pcs"] == np.uint64(bound)).any()
    assert (fx["exp_cover"] == 0x80000000).any() and (fx["exp_cover"] == 0xfeffffff).any()
    assert fx["call_failed"].any() and (fx["exp_cover_cnt"][fx["call_failed"] == 1] > 0).any()
    ab = GS.load_cover("abort_dedup1")
    ncalls = np.diff(ab["prog_call"])
    assert (ab["exp_completed"] < ncalls).any() and (ab["exp_completed"] == ncalls).any()
    assert (ab["exp_completed"] == 0).any() and ((ab["exp_completed"] > 0) & (ab["exp_completed"] < ncalls)).any()
    for p in np.flatnonzero(ab["exp_completed"] < ncalls):  # the aborting call and the later ones: no record
        c0 = int(ab["prog_call"][p])
        assert not ab["exp_cover_cnt"][c0 + int(ab["exp_completed"][p]):c0 + int(ncalls[p])].any()
        assert ab["call_len"][c0 + int(ab["exp_completed"][p])] > 0
    for v in (0xffffffff7fffffff, 0xffffffffff000000):  # one outside either bound
        assert (ab["pcs"] == np.uint64(v)).any()
    assert GS.load_cover("big_dedup0")["call_len"].tolist() == [262143]
    assert GS.load_cover("big_dedup1")["exp_cover_cnt"][0] > TC


# ---------------------------------------------------------------- comps

def _completed_calls(fx):
    return [c for p in range(fx["prog_call"].size - 1)
            for c in range(int(fx["prog_call"][p]), int(fx["prog_call"][p]) + int(fx["exp_completed"][p]))]


def _call_recs(fx, c):
    s, n = int(fx["call_start"][c]), int(fx["call_len"][c])
    return fx["comps"][s:s + n]


def _bad_type(fx, c):
    """the call has a record whose low type word is above 7 (ipc.go:429-433 rejects it)"""
    return bool(((_call_recs(fx, c)[:, 0] & np.uint64(0xffffffff)) > 7).any())


@pytest.mark.parametrize("name", GS.COMPS_NAMES)
def test_comps_restatement_matches_reference_fixtures(name):
    fx = GS.load_comps(name)
    out_start = int(fx["out_start"])
    done = _completed_calls(fx)
    for c in done:
        w, k = R.call_comps(_call_recs(fx, c).tolist(), out_start)
        s = 5 * int(fx["call_start"][c])
        assert (len(w), k) == (int(fx["exp_out_words"][c]), int(fx["exp_comps_cnt"][c])), c
        np.testing.assert_array_equal(np.array(w, np.uint64), fx["exp_words"][s:s + len(w)], err_msg=f"call {c}")
    # ... and the batch layout, over the calls the reference completed
    sel = np.array(done, np.int64)
    out, nw, cnt = R.exec_comps(fx["comps"], fx["call_start"][sel], fx["call_len"][sel], out_start)
    np.testing.assert_array_equal(nw, fx["exp_out_words"][sel])
    np.testing.assert_array_equal(cnt, fx["exp_comps_cnt"][sel])
    np.testing.assert_array_equal(out, fx["exp_words"])  # zeros for the calls without a record on both sides


def test_max_comps_is_where_the_reference_fails():
    fx = GS.load_comps("toomany")
    assert fx["exp_status"].tolist() == [GS.K_FAIL_STATUS, 0]
    lens, c0 = fx["call_len"], int(fx["prog_call"][0])
    bad = c0 + int(fx["exp_completed"][0])  # the call the child failed in
    assert int(lens[bad]) == R.MAX_COMPS + 1 == 65536
    with pytest.raises(ValueError):
        R.call_comps(_call_recs(fx, bad).tolist(), int(fx["out_start"]))
    assert fx["exp_completed"][0] == 1 and bad + 1 < int(fx["prog_call"][1])  # the call before it kept its record
    ok = int(fx["prog_call"][1])
    assert int(lens[ok]) == R.MAX_COMPS and fx["exp_completed"][1] == 1 and fx["exp_comps_cnt"][ok] > 0


@pytest.mark.parametrize("name", GS.COMPS_NAMES)
def test_reference_written_comps_regions_parse(name):
    """The regions as the executor wrote them through readOutCoverage (the
    framing hints.CompMap.from_regions depends on) and parse_comps."""
    fx = GS.load_comps(name)
    nprog = fx["prog_call"].size - 1
    ncalls = np.diff(fx["prog_call"]).tolist()
    regions = [fx["regions"][int(fx["region_off"][p]):int(fx["region_off"][p + 1])] for p in range(nprog)]
    frames = [GS.comps_region_calls(fx, p) for p in range(nprog)]
    exp_st = []
    for p in range(nprog):
        a = int(fx["region_off"][p])
        bad = [c for c, _, _ in frames[p] if _bad_type(fx, c)]
        exp_st.append(O.INGEST_ECOMPTYPE if bad else O.INGEST_OK)
        st, info = O.read_out_coverage(regions[p], ncalls[p], list(range(ncalls[p])))
        assert st == exp_st[-1], p
        for c, ws, we in frames[p]:
            np.testing.assert_array_equal(fx["regions"][ws:we], fx["exp_words"][5 * int(fx["call_start"][c]):][:we - ws])
            n = int(fx["exp_comps_cnt"][c])
            st, m = R.parse_comps(fx["regions"], ws, n, we)
            assert st == (R.INGEST_ECOMPTYPE if c in bad else R.INGEST_OK), c
            if c in bad:
                continue
            # exactly comps_cnt records in exactly out_words words: one word less no longer parses
            if n:
                assert R.parse_comps(fx["regions"], ws, n, we - 1)[0] == R.INGEST_ECOMPS
            if exp_st[-1] == O.INGEST_OK:  # readOutCoverage walked to the same place
                i = c - int(fx["prog_call"][p])
                err, so, sl, co, cl = info[i]
                assert (sl, cl, a + co + cl) == (0, 0, ws) and int(regions[p][so - 1]) == n
                assert err == (22 if fx["call_failed"][c] else 0)
        if exp_st[-1] == O.INGEST_OK:  # calls without a record: Errno = -1
            assert [i is not None for i in info] == [k < len(frames[p]) for k in range(ncalls[p])]
    r = O.ingest_batch(regions, ncalls, np.zeros(sum(ncalls), np.uint8),
                       np.concatenate([np.arange(n) for n in ncalls]).astype(np.uint32))
    np.testing.assert_array_equal(r[7], exp_st)
    if name == "edges":
        assert exp_st == [O.INGEST_OK, O.INGEST_ECOMPTYPE]


def test_comps_fixtures_hold_the_corner_cases():
    seg, lng, edges = GS.load_comps("segments"), GS.load_comps("long"), GS.load_comps("edges")
    out_start = int(edges["out_start"])
    out_end = out_start + R.K_MAX_OUTPUT
    for fx in (seg, lng, edges, GS.load_comps("toomany")):
        assert int(fx["out_start"]) == out_start
    assert set(seg["call_len"].tolist()) == {0, 1, 2, TM - 1, TM, TM + 1, 2 * TM + 3}
    assert (seg["exp_comps_cnt"] > TM).any()                      # survivors past one tile
    assert set(np.unique(seg["comps"][:, 0]).tolist()) == set(range(8))
    assert lng["call_len"].tolist() == [65535] and lng["exp_comps_cnt"][0] > TM
    rec = {tuple(r) for r in edges["comps"][:, :3].tolist()}
    types = {t for t, _, _ in rec}

    def written(t, a1, a2):
        """the words the fixture holds for this record, if it was written"""
        assert (t, a1, a2) in rec, (hex(t), hex(a1), hex(a2))
        for c in _completed_calls(edges):
            if (t, a1, a2) in {tuple(r) for r in _call_recs(edges, c)[:, :3].tolist()}:
                s = 5 * int(edges["call_start"][c])
                w = edges["exp_words"][s:s + int(edges["exp_out_words"][c])].tolist()
                want = R.write_comp(t, a1, a2)
                return sum(w[i:i + len(want)] == want for i in range(len(w)))
        raise AssertionError("record in no completed call")

    # a segment of one record repeated; a segment where every record is ignored, both past one tile
    c_len, c_cnt = edges["call_len"].tolist(), edges["exp_comps_cnt"].tolist()
    assert any(n > TM and k == 1 and len({tuple(r) for r in _call_recs(edges, c)[:, :3].tolist()}) == 1
               for c, (n, k) in enumerate(zip(c_len, c_cnt)))
    assert any(n > TM and k == 0 for n, k in zip(c_len, c_cnt))
    # records equal except for pc
    c2 = _call_recs(edges, 2)
    assert len({tuple(r) for r in c2[:, :3].tolist()}) < len({tuple(r) for r in c2.tolist()})
    assert set(range(8)) <= types
    # type with bits above bit 31 next to the same low word: two records, identical words
    assert {(0x100000002, 5, 6), (2, 5, 6)} <= rec and written(2, 5, 6) == 2
    assert any(t >> 63 for t in types)
    # type's low word above 7, every such call of a program of its own
    p1 = range(int(edges["prog_call"][1]), int(edges["prog_call"][2]))
    assert all(_bad_type(edges, c) for c in p1) and not any(_bad_type(edges, c) for c in range(p1[0]))
    assert edges["exp_completed"][1] == len(p1)
    assert {8, 0x10, 0xf, 0xffffffff, 0x100000009} <= types
    assert written(0xf, 0x1122334455667788, 2) == 1 and written(8, 1, 2) == 1
    # operands with bit 63 set; operands that differ only in their high 32 bits
    assert written(6, 0x8000000000000001, 5) == 1 and written(6, 0x0000000100000001, 5) == 1
    assert written(6, 1, 5) == 1 and written(6, 5, 0x8000000000000001) == 1
    assert written(4, 1, 5) == 3  # SIZE4: 0x8000000000000001, 0x100000001 and 1 leave as the same words
    # the sign boundaries of sizes 1, 2, 4
    for size in (0, 2, 4):
        for v in (0x7f, 0x80, 0xff, 0x7fff, 0x8000, 0x7fffffff, 0x80000000):
            assert written(size, v, 1) >= 1 and written(size | 1, 1, v) >= 1
    assert R.write_comp(0, 0x80, 1) == [0, 0xffffff80, 1] and R.write_comp(2, 0x8000, 1) == [2, 0xffff8000, 1]
    # pairs that differ only above the operand size
    for size, hi in ((0, 0x100), (2, 0x10000), (4, 0x100000000)):
        assert {(size, 0xfe, 1), (size, 0xfe | hi, 1)} <= rec and written(size, 0xfe, 1) >= 2
    # every boundary of ignore() at -1, 0, +1
    bounds = [out_start, out_end, KM0, KM1]
    for b in bounds:
        for v in ((b - 1) & M64, b, (b + 1) & M64):
            for t in (6, 7, 0, 2, 4):
                assert {(t, v, 1), (t, 1, v), (t, v, 0), (t, 0, v)} <= rec
    for v in (KM0 - 1, KM0, KM0 + 1, KM1 - 1, KM1, KM1 + 1):
        for w in (KM0 - 1, KM0, KM0 + 1, KM1 - 1, KM1, KM1 + 1):
            assert (6, v, w) in rec
    assert written(6, out_start - 1, 1) == 1 and written(6, out_start, 1) == 0
    assert written(6, out_end, 1) == 0 and written(6, out_end + 1, 1) == 1
    assert written(6, 1, out_start - 1) == 1 and written(6, 1, out_end) == 0 and written(6, 1, out_end + 1) == 1
    assert written(6, KM0, KM1) == 0 and written(6, KM0 - 1, KM1) == 1 and written(6, KM0, KM1 + 1) == 1
    assert written(6, KM0, 0) == 0 and written(6, KM0 - 1, 0) == 1 and written(6, KM1 + 1, 0) == 1
    assert written(6, 0, KM1) == 0 and written(6, 0, KM1 + 1) == 1 and written(6, 0, KM0 - 1) == 1
    assert written(6, KM0, 1) == 1                                 # one kernel pointer against a plain value
    assert written(4, out_start, 1) >= 1 and written(2, KM0, KM1) >= 1 and written(0, KM0, 0) >= 1  # not SIZE8
    # arg1 == 0 with and without CONST
    for t in range(8):
        assert {(t, 0, 0), (t, 0, 5), (t, 5, 0)} <= rec
    c6 = next(c for c in _completed_calls(edges) if (3, 0, 5) in {tuple(r) for r in _call_recs(edges, c)[:, :3].tolist()}
              and int(edges["call_len"][c]) == 24)
    s = 5 * int(edges["call_start"][c6])
    w6 = edges["exp_words"][s:s + int(edges["exp_out_words"][c6])].tolist()
    exp6 = []
    for t in range(8):  # the survivors in operator< order: (t, 0, 5) without CONST, then (t, 5, 0)
        if not t & 1:
            exp6 += R.write_comp(t, 0, 5)
        exp6 += R.write_comp(t, 5, 0)
    assert w6 == exp6


# ---------------------------------------------------------------- live

@pytest.mark.skipif(not os.path.exists(O.REF_HARNESS), reason="reference harness not built (no /root/reference)")
def test_restatements_match_live_reference_on_fresh_programs():
    # cover: fresh seeded traces, some aborted, both dedup values
    cfg = synth.synth_default(region_log2=10, bad_pc_ppm=80)
    nprog, cpp = 4, 5
    cl = synth.call_lengths(nprog, cpp, 0, ragged=(0, 6000), seed=123)
    pcs, cs, prio = synth.traces(cfg, 4321, nprog, cpp, cl)
    pidx = synth.prog_call_index(nprog, cpp)
    progs = [[(((prio[c] >> 1) & 1) == 0, pcs[cs[c]: cs[c] + cl[c]]) for c in range(pidx[p], pidx[p + 1])]
             for p in range(nprog)]
    _, _, comp = O.exec_batch(pcs, cs, cl, pidx)
    for dedup in (True, False):
        cover, cnt = CR.edge_cover(pcs, cs, cl, pidx, comp, dedup)
        ref = O.run_reference_executor(progs, mode="cover", dedup=dedup)
        seen = 0
        for p, (completed, calls) in enumerate(ref):
            assert completed == comp[p] == len(calls)
            for idx, _err, _sigs, cov in calls:
                c = pidx[p] + idx
                assert cov.size == cnt[c]
                np.testing.assert_array_equal(cover[cs[c]: cs[c] + cnt[c]], cov)
                seen += 1
        assert seen == int(comp.sum()) and 0 < seen < nprog * cpp  # some programs aborted, some calls kept
    # comps: fresh seeded records against the address the harness's region really has
    lens = [0, 3, 700, TM + 17, 1, 5000]
    _, inf = O.run_reference_executor([], mode="comps", info=True)
    for out_addr in (0, 0x1b2bc20000 + (77 << 20)):
        out_start = out_addr or inf["out_start"]
        comps, st = synth.comparisons(2024, lens, out_start, pool=20)
        progs = [[(False, comps[int(s): int(s) + n]) for s, n in zip(st[:3], lens[:3])],
                 [(True, comps[int(s): int(s) + n]) for s, n in zip(st[3:], lens[3:])]]
        ref, inf2 = O.run_reference_executor(progs, mode="comps", out_addr=out_addr, info=True)
        # out_addr = 0 maps anywhere, so the region may lie elsewhere than in the probing run: the reported
        # address is the one ignore() used
        out_start = inf2["out_start"]
        assert out_addr in (0, out_start)
        assert inf2["status"] == [0, 0]
        c = 0
        for completed, calls in ref:
            assert completed == len(calls) == 3
            for _idx, _err, words, k in calls:
                w, ek = R.call_comps(comps[int(st[c]): int(st[c]) + lens[c]].tolist(), out_start)
                assert k == ek and words.tolist() == w, c
                c += 1
