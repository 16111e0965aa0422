"""GPU: syzsig_file_set_dev (csrc/report.hip) against tests/fileset_ref.py,
exactly -- everything is integers.  The hand-derived cases of
tests/fileset_cases.py run on the device as they run on the restatement; the
sizes are the kernels' seams: the sort tile, the survivors' sweep of 256 keys,
the wave / workgroup threshold of the writer, a word of the funcs bitmap."""
import hashlib

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, report
from tests import fileset_cases as C
from tests import fileset_ref as R
from tests import report_ref as RR

pytestmark = pytest.mark.gpu

T = _lib.SYZSIG_FILESET_TILE
SWEEP = 256  # keys per sweep of the survivors' scan; also the longest list a wave writes


def _passes(maxlen):
    """rank-merge passes over a longest segment of maxlen keys: runs of T double until one holds it"""
    p, w = 0, T
    while w < maxlen:
        p, w = p + 1, 2 * w
    return p


def _expect_stats(cov, unc, want_kept):
    """(kept, long files, merge passes) from the frames: a file's segment is its
    covered frames plus its kept uncovered frames, repeats included."""
    seg = {}
    for f, _, _ in list(cov) + list(want_kept):
        seg[f] = seg.get(f, 0) + 1
    long_ = [n for n in seg.values() if n > T]
    return len(want_kept), len(long_), _passes(max(long_, default=0))


def _check(gpu, cov, unc, nlines=None, files=(), funcs=()):
    """The device's lists, shown and Coverage against the restatement; returns the stats."""
    fr = report.Frames(gpu, cov, unc, files, funcs)
    off, line, covered, shown, coverage = report.file_set(fr, nlines)
    want = R.file_set(cov, unc)
    off, line, covered = off.cpu().numpy(), line.cpu().numpy(), covered.cpu().numpy()
    assert off.size == fr.nfiles + 1 and off[0] == 0 and off[-1] == line.size == covered.size
    assert set(np.unique(covered).tolist()) <= {0, 1}
    got = {fr.files[f]: list(zip(line[off[f]:off[f + 1]].tolist(), covered[off[f]:off[f + 1]].astype(bool).tolist()))
           for f in np.flatnonzero(np.diff(off)).tolist()}
    assert got.keys() == want.keys()
    for f in want:
        assert got[f] == want[f], f
    assert sum(len(v) for v in want.values()) == off[-1]
    if nlines is None:
        assert shown is None and coverage is None
    else:
        shown, coverage = shown.cpu().numpy(), coverage.cpu().numpy()
        for i, f in enumerate(fr.files):
            assert (int(shown[i]), int(coverage[i])) == R.walk(nlines.get(f, 0), want.get(f, [])), f
    st = report.file_set_stats(gpu)
    funcs_cov = {fn for _, _, fn in cov}
    assert st[:3] == _expect_stats(cov, unc, [fr_ for fr_ in unc if fr_[2] in funcs_cov])
    assert st[3] == off[-1]
    return st


@pytest.mark.parametrize("case", C.FILE_SET, ids=[c[0] for c in C.FILE_SET])
def test_hand_cases(gpu, case):
    _, cov, unc, nlines, want, want_walk = case
    _check(gpu, cov, unc, nlines)
    fr = report.Frames(gpu, cov, unc)
    assert report.file_set_dict(fr) == want
    _, _, _, shown, coverage = report.file_set(fr, nlines)
    got = {f: (int(shown[i]), int(coverage[i])) for i, f in enumerate(fr.files) if f in want}
    assert got == want_walk


def _both_lists(rng, name, lines, func="f"):
    """A file's distinct `lines` fed from both lists: about half covered, the rest
    uncovered, a tenth in both, and repeats in each list."""
    lines = np.asarray(lines)
    is_cov = rng.random(lines.size) < 0.5
    both = rng.random(lines.size) < 0.1
    c = lines[is_cov].tolist()
    u = lines[~is_cov | both].tolist()
    c += rng.choice(c, size=len(c) // 20 + 1).tolist()
    u += rng.choice(u, size=len(u) // 20 + 1).tolist()
    return ([(name, int(x), func) for x in rng.permutation(c)], [(name, int(x), func) for x in rng.permutation(u)])


def test_tile_boundaries_and_stats(gpu):
    """Files of T - 1, T, T + 1 and 2T + 3 distinct lines from both lists with
    repeats, and two files without repeats whose segments are exactly T (the last
    one-workgroup sort) and T + 1 keys (two tiles, the second of one key)."""
    rng = np.random.default_rng(1)
    cov, unc, nlines = [], [], {}
    for name, d in (("a", T - 1), ("b", T), ("c", T + 1), ("d", 2 * T + 3)):
        lines = rng.choice(np.arange(-50, 3 * d), size=d, replace=False)
        c, u = _both_lists(rng, name, lines)
        cov, unc = cov + c, unc + u
        nlines[name] = 2 * d  # some lines past the end, and nothing shown where a line is below 1
    for name, n in (("e", T), ("g", T + 1)):
        lines = rng.permutation(np.arange(1, n + 1))
        cov += [(name, int(x), "f") for x in lines[: n // 2]]
        unc += [(name, int(x), "f") for x in lines[n // 2:]]
        nlines[name] = n - 7
    st = _check(gpu, cov, unc, nlines)
    seg_d = sum(f == "d" for f, _, _ in cov + unc)
    assert st[1] >= 2 and st[2] == _passes(seg_d) >= 2  # g and d at least; d needs two passes or more


def test_pair_straddles_tile_and_sweep(gpu):
    """Line T is covered and uncovered.  With lines 1 .. T covered and T .. T + 40
    uncovered, without repeats, its two keys are the sorted keys T - 1 and T: the
    last key of the first tile's run and of a sweep, the first of the next.  The
    same at the sweep boundary of a one-workgroup file, whose list of 256 entries
    is the longest a wave writes; its neighbour's 257 take the workgroup."""
    rng = np.random.default_rng(2)
    cov = [("big", int(x), "f") for x in rng.permutation(np.arange(1, T + 1))]
    unc = [("big", int(x), "f") for x in rng.permutation(np.arange(T, T + 41))]
    cov += [("small", int(x), "f") for x in rng.permutation(np.arange(1, SWEEP + 1))]
    unc += [("small", SWEEP, "f")]
    cov += [("next", int(x), "f") for x in rng.permutation(np.arange(1, SWEEP + 1))]
    unc += [("next", SWEEP, "f"), ("next", SWEEP + 1, "f")]
    st = _check(gpu, cov, unc, {"big": T, "small": SWEEP, "next": SWEEP + 1})
    assert st[:3] == (41 + 1 + 2, 1, 1)  # every uncovered frame is kept; `big` alone is long: T + 41 keys, one pass
    d = report.file_set_dict(report.Frames(gpu, cov, unc))
    assert d["big"][T - 1] == (T, True) and d["big"][T] == (T + 1, False) and len(d["big"]) == T + 40
    assert d["small"][-1] == (SWEEP, True) and len(d["small"]) == SWEEP
    assert d["next"][-2:] == [(SWEEP, True), (SWEEP + 1, False)] and len(d["next"]) == SWEEP + 1


def test_one_file_holds_every_frame(gpu):
    rng = np.random.default_rng(3)
    funcs = [f"fn{k}" for k in range(50)]
    cov = [("only.c", int(rng.integers(-5, 9000)), funcs[int(rng.integers(0, 30))]) for _ in range(7000)]
    unc = [("only.c", int(rng.integers(-5, 9000)), funcs[int(rng.integers(0, 50))]) for _ in range(5000)]
    st = _check(gpu, cov, unc, {"only.c": 8000})
    assert st[1] == 1 and st[2] == _passes(7000 + st[0])


def test_4000_files_mostly_empty(gpu):
    rng = np.random.default_rng(4)
    files = [f"dir/f{k}.c" for k in range(4000)]
    cov = [(files[int(rng.integers(0, 4000)) if k % 3 else 17], int(rng.integers(0, 60)), f"fn{k % 7}")
           for k in range(300)]
    unc = [(files[int(rng.integers(0, 4000))], int(rng.integers(0, 60)), f"fn{k % 11}") for k in range(300)]
    st = _check(gpu, cov, unc, {f: 40 for f in files}, files=files)
    assert st[1] == 0 and 0 < st[0] < 300
    d = report.file_set_dict(report.Frames(gpu, cov, unc, files=files))
    assert d == R.file_set(cov, unc) and len(d) < 600


def test_funcs_bitmap_words(gpu):
    """Function ids 0, 31, 32, 63, 64 and nfuncs - 1 covered, and several hundred
    covered frames whose functions all share the bitmap's second word; every
    function has an uncovered frame, kept only for the covered ones."""
    rng = np.random.default_rng(5)
    nfuncs = 131
    funcs = [f"fn{k}" for k in range(nfuncs)]
    edge = [0, 31, 32, 63, 64, nfuncs - 1]
    cov = [("e.c", 10 + k, funcs[k]) for k in edge]
    word = [33, 34, 40, 47, 62]
    cov += [("w.c", int(rng.integers(1, 200)), funcs[word[int(rng.integers(0, len(word)))]]) for _ in range(600)]
    unc = [("u.c", 1000 + k, funcs[k]) for k in range(nfuncs)] * 2
    st = _check(gpu, cov, unc, {"e.c": 500, "w.c": 100, "u.c": 2000}, funcs=funcs)
    assert st[0] == 2 * len(set(edge) | set(word))
    d = report.file_set_dict(report.Frames(gpu, cov, unc, funcs=funcs))
    assert [ln - 1000 for ln, _ in d["u.c"]] == sorted(set(edge) | set(word))


def test_one_function_and_interned_arrays(gpu):
    """nfuncs == 1, from arrays the caller interned (ids, not names)."""
    rng = np.random.default_rng(6)
    cf, cl = rng.integers(0, 5, size=700), rng.integers(-3, 90, size=700)
    uf, ul = rng.integers(0, 5, size=500), rng.integers(-3, 90, size=500)
    z = np.zeros(700, np.uint32)
    names = [f"f{k}" for k in range(5)]
    fr = report.Frames(gpu, (cf.astype(np.uint32), cl.astype(np.int32), z),
                       (torch.from_numpy(uf.astype(np.int32)), torch.from_numpy(ul.astype(np.int32)),
                        torch.zeros(500, dtype=torch.int32)), files=5, funcs=1)
    cov = [(names[f], int(ln), "fn") for f, ln in zip(cf, cl)]
    unc = [(names[f], int(ln), "fn") for f, ln in zip(uf, ul)]
    want = R.file_set(cov, unc)
    assert report.file_set_dict(fr) == {int(f[1:]): v for f, v in want.items()}
    assert report.file_set_stats(gpu)[0] == 500
    _check(gpu, cov, unc, {n: 50 for n in names}, files=names, funcs=["fn"])


def test_random_batch(gpu):
    """About 2 * 10^5 frames over 300 files and 2000 functions, neighbouring frames
    sharing file and function as frames of neighbouring PCs do; about a third of
    the uncovered frames belong to functions without a covered frame."""
    rng = np.random.default_rng(7)
    nfiles, nfuncs = 300, 2000
    files = [("./inc/h%d.h" if k % 5 == 0 else "src/f%d.c") % k for k in range(nfiles)]
    funcs = [f"fn{k}" for k in range(nfuncs)]
    func_file = (np.minimum(rng.zipf(1.2, nfuncs), nfiles) - 1).astype(np.int64)  # a few files own most functions
    covered_funcs = np.flatnonzero(rng.random(nfuncs) < 0.67)

    def frames(n, pool):
        runs = rng.integers(1, 12, size=n)
        fn = np.repeat(pool[rng.integers(0, pool.size, size=n)], runs)[:n]
        fl = func_file[fn].copy()
        inl = rng.random(n) < 0.1  # inlined into another file
        fl[inl] = rng.integers(0, nfiles, size=int(inl.sum()))
        ln = (fn * 37 % 5000 + rng.integers(0, 40, size=n)).astype(np.int64)
        ln[rng.random(n) < 0.001] = 0
        return fl, ln, fn

    cfl, cln, cfn = frames(110000, covered_funcs)
    ufl, uln, ufn = frames(90000, np.arange(nfuncs))
    cov = [(files[a], int(b), funcs[c]) for a, b, c in zip(cfl, cln, cfn)]
    unc = [(files[a], int(b), funcs[c]) for a, b, c in zip(ufl, uln, ufn)]
    nlines = {f: 2500 + 10 * k for k, f in enumerate(files)}
    st = _check(gpu, cov, unc, nlines, files=files, funcs=funcs)
    have = set(cfn.tolist())
    kept = sum(int(f) in have for f in ufn.tolist())
    assert st[0] == kept and 0.55 < kept / 90000 < 0.8
    assert st[1] >= 1  # the zipf's first files hold tens of thousands of frames


def test_lists_only(gpu):
    """d_nlines == NULL: the lists, no walk."""
    by = {c[0]: c for c in C.FILE_SET}
    _, cov, unc, _, want, _ = by["uncovered_creates_file"]
    fr = report.Frames(gpu, cov, unc)
    off, line, covered, shown, coverage = report.file_set(fr)
    assert shown is None and coverage is None
    assert off.tolist() == [0, 1, 3] and line.tolist() == [10, 30, 31] and covered.tolist() == [1, 0, 0]
    _check(gpu, cov, unc)
    off, line, covered, shown, coverage = report.file_set(report.Frames(gpu, [], []), {})
    assert off.tolist() == [0] and line.numel() == 0 and shown.numel() == 0 and coverage.numel() == 0


def test_errors_leave_outputs(gpu):
    _, cov, unc, nlines, want, _ = {c[0]: c for c in C.FILE_SET}["covered_wins"]
    cov, unc = cov + [("b.c", 1, "g")], unc + [("b.c", 2, "g")]
    fr = report.Frames(gpu, cov, unc)
    nf, nfn, need = fr.nfiles, fr.nfuncs, 4  # a.c: 7, 9; b.c: 1, 2
    sentinel = 0x5A

    def run(cov_t, unc_t, nfiles, nfuncs, cap, walk=(True, True, True)):
        outs = [torch.full((nf + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=gpu.dev),
                torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=gpu.dev),
                torch.full((8,), sentinel, dtype=torch.uint8, device=gpu.dev),
                torch.full((nf,), 0x5A5A5A5A, dtype=torch.int32, device=gpu.dev),
                torch.full((nf,), 0x5A5A5A5A, dtype=torch.int32, device=gpu.dev)]
        before = [o.clone() for o in outs]
        nl = torch.full((nf,), 20, dtype=torch.int32, device=gpu.dev)
        gpu.sync_stream()
        rc = gpu.L.syzsig_file_set_dev(gpu.eng.h, cov_t[0].data_ptr(), cov_t[1].data_ptr(), cov_t[2].data_ptr(),
                                       cov_t[0].numel(), unc_t[0].data_ptr(), unc_t[1].data_ptr(), unc_t[2].data_ptr(),
                                       unc_t[0].numel(), nfiles, nfuncs, nl.data_ptr() if walk[0] else None,
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), cap,
                                       outs[3].data_ptr() if walk[1] else None, outs[4].data_ptr() if walk[2] else None)
        torch.cuda.synchronize()
        return rc, all(bool((o == b).all()) for o, b in zip(outs, before))

    assert run(fr.cov, fr.unc, nf, nfn, need) == (_lib.SYZSIG_OK, False)
    assert run(fr.cov, fr.unc, nf, nfn, need - 1) == (_lib.SYZSIG_ERANGE, True)  # cap one below the need
    assert run(fr.cov, fr.unc, nf, nfn, 0) == (_lib.SYZSIG_ERANGE, True)
    for which in (0, 2):  # a file id at nfiles, a function id at nfuncs, in either list
        for lst in ("cov", "unc"):
            t = [x.clone() for x in getattr(fr, lst)]
            t[which][1] = nf if which == 0 else nfn
            args = (t, fr.unc) if lst == "cov" else (fr.cov, t)
            assert run(*args, nf, nfn, need) == (_lib.SYZSIG_EINVAL, True)
    assert run(fr.cov, fr.unc, nf - 1, nfn, need) == (_lib.SYZSIG_EINVAL, True)  # b.c's id is now nfiles
    assert run(fr.cov, fr.unc, nf, nfn - 1, need) == (_lib.SYZSIG_EINVAL, True)
    for walk in ((True, False, True), (True, True, False), (False, True, True), (False, False, True),
                 (False, True, False), (True, False, False)):
        assert run(fr.cov, fr.unc, nf, nfn, need, walk) == (_lib.SYZSIG_EINVAL, True)
    assert run(fr.cov, fr.unc, nf, nfn, need, (False, False, False))[0] == _lib.SYZSIG_OK
    with pytest.raises(_lib.SyzsigError) as e:
        report.file_set(fr, nlines, cap=need - 1)
    assert e.value.code == _lib.SYZSIG_ERANGE
    assert report.file_set_dict(fr, cap=need) == R.file_set(cov, unc)


def test_chain_corpus_to_cover_files(gpu):
    """Corpus -> cover_for -> report_pcs -> uncovered_pcs -> a table symbolizer that
    gives some PCs two inlined frames -> file_set with the walk (cover_files),
    against the restatements composed the same way; the files' IDs against sha1."""
    rng = np.random.default_rng(8)
    base = 0xFFFFFFFF
    names = ["read", "write", "mmap"]
    inputs = {f"i{k}": (names[k % 3], (0x81000000 + 16 * rng.integers(0, 400, size=25)).astype(np.uint32))
              for k in range(40)}
    corpus = report.Corpus(gpu, inputs)
    raw = report.cover_for(corpus).Serialize()
    lo = (base << 32) + 0x81000000
    syms = [(lo + 256 * k - 8, lo + 256 * k + 248) for k in range(26)]
    allc = [lo + 16 * k - 5 for k in range(400)]
    files = ["kernel/a.c", "./include/inl.h", "mm/b.c", "fs/c.c", ""]

    def table(pcs):
        """deterministic addr2line: the outer frame, and for every third site an inlined frame before it"""
        out = []
        for pc in pcs:
            site = (pc - lo + 5) // 16
            fn = f"fn{site // 16}"  # the function of syms that holds the site
            if site % 3 == 0:
                out.append(("./include/inl.h", int(site % 13), f"inl{site % 5}"))
            out.append((files[site // 16 % 5 if site // 16 % 5 != 1 else 0], int(site % 50 + 1), fn))
        return out

    calls = []

    def symbolize(t):
        assert torch.is_tensor(t) and t.dtype == torch.int64
        calls.append(t.numel())
        return table(t.cpu().numpy().view(np.uint64).tolist())

    nlines = {"kernel/a.c": 40, "./include/inl.h": 8, "mm/b.c": 50, "fs/c.c": 0, "": 25}
    got = report.cover_files(gpu, raw, base, "amd64", *report.sort_symbols(syms), report.all_cover_pcs(allc), symbolize,
                             nlines)
    pcs = RR.report_pcs(raw.tolist(), base, "amd64")[0]
    unc = RR.uncovered_pcs_in_funcs(syms, allc, pcs)
    assert calls == [len(pcs), len(unc)] and 0 < len(unc) < 400
    want = R.cover_files(table(pcs), table(unc), nlines)
    assert [g["Name"] for g in got] == [w[0] for w in want] and len(want) == 5 and want[-1][0] == "./include/inl.h"
    for g, (name, coverage, shown, lst) in zip(got, want):
        assert g["ID"] == hashlib.sha1(name.encode()).hexdigest()
        assert (g["Coverage"], g["shown"]) == (coverage, shown), name
        assert list(zip(g["line"].tolist(), g["covered"].tolist())) == lst, name
    assert any(w[1] for w in want) and any(w[2] < len(w[3]) for w in want)
    with pytest.raises(ValueError):  # "does not have debug info"
        report.cover_files(gpu, raw, base, "amd64", *report.sort_symbols(syms), report.all_cover_pcs(allc),
                           lambda t: [], nlines)
