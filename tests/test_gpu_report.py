"""GPU: the coverage-report kernels (csrc/report.hip) against tests/report_ref.py,
exactly -- everything is integers.  The hand-derived cases of
tests/report_cases.py run on the device as they run on the restatement."""
import ctypes

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, report
from syzkaller_amd import signal as S
from tests import report_cases as C
from tests import report_ref as R

pytestmark = pytest.mark.gpu

T = _lib.SYZSIG_COVER_TILE


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _check_call_cover(gpu, inputs, calls=(), select=None):
    """The device's per-call unions, counts and whole union against the restatement."""
    corpus = report.Corpus(gpu, inputs, calls)
    count, cover_len, off, cov, allc = report.call_cover(corpus, select, want_all=True)
    count, cover_len, off, cov, allc = _u32(count), _u32(cover_len), off.cpu().numpy(), _u32(cov), _u32(allc)
    rows = list(inputs.items()) if isinstance(inputs, dict) else [(r[0], (r[1], r[2])) for r in inputs]
    if select is not None:
        rows = [r for r, s in zip(rows, select) if s]
    want = R.collect_syscall_info(dict(rows))
    assert off[0] == 0 and off.size == corpus.ncalls + 1
    for c, name in enumerate(corpus.calls):
        n, cs = want.get(name, (0, set()))
        assert count[c] == n, name
        assert cover_len[c] == len(cs) == off[c + 1] - off[c], name
        assert cov[off[c]:off[c + 1]].tolist() == sorted(cs), name
    union = set().union(*[v[1] for v in want.values()]) if want else set()
    assert allc.tolist() == sorted(union)
    return corpus


# ---- part 1 ----

def test_call_cover_tile_boundaries(gpu):
    """Per-call union sizes T - 1, T, T + 1 and 2T + 3, each from several inputs
    without repeats, so that the segment lengths are the union sizes: two calls
    take the tile-sort and rank-merge path, 2T + 3 needs two passes."""
    rng = np.random.default_rng(1)
    inputs = {}
    for name, size in (("a", T - 1), ("b", T), ("c", T + 1), ("d", 2 * T + 3)):
        pcs = ((np.arange(size, dtype=np.uint64) * 2654435761 + int(rng.integers(1 << 32))) % (1 << 32)).astype(np.uint32)
        for k, part in enumerate(np.array_split(pcs, 5)):
            inputs[f"{name}{k}"] = (name, part)
    _check_call_cover(gpu, inputs)
    st = report.report_stats(gpu)
    assert st[0] == 2 and st[1] == 2


def test_call_cover_one_call_holds_every_input(gpu):
    rng = np.random.default_rng(2)
    inputs = {f"i{k}": ("read", rng.integers(0, 9000, size=int(rng.integers(0, 60))).astype(np.uint32))
              for k in range(400)}
    _check_call_cover(gpu, inputs)
    assert report.report_stats(gpu)[0] == 1  # about 12000 PCs in one segment
    info = report.syscall_info(report.Corpus(gpu, inputs))
    assert list(info) == ["read"] and info["read"][0] == 400


def test_call_cover_4000_calls_mostly_empty(gpu):
    rng = np.random.default_rng(3)
    calls = [f"c{k}" for k in range(4000)]
    inputs = {f"i{k}": (calls[int(rng.integers(0, 4000)) if k % 3 else 17],
                        rng.integers(0, 500, size=int(rng.integers(0, 40))).astype(np.uint32)) for k in range(300)}
    corpus = _check_call_cover(gpu, inputs, calls)
    info = report.syscall_info(corpus)
    want = R.collect_syscall_info(inputs)
    assert info == {k: (v[0], len(v[1])) for k, v in want.items()} and len(info) < 400


def test_call_cover_empty_corpus(gpu):
    _check_call_cover(gpu, {})
    _check_call_cover(gpu, {}, calls=["read", "write"])
    assert report.syscall_info(report.Corpus(gpu, {})) == {}
    assert report.cover_for(report.Corpus(gpu, {})).is_nil()


def test_call_cover_duplicates_and_hand_case(gpu):
    corpus = _check_call_cover(gpu, C.CORPUS, calls=["open"])
    assert report.syscall_info(corpus) == C.SYSCALL_INFO
    dup = np.array([5, 5, 5, 1, 1, 0xFFFFFFFF, 0, 0xFFFFFFFF], np.uint32)
    _check_call_cover(gpu, {"x": ("a", dup), "y": ("a", dup[::-1]), "z": ("b", dup), "w": ("b", [])})


def test_call_cover_select_and_cover_for(gpu):
    rng = np.random.default_rng(4)
    names = ["read", "write", "mmap"]
    inputs = {f"i{k}": (names[k % 3], rng.integers(0, 300, size=20).astype(np.uint32)) for k in range(30)}
    sel = np.zeros(30, np.uint8)
    sel[7] = 1
    _check_call_cover(gpu, inputs, select=sel)  # one input
    _check_call_cover(gpu, inputs, select=[k % 3 == 1 for k in range(30)])  # one call
    corpus = _check_call_cover(gpu, inputs)  # NULL
    for kw in ({}, {"call": "write"}, {"input": "i7"}, {"call": ""}):
        got = report.cover_for(corpus, **kw)
        assert sorted(got.Serialize().tolist()) == sorted(R.http_cover(inputs, **kw))
    assert report.cover_for(corpus, call="open").is_nil()  # no input matched: Go's cov stays nil
    with pytest.raises(KeyError):
        report.cover_for(corpus, input="nope")
    empty = report.cover_for(report.Corpus(gpu, {"e": ("read", [])}), input="e")
    assert not empty.is_nil() and len(empty) == 0  # merged into, and empty


def test_call_cover_errors_leave_outputs(gpu):
    corpus = report.Corpus(gpu, C.CORPUS)
    nc, n = corpus.ncalls, corpus.ninputs
    sentinel = 0x5A5A5A5A

    def run(off, call, cap):
        outs = [torch.full((nc,), sentinel, dtype=torch.int32, device=gpu.dev) for _ in range(2)]
        outs.append(torch.full((nc + 1,), sentinel, dtype=torch.int64, device=gpu.dev))
        outs += [torch.full((corpus.total,), sentinel, dtype=torch.int32, device=gpu.dev) for _ in range(2)]
        n_all = ctypes.c_uint64(77)
        rc = gpu.L.syzsig_call_cover_dev(gpu.eng.h, off.data_ptr(), corpus.cov.data_ptr(), n, corpus.total,
                                         call.data_ptr(), None, nc, outs[0].data_ptr(), outs[1].data_ptr(),
                                         outs[2].data_ptr(), outs[3].data_ptr(), cap, outs[4].data_ptr(),
                                         ctypes.byref(n_all))
        torch.cuda.synchronize()
        untouched = all(bool((o == sentinel).all()) for o in outs) and n_all.value == 77
        return rc, untouched

    assert run(corpus.off, corpus.call, corpus.total) == (_lib.SYZSIG_OK, False)
    assert run(corpus.off, corpus.call, corpus.total - 1) == (_lib.SYZSIG_ERANGE, True)
    bad_call = corpus.call.clone()
    bad_call[2] = nc
    assert run(corpus.off, bad_call, corpus.total) == (_lib.SYZSIG_EINVAL, True)
    bad_off = corpus.off.clone()
    bad_off[1], bad_off[2] = corpus.off[2], corpus.off[1]
    assert run(bad_off, corpus.call, corpus.total) == (_lib.SYZSIG_EINVAL, True)
    short = corpus.off.clone()
    short[-1] -= 1
    assert run(short, corpus.call, corpus.total) == (_lib.SYZSIG_EINVAL, True)


# ---- part 2 ----

@pytest.mark.parametrize("case", C.REPORT_PCS, ids=[c[0] for c in C.REPORT_PCS])
def test_report_pcs_hand_cases(gpu, case):
    _, arch, base, pcs, order, srt = case
    o, s = report.report_pcs(gpu, np.array(pcs, np.uint32), base, arch)
    assert _u64(o).tolist() == order and _u64(s).tolist() == srt


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2 * 2048 + 3])
def test_report_pcs_sizes_every_arch(gpu, n):
    """The last size leaves the one-workgroup sort (2048 keys of two words)."""
    rng = np.random.default_rng(n)
    pcs = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    pcs[: n // 4] = rng.integers(0, 8, size=n // 4)  # below every subtrahend at base 0: the wrap; repeats
    for arch in report.ARCH:
        for base in (0, 0xFFFFFFFF):
            o, s = report.report_pcs(gpu, pcs, base, arch)
            wo, ws = R.report_pcs(pcs.tolist(), base, arch)
            assert _u64(o).tolist() == wo and _u64(s).tolist() == ws


def test_report_pcs_unknown_arch_and_text(gpu):
    for arch in (5, "mips"):
        with pytest.raises(_lib.SyzsigError) as e:
            report.report_pcs(gpu, np.array([1], np.uint32), 0, arch)
        assert e.value.code == _lib.SYZSIG_EINVAL
    cov = S.Cover(gpu.eng)
    cov.Merge(np.array([0x1006, 0x1009, 0x1005, 0x1009], np.uint32))
    assert report.raw_cover_text(cov, 0, "arm", gpu) == "0x1002\n0x1002\n0x1006\n"
    assert report.raw_cover_text(cov, 0, "arm") == R.raw_cover_text([0x1005, 0x1006, 0x1009], 0, "arm")


# ---- part 3 ----

def _uncovered(gpu, syms, allc, pcs):
    a = np.array(syms, np.uint64).reshape(-1, 2)
    return _u64(report.uncovered_pcs(gpu, a[:, 0], a[:, 1], np.array(allc, np.uint64), np.array(pcs, np.uint64))).tolist()


@pytest.mark.parametrize("case", C.UNCOVERED, ids=[c[0] for c in C.UNCOVERED])
def test_uncovered_hand_cases(gpu, case):
    _, syms, allc, pcs, want = case
    assert _uncovered(gpu, syms, allc, pcs) == want


def _overlapping_symbols(rng, nsym, span):
    """Symbols over [0, span): nested, aliased, zero-size and disjoint ones, sorted by start."""
    start = np.sort(rng.integers(0, span, size=nsym))
    start[rng.random(nsym) < 0.15] = 0  # marks: made aliases of their predecessor below
    for i in range(1, nsym):
        if start[i] == 0:
            start[i] = start[i - 1]
    size = rng.integers(0, max(span // nsym, 2) * 6, size=nsym)
    size[rng.random(nsym) < 0.05] = 0
    return [(int(s), int(s + z)) for s, z in zip(start, size)]


@pytest.mark.parametrize("npc", [1, 64, 65, 256, 257])
@pytest.mark.parametrize("nsym", [1, 2, 257])
def test_uncovered_sizes(gpu, npc, nsym):
    rng = np.random.default_rng(1000 * nsym + npc)
    syms = _overlapping_symbols(rng, nsym, 4000)
    allc = report.all_cover_pcs(rng.integers(0, 4200, size=1500)).tolist()
    pcs = rng.integers(0, 4200, size=npc).tolist()
    assert _uncovered(gpu, syms, allc, pcs) == R.uncovered_pcs_in_funcs(syms, allc, pcs)


def test_uncovered_block_path_and_stats(gpu):
    """One function of 1000 sites among 3000 of 0-3 sites each."""
    rng = np.random.default_rng(5)
    syms, allc, at = [], [], 100
    for f in range(3001):
        nsites = 1000 if f == 1234 else int(rng.integers(0, 4))
        size = 4 * nsites + 8
        syms.append((at, at + size))
        allc += [at + 4 * k + 2 for k in range(nsites)]
        at += size + int(rng.integers(1, 9))
    pcs = [int(s + rng.integers(0, e - s)) for s, e in syms if rng.random() < 0.5]
    big = syms[1234]
    pcs += [big[0] + 2, big[0] + 6, big[0] + 2]
    pcs = [pcs[i] for i in rng.permutation(len(pcs))]
    got = _uncovered(gpu, syms, allc, pcs)
    assert got == R.uncovered_pcs_in_funcs(syms, allc, pcs)
    st = report.report_stats(gpu)
    assert st[3] == 1 and st[2] == len(_handled(syms, pcs))
    assert sum(big[0] < q < big[1] for q in got) == 998


def _handled(syms, pcs):
    """The keys of handledFuncs, by the restated search."""
    out = set()
    for pc in pcs:
        idx = R.sort_search(len(syms), lambda i: pc < syms[i][1])
        if idx < len(syms) and syms[idx][0] <= pc <= syms[idx][1]:
            out.add(syms[idx][0])
    return out


def test_uncovered_two_shuffles_differ(gpu):
    """The same pcs in two orders whose reference results differ: abutting
    functions share their boundary site, as A and B of the worked example."""
    rng = np.random.default_rng(6)
    syms = [(100 * k, 100 * k + 100) for k in range(300)]
    allc = sorted({100 * k for k in range(301)} | set(rng.integers(0, 30000, size=2000).tolist()))
    pcs = [100 * k for k in range(1, 300)] + [100 * k + 50 for k in range(300)]
    a = [pcs[i] for i in rng.permutation(len(pcs))]
    b = [pcs[i] for i in rng.permutation(len(pcs))]
    wa, wb = R.uncovered_pcs_in_funcs(syms, allc, a), R.uncovered_pcs_in_funcs(syms, allc, b)
    assert wa != wb
    assert _uncovered(gpu, syms, allc, a) == wa and _uncovered(gpu, syms, allc, b) == wb


def test_uncovered_random_batch_overlapping(gpu):
    rng = np.random.default_rng(7)
    syms = _overlapping_symbols(rng, 900, 60000)
    allc = report.all_cover_pcs(rng.integers(0, 61000, size=20000)).tolist()
    pcs = rng.choice(np.array(allc + list(range(0, 61000, 7))), size=5000).tolist()
    assert _uncovered(gpu, syms, allc, pcs) == R.uncovered_pcs_in_funcs(syms, allc, pcs)


def test_uncovered_rejects_repeats_and_unsorted(gpu):
    for allc in ([12, 12, 15], [15, 12]):
        with pytest.raises(_lib.SyzsigError) as e:
            _uncovered(gpu, [(10, 20)], allc, [12])
        assert e.value.code == _lib.SYZSIG_EINVAL
    with pytest.raises(_lib.SyzsigError) as e:
        _uncovered(gpu, [(30, 40), (10, 20)], [12], [12])
    assert e.value.code == _lib.SYZSIG_EINVAL
    assert report.all_cover_pcs([15, 12, 12]).tolist() == [12, 15]


# ---- chain ----

def test_chain_new_input_to_uncovered(gpu):
    """manager_new_input's key covers -> syscall_info -> cover_for -> report_pcs -> uncovered_pcs."""
    rng = np.random.default_rng(8)
    base, nkeys = 0xFFFFFFFF, 12
    names = ["read", "write", "mmap"]
    rows = []
    for i in range(40):
        e = rng.choice(5000, size=30, replace=False).astype(np.uint32)
        cover = (0x81000000 + 16 * rng.integers(0, 400, size=25)).astype(np.uint32)
        rows.append((int(rng.integers(0, nkeys)), S.Serial(e, np.zeros(30, np.int8)), cover))
    cs, cc = S.Signal(None, gpu.eng), S.Cover(gpu.eng)
    _, _, entries = S.manager_new_input(cs, cc, rows, nkeys, gpu.eng)
    inputs = {f"k{k}": (names[k % 3], cov) for k, (_, cov) in entries.items()}
    corpus = report.Corpus(gpu, inputs)
    want = R.collect_syscall_info(inputs)
    assert report.syscall_info(corpus) == {k: (v[0], len(v[1])) for k, v in want.items()}
    cov = report.cover_for(corpus)
    assert sorted(cov.Serialize().tolist()) == sorted(cc.Serialize().tolist())  # the manager's corpusCover
    raw = cov.Serialize()
    order, _ = report.report_pcs(gpu, raw, base, "amd64")
    pcs = _u64(order).tolist()
    assert pcs == R.report_pcs(raw.tolist(), base, "amd64")[0]
    lo = (base << 32) + 0x81000000
    syms = [(lo + 256 * k - 8, lo + 256 * k + 248) for k in range(26)]
    allc = [lo + 16 * k - 5 for k in range(400)]
    got = _u64(report.uncovered_pcs(gpu, *report.sort_symbols(syms), report.all_cover_pcs(allc), order)).tolist()
    assert got == R.uncovered_pcs_in_funcs(syms, allc, pcs) and 0 < len(got) < 400
