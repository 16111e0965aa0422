"""prog/prio.go:133-245 restated line by line in numpy float32, every operation
rounded on its own (the reference on amd64 has no fused multiply-add):
calcDynamicPrio, normalizePrio, the product of CalculatePriorities, the
deterministic tail of calcStaticPriorities (:118-129), BuildChoiceTable and the
lookup of Choose.  The device (csrc/prio.hip) is held to this bit for bit, and
tests/test_prio_ref_cpu.py holds this to cases worked by hand.

`fused=True` evaluates normalizePrio's `q*0.9 + 0.1` as one fused multiply-add
(exactly, in float64, then rounded once).  It exists only so that a test can
show that the two evaluations differ; nothing else uses it.
"""
import numpy as np

F = np.float32
CLAMP = 1 << 24  # float32 `+= 1.0` sticks here: 2^24 + 1 is not representable and rounds back to even


def pair_counts(corpus, ncalls):
    """The integer number of ordered pairs (position of id0, position of id1)
    per cell over every program, prio.go:138-146 without the float: for one
    program it is occ(id0) * occ(id1), self-pairs and repeats included."""
    cnt = np.zeros((ncalls, ncalls), np.int64)
    for prog in corpus:
        ids = np.asarray(prog, np.int64)
        if ids.size == 0:
            continue
        if ids.min() < 0 or ids.max() >= ncalls:
            raise IndexError("call id out of range")  # (Go panics on the index)
        occ = np.bincount(ids, minlength=ncalls)
        nz = np.flatnonzero(occ)
        cnt[np.ix_(nz, nz)] += np.outer(occ[nz], occ[nz])
    return cnt


def counts_to_f32(cnt):
    """prios[id0][id1] += 1.0, count times: exactly min(count, 2^24)."""
    return np.minimum(np.asarray(cnt, np.int64), CLAMP).astype(F)


def normalize_row(prio, fused=False):
    """normalizePrio's body for one row (prio.go:154-186), in place on a float32 row."""
    assert prio.dtype == F
    mx = F(0)  # :155
    mn = F(1e10)  # :156
    nzero = 0
    for p in prio:  # :158-168
        if mx < p:
            mx = p
        if p != 0 and mn > p:
            mn = p
        if p == 0:
            nzero += 1
    with np.errstate(all="ignore"):
        if nzero != 0:  # :169-171
            mn = F(mn / F(F(2) * F(nzero)))
        for i in range(prio.size):  # :172-185
            p = prio[i]
            if mx == 0:
                prio[i] = F(1)
                continue
            if p == 0:
                p = mn
            q = F(F(p - mn) / F(mx - mn))
            if fused:
                p = F(np.float64(q) * np.float64(F(0.9)) + np.float64(F(0.1)))  # exact in float64, one rounding
            else:
                p = F(F(q * F(0.9)) + F(0.1))
            if p > 1:
                p = F(1)
            prio[i] = p
    return prio


def normalize_prio(prios, fused=False):
    """normalizePrio, the same thing row-vectorised (checked against normalize_row by the CPU tests)."""
    prios = np.array(prios, F, copy=True)
    if prios.size == 0:
        return prios
    with np.errstate(all="ignore"):
        mx = np.maximum(F(0), np.where(np.isnan(prios), F(0), prios).max(axis=1)).astype(F)
        nonzero = (prios != 0) & ~np.isnan(prios)
        mn = np.minimum(F(1e10), np.where(nonzero, prios, F(np.inf)).min(axis=1)).astype(F)
        nzero = (prios == 0).sum(axis=1)
        div = (F(2) * nzero.astype(F)).astype(F)
        mn = np.where(nzero != 0, (mn / np.where(nzero != 0, div, F(1))).astype(F), mn).astype(F)
        p = np.where(prios == 0, mn[:, None], prios).astype(F)
        q = ((p - mn[:, None]).astype(F) / (mx - mn).astype(F)[:, None]).astype(F)
        if fused:
            r = (q.astype(np.float64) * np.float64(F(0.9)) + np.float64(F(0.1))).astype(F)
        else:
            r = ((q * F(0.9)).astype(F) + F(0.1)).astype(F)
        r = np.where(r > 1, F(1), r).astype(F)
        r[mx == 0] = F(1)
    return r


def calc_dynamic_prio(corpus, ncalls, fused=False):
    """calcDynamicPrio, prio.go:133-149."""
    return normalize_prio(counts_to_f32(pair_counts(corpus, ncalls)), fused)


def calculate_priorities(corpus, ncalls, static=None, fused=False):
    """CalculatePriorities, prio.go:27-36, with the static matrix an input."""
    dyn = calc_dynamic_prio(corpus, ncalls, fused)
    if static is not None:
        with np.errstate(all="ignore"):
            dyn = (dyn * np.asarray(static, F)).astype(F)  # :32
    return dyn


def static_finish(mat):
    """The tail of calcStaticPriorities, prio.go:118-129, on the summed matrix:
    pp[c0] = the row's max with whatever the diagonal holds on entry (0 in the
    reference, which skips c0 == c1), then normalizePrio."""
    m = np.array(mat, F, copy=True)
    for c0 in range(m.shape[0]):
        mx = F(0)
        for p in m[c0]:
            if mx < p:
                mx = p
        m[c0, c0] = mx
    return normalize_prio(m)


def build_choice_table(prios, enabled, ncalls):
    """BuildChoiceTable, prio.go:198-228: run int32[N, N]; a disabled row (nil
    in Go) is a row of zeros.  int() of a NaN, negative or too large weight is
    implementation-defined in Go: ValueError, naming the first such row."""
    en = np.ones(ncalls, bool) if enabled is None else np.asarray(enabled).astype(bool)
    run = np.zeros((ncalls, ncalls), np.int32)
    for i in range(ncalls):
        if not en[i]:
            continue
        s = 0
        for j in range(ncalls):
            if en[j]:
                w = 1
                if prios is not None:
                    x = F(F(prios[i][j]) * F(1000))
                    if not (x >= 0) or x >= F(2 ** 31) / F(ncalls):
                        raise ValueError(f"row {i}: weight out of range")
                    w = int(x)
                s += w
            run[i, j] = s
    return run


def build_choice_table_fast(prios, enabled, ncalls):
    """build_choice_table row-vectorised (checked against it by the CPU tests), for the larger N."""
    en = np.ones(ncalls, bool) if enabled is None else np.asarray(enabled).astype(bool)
    if prios is None:
        w = np.ones((ncalls, ncalls), np.int64)
    else:
        with np.errstate(all="ignore"):
            x = (np.asarray(prios, F) * F(1000)).astype(F)
        bad = (~(x >= 0) | (x >= F(2 ** 31) / F(ncalls))) & en[:, None] & en[None, :]
        if bad.any():
            raise ValueError(f"row {int(np.flatnonzero(bad.any(axis=1))[0])}: weight out of range")
        w = np.where(bad | ~en[None, :], 0, np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)).astype(np.int64)
    w = w * en[None, :] * en[:, None]
    return np.cumsum(w, axis=1).astype(np.int32)


def search_ints(run_row, x):
    """sort.SearchInts: the smallest i with run_row[i] >= x (len if none)."""
    lo, hi = 0, len(run_row)
    while lo < hi:
        mid = (lo + hi) // 2
        if run_row[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def lookup(run, enabled, call, x):
    """Choose's lookup, prio.go:230-245, for a given draw x: the sentinel N for
    call < 0 or a disabled (nil) row, else SearchInts; x outside [1, total]
    cannot come from r.Intn(total) + 1: ValueError."""
    n = run.shape[0]
    en = np.ones(n, bool) if enabled is None else np.asarray(enabled).astype(bool)
    if call < 0 or not en[call]:
        return n
    total = int(run[call, n - 1])
    if x < 1 or x > total:
        raise ValueError("x outside [1, total]")
    return search_ints(run[call], x)
