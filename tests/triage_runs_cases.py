"""Triage-item batches built for csrc/stable.hip, with the outcome each item
must have worked out by hand (no GPU use, no Signal op).

syzsig_triage_runs_dev and syzsig_minimize_pred_dev read the same nine arrays
(the layout of make_items in test_gpu_triage_runs.py):

  item_off u64[n + 1], elems u32[], prios i8[], item_flags u8[n]
  run_off u64[n * R + 1], run_sigs u32[], run_prio u8[n * R],
  run_errno i32[n * R], run_exec u8[n * R]

item i's newSignal is elems/prios[item_off[i] : item_off[i + 1]], its r-th
re-run (triage_runs) or attempt (minimize_pred) is run i * R + r.  Every
builder returns a Case: the arrays, R, and the expected item_keep, per-element
keep and predicate, each derived from the rule its comment states.  An element
of a dropped item has keep 0.  Builders are cached, the arrays read-only: the
triage_runs test and the minimize_pred test of a batch share one build."""
import functools
from typing import NamedTuple

import numpy as np

MINIMIZED = 1  # SYZSIG_TRIAGE_MINIMIZED: item.flags & ProgMinimized
ORIG_OK = 2    # SYZSIG_TRIAGE_ORIG_OK:   item.info.Errno == 0
MAX_RUNS = 8   # kStableMaxRuns
BLOCK = 256    # threads of k_runs_insert / k_stable_elems / k_stable_final
GRID_CAP = 8192  # their block cap: past it a block serves a second item or run

EINVAL_ERRNO = 22


class Case(NamedTuple):
    arrays: tuple       # the nine arrays
    runs: int           # R = runs per item = attempts per item
    keep: np.ndarray    # u8[n]     item_keep
    elem_keep: np.ndarray  # u8[nelem] membership in the final newSignal of a kept item
    pred: np.ndarray    # u8[n]     the minimize predicate


class _Batch:
    """Collects items; a run is (raw signal, prio byte, errno, executed)."""

    def __init__(self, runs):
        self.R = runs
        self.elems, self.prios, self.flags = [], [], []
        self.sigs, self.rprio, self.rerrno, self.rexec = [], [], [], []
        self.keep, self.ek, self.pred = [], [], []

    def item(self, elems, prios, flags, runs, keep, elem_keep, pred):
        e = np.asarray(elems, np.uint32)
        ek = np.asarray(elem_keep, np.uint8)
        assert len(runs) == self.R and e.size == len(prios) == ek.size
        assert keep or not ek.any()
        self.elems.append(e)
        self.prios.append(np.asarray(prios, np.int8))
        self.flags.append(flags)
        for sig, prio, errno, executed in runs:
            self.sigs.append(np.asarray(sig, np.uint32))
            self.rprio.append(prio)
            self.rerrno.append(errno)
            self.rexec.append(executed)
        self.keep.append(keep)
        self.ek.append(ek)
        self.pred.append(pred)

    def case(self):
        def cat(xs, dt):
            return np.concatenate(xs).astype(dt) if xs else np.empty(0, dt)

        def off(xs):
            return np.concatenate([[0], np.cumsum([x.size for x in xs], dtype=np.uint64)]).astype(np.uint64)

        arrays = (off(self.elems), cat(self.elems, np.uint32), cat(self.prios, np.int8),
                  np.array(self.flags, np.uint8), off(self.sigs), cat(self.sigs, np.uint32),
                  np.array(self.rprio, np.uint8), np.array(self.rerrno, np.int32), np.array(self.rexec, np.uint8))
        out = Case(arrays, self.R, np.array(self.keep, np.uint8), cat(self.ek, np.uint8),
                   np.array(self.pred, np.uint8))
        for a in arrays + (out.keep, out.elem_keep, out.pred):
            a.setflags(write=False)
        return out


def _good(sig, prio=0):
    return (sig, prio, 0, 1)


# proc.go:122-130: a run is skipped when the call was not executed (len(info) ==
# 0), has no signal, or failed (Errno != 0) although item.info.Errno == 0; the
# item is given up once notexecuted > signalRuns/2 + 1.  A skipped run changes
# nothing, so an item kept with k <= R/2 + 1 skipped runs keeps all three
# elements -- also when no run is usable at all (R <= 2).  An Errno != 0 run of
# an item whose original failed too (no ORIG_OK) is used (:123).
# The predicate (:144-161) passes over an unexecuted or empty attempt, answers
# false at a failed one (ORIG_OK) and true at a usable one, which here holds
# all of newSignal: it is the answer of the first attempt that is neither
# unexecuted nor empty, false when there is none.
@functools.lru_cache(maxsize=None)
def skip_table(R):
    assert 1 <= R <= MAX_RUNS
    b = _Batch(R)
    causes = ("noexec", "empty", "fail")
    n = 0
    for k in range(R + 1):
        first = list(range(k))
        last = list(range(R - k, R))
        alt = ([r for r in range(0, R, 2)] + [r for r in range(1, R, 2)])[:k]
        for place in (first, last, alt):
            for shift in range(3):
                e = np.arange(3, dtype=np.uint32) + np.uint32(16 * n)
                other = e + np.uint32(8)  # what a skipped run saw: nothing of the item
                n += 1
                kind = {r: causes[(j + shift) % 3] for j, r in enumerate(sorted(place))}
                runs = []
                for r in range(R):
                    c = kind.get(r)
                    runs.append(_good(e) if c is None else (other, 0, 0, 0) if c == "noexec"
                                else ([], 0, 0, 1) if c == "empty" else (other, 0, EINVAL_ERRNO, 1))
                keep = int(k <= R // 2 + 1)
                deciding = [kind.get(r) for r in range(R) if kind.get(r) not in ("noexec", "empty")]
                pred = int(bool(deciding) and deciding[0] is None)
                b.item(e, [0, 0, 0], ORIG_OK, runs, keep, [keep] * 3, pred)
        # control: the k runs failed, but so had the original: they are used
        e = np.arange(3, dtype=np.uint32) + np.uint32(16 * n)
        n += 1
        b.item(e, [0, 0, 0], 0, [(e, 0, EINVAL_ERRNO if r < k else 0, 1) for r in range(R)], 1, [1, 1, 1], 1)
    # the give-up rule cannot drop an item for R <= 2; so that every batch holds a
    # dropped item and a false predicate: usable runs without any of its elements
    # (proc.go:136-138, :157)
    e = np.arange(3, dtype=np.uint32) + np.uint32(16 * n)
    b.item(e, [0, 0, 0], ORIG_OK, [_good(e + np.uint32(8))] * R, 0, [0, 0, 0], 0)
    return b.case()


PRIO_ELEM = (-128, -1, 0, 1, 127)
PRIO_RUN = (0, 1, 127, 128, 255)


# signal.go:31-37 FromRaw stores prioType(prio), an int8, so a prio byte of
# 128..255 is -128..-1; signal.go:104-115 Intersection keeps e iff the run has
# it with p1 >= p.  One usable run: the element survives iff int8(run prio) >=
# its prio; proc.go:136 drops the emptied item unless it is minimized; the
# predicate (:157) is true iff the one element survives.
@functools.lru_cache(maxsize=None)
def prio_grid():
    b = _Batch(1)
    n = 0
    for flags in (0, MINIMIZED):
        for pe in PRIO_ELEM:
            for rp in PRIO_RUN:
                e = np.uint32(1000 + n)
                n += 1
                as_int8 = rp - 256 if rp >= 128 else rp
                lives = int(as_int8 >= pe)
                b.item([e], [pe], flags, [_good([e, e], rp)], int(lives or flags == MINIMIZED), [lives], lives)
    return b.case()


# Hand-listed items, R = 3.  proc.go:133 chains the Intersections: what one run
# removed stays removed; the predicate (:157) intersects the untouched newSignal
# with every attempt on its own.  Each item's comment gives the reasoning.
@functools.lru_cache(maxsize=None)
def chains():
    b = _Batch(3)
    # 10 is in runs 0 and 2 but not in run 1: run 1 removes it for good.  Attempt 0 holds both.
    b.item([10, 11], [0, 0], 0, [_good([10, 11]), _good([11]), _good([11, 10])], 1, [0, 1], 1)
    # 20 (prio 2) is in all runs, the last at prio 1 < 2 (signal.go:110): dead.  Attempt 0 is at prio 2.
    b.item([20, 21], [2, 0], 0, [_good([20, 21], 2), _good([21, 20], 2), _good([20, 21], 1)], 1, [0, 1], 1)
    # a skipped run (not executed; what it saw is never read) between two usable
    # ones; run 2 lacks 30.
    b.item([30, 31], [0, 0], 0, [_good([30, 31]), ([99], 0, 0, 0), _good([31])], 1, [0, 1], 1)
    # run 0 removes 36 for triage; attempt 0 is not all of newSignal, attempt 1 is
    # passed over, attempt 2 alone holds all of it: predicate true
    b.item([35, 36], [0, 0], 0, [_good([35]), ([35, 36], 0, 0, 0), _good([36, 35])], 1, [1, 0], 1)
    # minimized, emptied by run 0 (proc.go:136 does not return): stays empty
    # although run 2 holds everything; kept with an empty newSignal.  Attempt 2 is a yes.
    emptied = [_good([77]), _good([78]), _good([40, 41, 42])]
    b.item([40, 41, 42], [0, 0, 0], MINIMIZED, emptied, 1, [0, 0, 0], 1)
    # the same, not minimized: dropped at run 0
    b.item([40, 41, 42], [0, 0, 0], 0, emptied, 0, [0, 0, 0], 1)
    # neighbours with the same elements: A's runs hold them, B's do not
    b.item([50, 51, 52], [0, 0, 0], 0, [_good([50, 51, 52])] * 3, 1, [1, 1, 1], 1)
    b.item([50, 51, 52], [0, 0, 0], 0, [_good([60, 61])] * 3, 0, [0, 0, 0], 0)
    # and the other way round: the later item's runs hold them
    b.item([55, 56], [0, 0], 0, [_good([57])] * 3, 0, [0, 0], 0)
    b.item([55, 56], [0, 0], 0, [_good([56, 55])] * 3, 1, [1, 1], 1)
    # empty newSignal (proc.go:109-111: nothing to triage, minimized or not).
    # Intersection of the empty set has Len 0 == Len: the first executed attempt
    # with signal is a yes; with none, no.
    b.item([], [], MINIMIZED, [([], 0, 0, 1), ([5], 0, 0, 0), _good([5])], 0, [], 1)
    b.item([], [], 0, [([], 0, 0, 1), ([5], 0, 0, 0), ([], 0, 0, 0)], 0, [], 0)
    # the original succeeded, attempt 0 failed: false (proc.go:150-154) although
    # attempts 1 and 2 hold everything.  Triage skips run 0 (1 <= 3/2 + 1) and keeps all.
    failed_first = [([1000], 0, EINVAL_ERRNO, 1), _good([70, 71]), _good([71, 70])]
    b.item([70, 71], [0, 0], ORIG_OK, failed_first, 1, [1, 1], 0)
    # the original had failed too: attempt 0 is an ordinary no, attempt 1 a yes;
    # triage uses run 0, which empties the item
    b.item([70, 71], [0, 0], 0, failed_first, 0, [0, 0], 1)
    return b.case()


SIZES_ITEMS = (1, 255, 256, 257, 1000)
SIZES_RUNS = {1: (1, 1), 255: (255, 256), 256: (256, 257), 257: (257, 255), 1000: (5000, 5000)}


def _tile(vals, n, rng):
    """a raw signal of n entries over vals: every value at least once when n allows, in a fixed shuffled order"""
    v = np.asarray(vals, np.uint32)
    assert 0 < v.size <= n
    return rng.permutation(np.resize(v, n))


# R = 2, item and run sizes on both sides of the 256-thread block.  Run 0 is
# the whole item as a raw signal with duplicates (FromRaw, signal.go:31-39,
# makes a set of it), run 1 leaves out the elements of index % 3 == 1: exactly
# those die (signal.go:104-115), the item is kept (index 0 survives).  Element
# prio is index % 3, the runs have prio 2 >= it.  Attempt 0 holds all: true.
# A second item of each size has run 0 = the same survivors and run 1 = values
# it does not hold: dropped (proc.go:136-138), and the predicate is false
# unless nothing was left out (the item of one element).
@functools.lru_cache(maxsize=None)
def sizes():
    b = _Batch(2)
    rng = np.random.default_rng(256)
    for j, n in enumerate(SIZES_ITEMS):
        # ascending, from 0 up to 0xFFFFFFFF for the two largest items
        e = np.arange(n, dtype=np.uint32) * np.uint32(7) + np.uint32(0 if n >= 257 else 100000 * (j + 1))
        if n >= 257:
            e[-1] = 0xFFFFFFFF
        idx = np.arange(n)
        live = idx % 3 != 1
        t0, t1 = SIZES_RUNS[n]
        b.item(e, idx % 3, 0, [_good(_tile(e, t0, rng), 2), _good(_tile(e[live], t1, rng), 2)], 1,
               live.astype(np.uint8), 1)
        foreign = e[live] + np.uint32(3)  # the elements are 7 apart (0xFFFFFFFF + 3 wraps to 2)
        assert not np.isin(foreign, e).any()
        b.item(e, idx % 3, 0, [_good(_tile(e[live], t0, rng), 2), _good(_tile(foreign, t1, rng), 2)], 0,
               np.zeros(n, np.uint8), int(live.all()))
    return b.case()


MANY_ITEMS = GRID_CAP + 8


# More items and more runs than the 8192 blocks, R = 2, prio 0 throughout.
# Item i by i % 3 (8192 % 3 == 2, so items i and i - 8192 never agree):
#   0  both runs hold the item: kept whole, predicate true at attempt 0
#   1  run 0 lacks element 0, run 1 holds all: element 0 is gone (proc.go:133
#      chains), the others stay (two or three elements); attempt 1 is a yes
#   2  neither run holds any of it: dropped at run 0, predicate false
@functools.lru_cache(maxsize=None)
def many():
    b = _Batch(2)
    for i in range(MANY_ITEMS):
        kind = i % 3
        n = 2 + (i // 3) % 2 if kind == 1 else 1 + (i // 3) % 3
        e = np.arange(n, dtype=np.uint32) + np.uint32(4 * i)  # items share no element
        if kind == 0:
            b.item(e, [0] * n, 0, [_good(e), _good(e[::-1])], 1, [1] * n, 1)
        elif kind == 1:
            b.item(e, [0] * n, 0, [_good(e[1:]), _good(e)], 1, [0] + [1] * (n - 1), 1)
        else:
            other = [np.uint32(4 * i + 3)]
            b.item(e, [0] * n, 0, [_good(other), _good(other)], 0, [0] * n, 0)
    return b.case()


# R = 0: the loop of proc.go:120 does not run, so an item with new signal is
# kept whole and one without is not triaged (:109-111); with no attempt the
# predicate is false (:161).
@functools.lru_cache(maxsize=None)
def no_runs():
    b = _Batch(0)
    b.item([1, 2, 3], [0, 1, -1], 0, [], 1, [1, 1, 1], 0)
    b.item([], [], MINIMIZED, [], 0, [], 0)
    b.item([2 ** 32 - 1], [3], ORIG_OK, [], 1, [1], 0)
    return b.case()


def all_cases():
    """(name, builder call) of every batch the GPU tests run"""
    return ([(f"skip_table-{R}", functools.partial(skip_table, R)) for R in range(1, MAX_RUNS + 1)] +
            [("prio_grid", prio_grid), ("chains", chains), ("sizes", sizes), ("many", many)])
