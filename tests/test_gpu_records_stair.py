"""GPU: the owner side of a sharded step (csrc/recs.hip, and the per-record
path behind exact=True) on the exhaustive table the finalize is pinned to
(tests/agg_keys.py staircase_cases), against the compiled oracle."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import agg_keys as AK

pytestmark = pytest.mark.gpu

LEVELS = [0, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def _case():
    """The staircase batch as shuffled records e << 32 | level << 24 | serial
    (serial = the call's index), about ten of them twice, and what the oracle's
    sequential checkNewSignal makes of the batch.  Shared and read-only."""
    elems, orders, (hs, hcs, hcnt, hprio), (m0e, m0p) = AK.staircase_cases()
    oms, ons, obits, _ = O.triage_batch(m0e, m0p, hs, hcs, hcnt, hprio)
    call = np.repeat(np.arange(hcnt.size, dtype=np.uint64), hcnt)
    rec = (hs.astype(np.uint64) << np.uint64(32)) | (hprio[call].astype(np.uint64) << np.uint64(24)) | call
    new = np.unpackbits(obits.view(np.uint8), bitorder="little")[: rec.size].astype(np.uint8)
    assert rec.size == 1300 and np.array_equal(np.unique(hs), np.sort(elems))  # every element of the table
    rng = np.random.default_rng(320)
    # within-call duplicates (same element, level and serial): DiffRaw collapses
    # them, so both copies carry the flag -- five new records and five old ones
    dup = np.concatenate([rng.choice(np.nonzero(new)[0], 5, replace=False),
                          rng.choice(np.nonzero(new == 0)[0], 5, replace=False)])
    rec, new = np.concatenate([rec, rec[dup]]), np.concatenate([new, new[dup]])
    perm = rng.permutation(rec.size)
    rec, new = rec[perm], new[perm]
    oe, op = oms.Serialize()
    ne, npr = ons.Serialize()
    want = {"rec": rec, "new": new, "m0e": m0e, "m0p": m0p, "max": (oe, op), "newsig": (ne, npr)}
    for v in want.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    # each element changes at most once: newSignal holds exactly the changed ones
    want["changed"], want["inserted"] = int(ne.size), int(oe.size - m0e.size)
    assert want["changed"] > 0 and want["inserted"] > 0 and 0 < int(new.sum()) < new.size
    return want


def _own(gpu, w, shard, ns, exact):
    """One step_own of the records as the only source's bucket + step_finish
    -> (status byte, the records' flags, the step's status)."""
    n = w["rec"].size
    cap = n + 5
    recv = torch.zeros(cap + 1, dtype=torch.int64, device=gpu.dev)
    recv[0] = n
    recv[1: 1 + n] = torch.from_numpy(w["rec"].view(np.int64).copy()).to(gpu.dev)
    f = torch.full((cap + 1,), 7, dtype=torch.uint8, device=gpu.dev)
    gpu.step_own(shard, ns, recv, 1, cap, LEVELS, f, exact=exact)
    st = gpu.step_finish()
    f = f.cpu().numpy()
    return int(f[0]), f[1: 1 + n], st


def _same(dev_sig, elems, prios, eng):
    """dev_sig holds exactly (elems, prios): by Len, by Diff both ways, and entry by entry."""
    from syzkaller_amd import signal as S

    want = S.Serial(elems.copy(), prios.copy()).Deserialize(eng)
    assert dev_sig.Len() == want.Len() == elems.size
    assert dev_sig.Diff(want).Len() == 0 and want.Diff(dev_sig).Len() == 0
    assert dev_sig.to_dict() == {int(e): int(p) for e, p in zip(elems, prios)}


def _entries(sig):
    """A set's Serial in element order."""
    ser = sig.Serialize()
    k = np.argsort(ser.Elems, kind="stable")
    return ser.Elems[k], ser.Prios[k]


@pytest.mark.parametrize("exact", [False, True], ids=["lds", "exact"])
def test_step_own_staircase_every_order(gpu, exact):
    """Every order of first appearance of the levels 0..3 x every M0 state,
    one element each (320 elements, 1300 records, ten of them twice), as one
    owner step: the LDS path (k_rp_agg / k_rp_elems / k_rp_flags on the shared
    decision of csrc/decide.h; it runs at any size here) and the per-record
    path (exact).  A record is flagged iff the oracle's checkNewSignal sets its
    (call, element) bit; the shard and newSignal end as the oracle's, and the
    step reports the oracle's changed and inserted counts."""
    from syzkaller_amd import signal as S

    w = _case()
    shard = S.Serial(w["m0e"].copy(), w["m0p"].copy()).Deserialize(gpu.eng)
    ns = S.Signal.make(1 << 12, gpu.eng)
    status, flags, st = _own(gpu, w, shard, ns, exact)
    print(f"exact={exact}: status {status}, flagged {int(flags.sum())} / oracle {int(w['new'].sum())}, "
          f"changed {st['changed']} / {w['changed']}, inserted {st['inserted']} / {w['inserted']}, "
          f"own_parts {st['own_parts']}")
    assert status == 0 and not st["owners_void"] and not st["global_void"], st
    assert st["received"] == w["rec"].size
    assert (st["own_parts"] > 0) == (not exact), st  # the LDS path reports its partitions
    np.testing.assert_array_equal(flags, w["new"])
    _same(shard, *w["max"], gpu.eng)
    _same(ns, *w["newsig"], gpu.eng)
    assert st["changed"] == w["changed"] and st["inserted"] == w["inserted"], st


def test_step_own_staircase_gated(gpu):
    """The same step with every partition reported over capacity
    (SYZSIG_DEBUG_RECS_GATE): status 2, no flag, and the shard and newSignal
    serialize exactly as before the call (a Serial's order is the table's, as
    Go's is the map's, and the step's reservation may grow the table: the
    entries are compared in element order)."""
    from syzkaller_amd import signal as S
    from syzkaller_amd._lib import SYZSIG_DEBUG_RECS_GATE

    w = _case()
    shard = S.Serial(w["m0e"].copy(), w["m0p"].copy()).Deserialize(gpu.eng)
    ns = S.Signal.make(1 << 12, gpu.eng)
    before = _entries(shard), _entries(ns)
    gpu.eng.set_debug(SYZSIG_DEBUG_RECS_GATE)
    try:
        status, flags, st = _own(gpu, w, shard, ns, False)
    finally:
        gpu.eng.set_debug(0)
    assert status == 2 and not flags.any(), (status, int(flags.sum()))
    assert st["changed"] == 0 and st["inserted"] == 0, st
    for got, was in zip((_entries(shard), _entries(ns)), before):
        np.testing.assert_array_equal(got[0], was[0])
        np.testing.assert_array_equal(got[1], was[1])
    assert shard.Len() == w["m0e"].size and ns.Len() == 0
