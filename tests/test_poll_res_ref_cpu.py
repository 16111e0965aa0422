"""CPU: the restatement of the fuzzer's poll-reply loop (tests/poll_res_ref.py)
held to hand-derived cases, every number written out; and the LDS-hash helper
of the GPU tests (tests/pollres_keys.py)."""
import numpy as np

from oracle import oracle as O
from tests import poll_res_ref as R
from tests import pollres_keys as K

MS, IN = R.SEG_MAXSIGNAL, R.SEG_INPUT


def _seg(kind, pairs):
    return (kind, np.array([e for e, _ in pairs], np.uint32), np.array([p for _, p in pairs], np.int8))


def _run(c0, m0, segs, rule=R.poll_res):
    cs = O.deserialize(*zip(*c0)) if c0 is not None else O.OSig()
    ms = O.deserialize(*zip(*m0)) if m0 is not None else O.OSig()
    rule(cs, ms, segs)
    return cs, ms


def test_last_entry_wins_even_when_lower():
    # 7 appears with 3 and then with 1: Deserialize keeps 1 (signal.go:68), and 1 is merged
    cs, ms = _run(None, None, [_seg(IN, [(7, 3), (9, 2), (7, 1)])])
    assert cs.to_dict() == {7: 1, 9: 2} and ms.to_dict() == {7: 1, 9: 2}
    # the wrong rule (a max over the raw entries) gives 3: the two rules differ here
    cw, mw = _run(None, None, [_seg(IN, [(7, 3), (9, 2), (7, 1)])], R.poll_res_raw_max)
    assert cw.to_dict() == {7: 3, 9: 2} and mw.to_dict() == {7: 3, 9: 2}


def test_last_low_in_one_segment_high_in_another():
    # segment 0: 7 -> last is 0 (after a 4); segment 1: 7 -> 2.  Across segments the max: 2
    segs = [_seg(IN, [(7, 4), (7, 0)]), _seg(MS, [(7, 2)])]
    cs, ms = _run(None, None, segs)
    assert ms.to_dict() == {7: 2} and cs.to_dict() == {7: 0}
    cs, ms = _run(None, None, segs[::-1])  # and in the other order
    assert ms.to_dict() == {7: 2} and cs.to_dict() == {7: 0}


def test_int8_extremes_and_absent():
    # -128 against absent: absent is below every int8, so -128 is inserted; 127 stays over anything
    cs, ms = _run(None, [(5, 127)], [_seg(IN, [(4, -128), (5, -128), (6, 127)])])
    assert ms.to_dict() == {4: -128, 5: 127, 6: 127} and ms.Len() == 3
    assert cs.to_dict() == {4: -128, 5: -128, 6: 127}
    # -128 already there, -127 arrives: raised
    _, ms = _run(None, [(4, -128)], [_seg(MS, [(4, -127)])])
    assert ms.to_dict() == {4: -127}


def test_empty_segments_leave_nil_receivers_nil():
    cs, ms = _run(None, None, [_seg(MS, []), _seg(IN, [])])
    assert cs.is_nil() and ms.is_nil()


def test_maxsignal_segment_never_reaches_corpus_signal():
    cs, ms = _run(None, None, [_seg(MS, [(1, 1), (2, 2)])])
    assert cs.is_nil() and ms.to_dict() == {1: 1, 2: 2}
    cs, ms = _run([(3, 0)], [(3, 0)], [_seg(MS, [(3, 2)]), _seg(IN, [(4, 1)])])
    assert cs.to_dict() == {3: 0, 4: 1} and ms.to_dict() == {3: 2, 4: 1}


def test_equal_prio_changes_nothing_lower_neither():
    cs, ms = _run([(1, 2), (2, 2)], [(1, 2), (2, 3)], [_seg(IN, [(1, 2), (2, 1)])])
    assert cs.to_dict() == {1: 2, 2: 2} and ms.to_dict() == {1: 2, 2: 3}
    assert cs.Len() == 2 and ms.Len() == 2


def test_lds_home_helper():
    # (1 * 0x9E3779B1) >> 19 = 0x13C6; (2 * 0x9E3779B1 mod 2^32 = 0x3C6EF362) >> 19 = 0x78D
    assert K.lds_home(np.array([0, 1, 2], np.uint32)).tolist() == [0, 0x13C6, 0x78D]
    e = K.same_home(5, K.TILE // 2)
    assert e.size == K.TILE // 2 and np.unique(e).size == e.size and (K.lds_home(e) == 5).all()
    e = K.same_home(K.SLOTS - 1, 40)
    assert (K.lds_home(e) == K.SLOTS - 1).all()
