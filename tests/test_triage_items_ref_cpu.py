"""CPU: tests/triage_items_ref.py (the restated proc.go:107-111, :232-245 and
fuzzer.go:446-460) on hand-derived cases, each with its own expected numbers,
and the SYZSIG_ITEMS_TILE constant of the header against _lib's."""
import os
import re

import numpy as np

from oracle import oracle as O
from syzkaller_amd import _lib
from tests import triage_items_ref as R
from tests.conftest import ROOT


def _batch(calls):
    """calls = [(records, prio, flagged), ...] -> sigs, start, len, prio, new,
    with three unused records between calls"""
    sigs, start, ln, prio, new = [], [], [], [], []
    for rec, p, f in calls:
        sigs += [0xdead] * 3
        start.append(len(sigs))
        sigs += list(rec)
        ln.append(len(rec))
        prio.append(p)
        new.append(f)
    return (np.array(sigs, np.uint32), np.array(start, np.uint64), np.array(ln, np.uint32), np.array(prio, np.uint8),
            np.array(new, np.uint8))


def _corpus(d):
    return O.deserialize(np.array(list(d), np.uint32), np.array(list(d.values()), np.int8)) if d else O.OSig()


def _item(r, i):
    a, b, c, d = (int(x) for x in (r["input_off"][i], r["input_off"][i + 1], r["item_off"][i], r["item_off"][i + 1]))
    return r["input_elems"][a:b].tolist(), r["elems"][c:d].tolist(), r["prios"][c:d].tolist()


def test_duplicates_collapse_and_order_is_call_order():
    r = R.triage_items(O.OSig(), *_batch([([9, 3, 9, 9, 3, 7], 2, 1), ([5, 5], 1, 0), ([4, 1, 4], 0, 7)]))
    assert r["item_call"].tolist() == [0, 2] and r["item_prio"].tolist() == [2, 0]
    assert r["input_off"].tolist() == [0, 3, 5] and r["item_off"].tolist() == [0, 3, 5]
    assert _item(r, 0) == ([3, 7, 9], [3, 7, 9], [2, 2, 2])  # nil corpusSignal: everything is new
    assert _item(r, 1) == ([1, 4], [1, 4], [0, 0])


def test_equal_prio_is_not_new_greater_is():
    corpus = _corpus({10: 1, 11: 2, 12: 0})
    r = R.triage_items(corpus, *_batch([([10, 11, 12, 13], 1, 1)]))
    # 10: corpus 1 >= 1 known; 11: 2 >= 1 known; 12: 0 < 1 new; 13: absent new
    assert _item(r, 0) == ([10, 11, 12, 13], [12, 13], [1, 1])


def test_corpus_prio_extremes_against_item_prios():
    corpus = _corpus({100: -128, 200: 127})
    for p in range(4):
        r = R.triage_items(corpus, *_batch([([200, 100], p, 1)]))
        assert _item(r, 0) == ([100, 200], [100], [p])  # -128 < p <= 127


def test_call_prio_cast_to_int8():
    corpus = _corpus({1: -128, 2: -127, 3: -1, 4: 0, 5: -2})
    r = R.triage_items(corpus, *_batch([([1, 2, 3, 4, 5, 6], 0x80, 1), ([1, 2, 3, 4, 5, 6], 0xff, 1)]))
    assert r["item_prio"].tolist() == [-128, -1]
    # prio -128 loses to every corpus entry (all >= -128); only the absent 6 is new
    assert _item(r, 0) == ([1, 2, 3, 4, 5, 6], [6], [-128])
    # prio -1: known where corpus >= -1 (3: -1, 4: 0); new where below (1, 2, 5) or absent (6)
    assert _item(r, 1) == ([1, 2, 3, 4, 5, 6], [1, 2, 5, 6], [-1, -1, -1, -1])


def test_nothing_new_and_flagged_empty_call():
    corpus = _corpus({7: 3, 8: 3})
    r = R.triage_items(corpus, *_batch([([8, 7, 8], 3, 1), ([], 2, 1), ([7], 3, 0)]))
    assert r["item_call"].tolist() == [0, 1]
    assert r["input_off"].tolist() == [0, 2, 2] and r["item_off"].tolist() == [0, 0, 0]
    assert _item(r, 0) == ([7, 8], [], []) and _item(r, 1) == ([], [], [])


def test_every_item_diffs_against_the_corpus_as_passed_in():
    r = R.triage_items(O.OSig(), *_batch([([1, 2], 1, 1), ([2, 1], 1, 1)]))
    assert _item(r, 0) == ([1, 2], [1, 2], [1, 1]) and _item(r, 1) == ([1, 2], [1, 2], [1, 1])


def test_add_inputs_nil_receivers_and_max_merge():
    corpus, mx = O.OSig(), _corpus({1: 3, 2: 0})
    off, el, pr = np.array([0, 2, 2, 4], np.uint64), np.array([1, 2, 2, 3], np.uint32), np.array([1, 2, 2], np.int8)
    R.add_inputs(corpus, mx, off, el, pr)
    assert corpus.to_dict() == {1: 1, 2: 2, 3: 2} and mx.to_dict() == {1: 3, 2: 2, 3: 2}
    R.add_inputs(corpus, mx, off, el, np.array([0, 0, -5], np.int8))  # lower prios change nothing
    assert corpus.to_dict() == {1: 1, 2: 2, 3: 2} and mx.to_dict() == {1: 3, 2: 2, 3: 2}


def test_add_inputs_nothing_kept_leaves_nil_nil():
    off, el, pr = np.array([0, 2, 2], np.uint64), np.array([1, 2], np.uint32), np.array([1, 2], np.int8)
    corpus, mx = O.OSig(), O.OSig()
    R.add_inputs(corpus, mx, off, el, pr, np.array([0, 0], np.uint8))
    assert corpus.is_nil() and mx.is_nil()
    R.add_inputs(corpus, mx, off, el, pr, np.array([0, 1], np.uint8))  # the kept item's sign is empty: fuzzer.go:454
    assert corpus.is_nil() and mx.is_nil()
    R.add_inputs(corpus, mx, off, el, pr, np.array([5, 0], np.uint8))
    assert corpus.to_dict() == {1: 1, 2: 1} and mx.to_dict() == {1: 1, 2: 1}


def test_items_tile_of_header_and_lib_agree():
    txt = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    m = re.search(r"#define SYZSIG_ITEMS_TILE (\d+)", txt)
    assert m and int(m.group(1)) == _lib.SYZSIG_ITEMS_TILE
    t = _lib.SYZSIG_ITEMS_TILE
    assert t & (t - 1) == 0 and 256 <= t and 4 * t <= 64 * 1024  # items.hip's static_asserts
