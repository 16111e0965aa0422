"""CPU: the restated Manager.NewInput loop (tests/corpus_ref.py) on hand-derived
cases with their own numbers, and the library's side of the new entry point
that needs no GPU (the exported symbol, the ABI version)."""
import os
import re
import subprocess

import pytest

from oracle import oracle as O
from tests import corpus_ref as R
from tests.conftest import ROOT


def _manager(sig0, cov0):
    mgr = R.Manager(O.deserialize(*R.ser(sig0)) if sig0 is not None else None)
    if cov0 is not None:
        mgr.corpusCover.Merge(cov0)
    return mgr


@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_hand_derived_cases(case):
    _, sig0, cov0, rows, acc, new, entries, sig1, cov1 = case
    mgr = _manager(sig0, cov0)
    got_acc, got_new, got_entries = R.new_input_batch(mgr, rows)
    assert got_acc.tolist() == acc
    assert got_new.tolist() == new
    assert got_entries == entries
    if sig1 is None:
        assert mgr.corpusSignal.is_nil()
    else:
        assert not mgr.corpusSignal.is_nil() and mgr.corpusSignal.to_dict() == sig1
    if cov1 is None:
        assert mgr.corpusCover.c is None
    else:
        assert mgr.corpusCover.c is not None and mgr.corpusCover.c == cov1


def test_rejected_input_reaches_nothing():
    """Equal prio is rejected, and nothing of the rejected input reaches
    corpusSignal, corpusCover or its key."""
    mgr = _manager([(5, 2), (6, 1)], [100])
    acc, new, entries = R.new_input_batch(mgr, [(4, R.ser([(5, 2), (6, 1), (6, 0)]), [300], False)])
    assert acc.tolist() == [0] and new.tolist() == [0] and entries == {}
    assert mgr.corpusSignal.to_dict() == {5: 2, 6: 1} and mgr.corpusCover.c == {100} and 4 not in mgr.corpus


def test_nil_sets_stay_nil_when_nothing_is_accepted():
    mgr = _manager(None, None)
    acc, _, _ = R.new_input_batch(mgr, [(0, R.ser([]), [1], False), (0, R.ser([(1, 1)]), [2], True)])
    assert acc.tolist() == [0, 1]  # (the present row is accepted for its key's merge only)
    assert mgr.corpusSignal.is_nil() and mgr.corpusCover.c is None


def test_library_exports_new_input_and_abi_7():
    from syzkaller_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (syzsig_\w+)", out))
    assert {"syzsig_manager_new_input_batch", "syzsig_new_input_stats"} <= exported
    assert "syzsig_manager_new_input_batch" in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "syzsig.h")).read()
    assert int(re.search(r"#define SYZSIG_ABI_VERSION (\d+)", hdr).group(1)) == 7
    assert _lib.lib().syzsig_abi_version() == 7
    assert int(re.search(r"#define SYZSIG_CORPUS_TILE (\d+)", hdr).group(1)) == _lib.SYZSIG_CORPUS_TILE
    assert int(re.search(r"#define SYZSIG_INPUT_PRESENT (\d+)u", hdr).group(1)) == _lib.SYZSIG_INPUT_PRESENT
