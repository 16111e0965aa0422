"""CPU: tests/cover_ref.py -- the restatement that checks the device cover
path -- against cases derived by hand from the reference lines they cite
(executor/executor.h:514-527, syz-fuzzer/proc.go:119-139 and :173)."""
import numpy as np

from oracle import oracle as O
from tests import cover_ref as CR

B = 0xffffffff81000000


def test_executor_kat_trace():
    # the executor KAT trace of SURVEY.md: {...10, ...20, ...10, ...20, ...30}
    pcs = np.array([B + 0x10, B + 0x20, B + 0x10, B + 0x20, B + 0x30], np.uint64)
    # executor.h:518-522 sort + unique, :525-526 truncation
    assert CR.call_cover(pcs, dedup=True).tolist() == [0x81000010, 0x81000020, 0x81000030]
    # :525-527 alone: the five PCs truncated in trace order
    assert CR.call_cover(pcs, dedup=False).tolist() == [0x81000010, 0x81000020, 0x81000010, 0x81000020, 0x81000030]
    cover, cnt = CR.edge_cover(pcs, [0], [5], [0, 1], [1], dedup=True, fill=0xdeadbeef)
    assert cnt.tolist() == [3]  # :527 *cover_count_pos = cover_size
    assert cover.tolist() == [0x81000010, 0x81000020, 0x81000030, 0xdeadbeef, 0xdeadbeef]


def test_sort_is_u64_order_truncated():
    # low words on both sides of 2^31 .. the end of cover_check's range: the
    # u64 order of PCs with the upper word 0xffffffff is their low words' order
    pcs = np.array([0xfffffffffeffffff, 0xffffffff80000000, 0xffffffffc0000000, 0xffffffff80000000], np.uint64)
    assert CR.call_cover(pcs).tolist() == [0x80000000, 0xc0000000, 0xfeffffff]


def test_abort_at_call_2():
    # executor.h:502-503: a PC failing cover_check exits inside the signal loop of
    # call 2, before :514 of that call; calls 0-1 were complete, 3 never ran
    lens = np.array([3, 2, 4, 2], np.uint32)
    start = np.array([0, 3, 5, 9], np.uint64)
    pcs = np.array([B + 5, B + 1, B + 5,  B + 9, B + 9,  B + 2, 0x1000, B + 3, B + 4,  B + 7, B + 6], np.uint64)
    prog_call = np.array([0, 4], np.uint32)
    _, _, completed = O.exec_batch(pcs, start, lens, prog_call)
    assert completed.tolist() == [2]
    cover, cnt = CR.edge_cover(pcs, start, lens, prog_call, completed, dedup=True, fill=7)
    assert cnt.tolist() == [2, 1, 0, 0]
    assert cover.tolist() == [0x81000001, 0x81000005, 7, 0x81000009, 7, 7, 7, 7, 7, 7, 7]
    cover, cnt = CR.edge_cover(pcs, start, lens, prog_call, completed, dedup=False, fill=7)
    assert cnt.tolist() == [3, 2, 0, 0]
    assert cover.tolist() == [0x81000005, 0x81000001, 0x81000005, 0x81000009, 0x81000009, 7, 7, 7, 7, 7, 7]


def _item(flags, new_signal, runs):
    """One item: runs = [(sig list, prio, errno, exec, cover list)]."""
    run_off = np.cumsum([0] + [len(r[0]) for r in runs]).astype(np.uint64)
    sigs = np.array([x for r in runs for x in r[0]], np.uint32)
    keep, covers = CR.triage_cover(
        np.array([0, len(new_signal)], np.uint64), np.array(new_signal, np.uint32), np.zeros(len(new_signal), np.int8),
        np.array([flags], np.uint8), len(runs), run_off, sigs, np.array([r[1] for r in runs], np.uint8),
        np.array([r[2] for r in runs], np.int32), np.array([r[3] for r in runs], np.uint8),
        [np.array(r[4], np.uint32) for r in runs])
    return int(keep[0]), covers[0].tolist()


MIN, ORIG_OK = 1, 2


def test_item_all_runs_merge():
    # no skip, no return: :139 three times, :173 the union (sorted here)
    assert _item(0, [1, 2], [([1, 2], 0, 0, 1, [30, 10]), ([2, 1, 9], 0, 0, 1, [10, 20]),
                             ([1, 2], 0, 0, 1, [40])]) == (1, [10, 20, 30, 40])


def test_item_skip_not_executed():
    # :122 len(info) == 0 -> :125-129 continue before :139; 1 skip <= 3/2+1
    assert _item(0, [1], [([1], 0, 0, 1, [10]), ([1], 0, 0, 0, [66]), ([1], 0, 0, 1, [20])]) == (1, [10, 20])


def test_item_skip_empty_signal():
    # :122 len(info[item.call].Signal) == 0
    assert _item(0, [1], [([], 0, 0, 1, [66]), ([1], 0, 0, 1, [10]), ([1], 0, 0, 1, [5])]) == (1, [5, 10])


def test_item_skip_failed_after_ok():
    # :123 item.info.Errno == 0 && info[item.call].Errno != 0
    assert _item(ORIG_OK, [1], [([1], 0, 0, 1, [10]), ([1], 0, 22, 1, [66]), ([1], 0, 0, 1, [20])]) == (1, [10, 20])
    # the original failed too: the run is not skipped
    assert _item(0, [1], [([1], 0, 0, 1, [10]), ([1], 0, 22, 1, [66]), ([1], 0, 0, 1, [20])]) == (1, [10, 20, 66])


def test_item_give_up_rule():
    # :126 notexecuted > signalRuns/2+1: with 3 runs that is > 2 -- two skips
    # go on, the third returns (:127) and the item never reaches :173
    assert _item(0, [1], [([1], 0, 0, 0, [66]), ([1], 0, 0, 0, [66]), ([1], 0, 0, 1, [10])]) == (1, [10])
    assert _item(0, [1], [([1], 0, 0, 0, [66]), ([1], 0, 0, 0, [66]), ([1], 0, 0, 0, [66])]) == (0, [])
    # 8 runs: 8/2+1 = 5 skips go on, the sixth returns
    run, skip = ([1], 0, 0, 1, [10]), ([1], 0, 0, 0, [66])
    assert _item(0, [1], [skip] * 5 + [run] * 3) == (1, [10])
    assert _item(0, [1], [skip] * 6 + [run] * 2) == (0, [])


def test_item_emptied_in_run_2_not_minimized():
    # :133 newSignal empties in the second run, :136-137 return before :139
    # of that run and before :173: no cover at all
    assert _item(0, [1], [([1], 0, 0, 1, [10]), ([2], 0, 0, 1, [20]), ([1], 0, 0, 1, [30])]) == (0, [])


def test_item_emptied_in_run_1_minimized():
    # ProgMinimized: :136 does not return, so :139 runs for runs 1-3
    assert _item(MIN, [1], [([2], 0, 0, 1, [10]), ([1], 0, 0, 1, [20]), ([3], 0, 0, 1, [30, 10])]) == (1, [10, 20, 30])


def test_item_intersection_needs_prio():
    # signal.go:104-115: e stays iff the run's prio >= e's; newSignal prio 0,
    # run prio 0 keeps it -- and the empty newSignal of :109-111 returns at once
    assert _item(0, [], [([1], 0, 0, 1, [10])] * 3) == (0, [])
