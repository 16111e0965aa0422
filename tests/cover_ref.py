"""Restatement of the cover half of the per-execution path, the checker of
syzsig_edge_cover_dev and syzsig_triage_cover_dev.

call_cover / edge_cover are pinned to the compiled reference: the harness
(oracle/ref_harness.cc, cover mode) runs the reference's own
write_coverage_signal with flag_collect_cover on, both values of
flag_dedup_cover, and tests/test_golden_cover_comps_cpu.py holds this file
word for word to what it wrote (tests/golden/cover, and a live run on fresh
traces where the harness is built).  triage_cover restates Go (proc.go, no Go
toolchain) and stays restatement-only; tests/test_cover_ref_cpu.py holds it to
hand-derived cases.

  call_cover / edge_cover   executor/executor.h:514-527
  triage_cover              syz-fuzzer/proc.go:119-139 and :173
"""
import numpy as np

from oracle import oracle as O


def call_cover(pcs, dedup=True):
    """One completed call's cover output: executor.h:518-522 std::sort +
    std::unique over the u64 PCs with flag_dedup_cover, then :525-526 the
    truncation to u32."""
    pcs = np.asarray(pcs, np.uint64)
    if dedup:
        pcs = np.unique(pcs)
    return pcs.astype(np.uint32)


def edge_cover(pcs, call_start, call_len, prog_call, completed, dedup=True, fill=0):
    """Every call of a batch.  Call c of program p has a cover record iff
    c - prog_call[p] < completed[p]: the aborting call and the later ones exit
    in the signal loop (executor.h:502-503), before :514.  Returns (cover
    u32[npc] in pcs indexing, `fill` wherever nothing is written, cover_cnt)."""
    pcs = np.asarray(pcs, np.uint64)
    cover = np.full(pcs.size, fill, np.uint32)
    cnt = np.zeros(len(call_len), np.uint32)
    for p in range(len(prog_call) - 1):
        cb = int(prog_call[p])
        for c in range(cb, min(int(prog_call[p + 1]), cb + int(completed[p]))):
            s, n = int(call_start[c]), int(call_len[c])
            out = call_cover(pcs[s:s + n], dedup)
            cover[s:s + out.size] = out
            cnt[c] = out.size
    return cover, cnt


def triage_cover(item_off, elems, prios, item_flags, runs, run_off, run_sigs, run_prio, run_errno, run_exec,
                 run_cover):
    """proc.go:107-140 and :173 per item, the loop written out: run_cover[r] is
    inf.Cover of run r = i * runs + k (any u32 array).  Returns (item_keep
    u8[], covers): covers[i] = RPCInput.Cover of item i as a sorted u32 array
    (Go's Serialize order is map order; sorted is the fixed one), empty for an
    item that took one of the loop's returns."""
    keep, covers = [], []
    for i in range(len(item_off) - 1):
        a, b = int(item_off[i]), int(item_off[i + 1])
        new_signal = O.deserialize(elems[a:b], prios[a:b])
        minimized, orig_ok = bool(item_flags[i] & 1), bool(item_flags[i] & 2)
        input_cover = set()                                   # :113 var inputCover cover.Cover
        returned = new_signal.Len() == 0                      # :109-111
        notexecuted = 0                                       # :119
        for k in range(runs):                                 # :120
            if returned:
                break
            r = i * runs + k
            ra, rb = int(run_off[r]), int(run_off[r + 1])
            if not run_exec[r] or rb == ra or (orig_ok and run_errno[r] != 0):  # :122-123
                notexecuted += 1                              # :125
                if notexecuted > runs // 2 + 1:               # :126
                    returned = True                           # :127
                continue                                      # :129
            this_signal = O.from_raw(run_sigs[ra:rb], int(run_prio[r]))  # :132
            new_signal = new_signal.Intersection(this_signal)            # :133
            if new_signal.Len() == 0 and not minimized:       # :136
                returned = True                               # :137
                continue
            input_cover.update(int(x) for x in np.asarray(run_cover[r], np.uint32))  # :139
        keep.append(int(not returned))
        covers.append(np.array(sorted(input_cover) if not returned else [], np.uint32))  # :173
    return np.array(keep, np.uint8), covers
