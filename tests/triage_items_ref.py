"""The reference loops that syzsig_triage_items_dev and
syzsig_corpus_add_inputs_dev replace, restated line by line over the oracle's
own Signal ops (no GPU use).

triage_items: syz-fuzzer/proc.go:230-247 (execute enqueues one WorkTriage per
call checkNewSignal returned, in call order) followed by the head of
triageInput, proc.go:107-111, for each item -- every item against the same
corpusSignal, the interleaving in which all Procs reach :108 before any
reaches :176.
add_inputs: syz-fuzzer/fuzzer.go:446-460 addInputToCorpus, item after item.
"""
import numpy as np

from oracle import oracle as O


def _sorted_serial(sig):
    """Serialize (signal.go:42-57) in ascending element order: one fixed
    instance of the map's iteration order."""
    e, p = sig.Serialize()
    o = np.argsort(e, kind="stable")
    return e[o], p[o]


def triage_items(corpus_signal, sigs, call_start, call_len, call_prio, call_new):
    """corpus_signal: an OSig (a nil one is Go's nil corpusSignal).  Returns a
    dict of item_call u32[n], item_prio i8[n], input_off u64[n + 1],
    input_elems u32[], item_off u64[n + 1], elems u32[], prios i8[]."""
    sigs = np.asarray(sigs, np.uint32)
    item_call, item_prio, inputs, news = [], [], [], []
    for c in range(len(call_len)):  # proc.go:232: range over checkNewSignal's calls, ascending
        if not call_new[c]:  # fuzzer.go:498-503: the call is not in `calls`
            continue
        raw = sigs[int(call_start[c]):int(call_start[c]) + int(call_len[c])]  # proc.go:233-235 info.Signal
        prio = int(call_prio[c])  # signalPrio(...), fuzzer.go:513-521, as the batch carries it
        input_signal = O.from_raw(raw, prio)  # proc.go:107 (signal.go:35 casts the prio to int8)
        new_signal = corpus_signal.Diff(input_signal)  # proc.go:108, fuzzer.go:486-490
        # proc.go:109-111 `if newSignal.Empty() { return }`: the item keeps an empty range
        item_call.append(c)
        item_prio.append(np.array(prio & 0xFF, np.uint8).view(np.int8))
        inputs.append(_sorted_serial(input_signal))
        news.append(_sorted_serial(new_signal))
        assert (inputs[-1][1] == item_prio[-1]).all() and (news[-1][1] == item_prio[-1]).all()  # FromRaw: one prio

    def cat(parts, dt):
        return np.concatenate(parts).astype(dt) if parts else np.empty(0, dt)

    return {"item_call": np.array(item_call, np.uint32), "item_prio": np.array(item_prio, np.int8),
            "input_off": np.cumsum([0] + [e.size for e, _ in inputs]).astype(np.uint64),
            "input_elems": cat([e for e, _ in inputs], np.uint32),
            "input_prios": cat([p for _, p in inputs], np.int8),
            "item_off": np.cumsum([0] + [e.size for e, _ in news]).astype(np.uint64),
            "elems": cat([e for e, _ in news], np.uint32), "prios": cat([p for _, p in news], np.int8)}


def add_inputs(corpus_signal, max_signal, input_off, input_elems, item_prio, item_keep=None):
    """fuzzer.go:446-460 for item after item; corpus_signal / max_signal are
    OSig objects changed in place (a nil one is allocated by its first Merge,
    signal.go:121-125)."""
    for i in range(len(item_prio)):
        if item_keep is not None and not item_keep[i]:  # triageInput returned before proc.go:176
            continue
        a, b = int(input_off[i]), int(input_off[i + 1])
        sign = O.deserialize(input_elems[a:b], np.full(b - a, item_prio[i], np.int8))  # the item's inputSignal
        if sign.Len() != 0:  # fuzzer.go:454 `if !sign.Empty()`
            corpus_signal.Merge(sign)  # fuzzer.go:456
            max_signal.Merge(sign)  # fuzzer.go:457
