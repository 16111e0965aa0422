"""What the fuzzer does with the reply to its poll, restated line by line over
the oracle's own Signal ops (no GPU use): the loop syzsig_fuzzer_poll_res_dev
replaces.

syz-fuzzer/fuzzer.go:344-350 (the poll loop), :468-475 (addMaxSignal),
:433-444 (addInputFromAnotherFuzzer) and :446-460 (addInputToCorpus), segment
after segment in arrival order.  No Go toolchain is at hand, so this is a
restatement, pinned by the hand-derived cases of test_poll_res_ref_cpu.py.
"""
import numpy as np

from oracle import oracle as O

SEG_MAXSIGNAL = 0  # include/syzsig.h SYZSIG_SEG_MAXSIGNAL: r.MaxSignal
SEG_INPUT = 1  # SYZSIG_SEG_INPUT: the Signal of one of r.NewInputs


def add_max_signal(max_signal, sign):
    """fuzzer.go:468-475"""
    if sign.Len() == 0:  # :469-471
        return
    max_signal.Merge(sign)  # :474


def add_input_to_corpus(corpus_signal, max_signal, sign):
    """fuzzer.go:446-460 (the corpus list and its hashes, :447-452, carry no signal)"""
    if sign.Len() != 0:  # :454 `if !sign.Empty()`
        corpus_signal.Merge(sign)  # :456
        max_signal.Merge(sign)  # :457


def add_input_from_another_fuzzer(corpus_signal, max_signal, elems, prios):
    """fuzzer.go:433-444"""
    sign = O.deserialize(elems, prios)  # :442 inp.Signal.Deserialize()
    add_input_to_corpus(corpus_signal, max_signal, sign)  # :443


def poll_res(corpus_signal, max_signal, segments):
    """segments = [(kind, elems, prios)] in arrival order; corpus_signal /
    max_signal are OSig objects changed in place (a nil one is allocated by its
    first Merge, signal.go:121-125)."""
    for kind, elems, prios in segments:
        if kind == SEG_MAXSIGNAL:
            sign = O.deserialize(elems, prios)  # :344 maxSignal := r.MaxSignal.Deserialize()
            add_max_signal(max_signal, sign)  # :347
        elif kind == SEG_INPUT:
            add_input_from_another_fuzzer(corpus_signal, max_signal, elems, prios)  # :348-350
        else:
            raise ValueError("unknown segment kind")


def poll_res_raw_max(corpus_signal, max_signal, segments):
    """The WRONG rule, for tests that must tell it from the right one: a max
    over the raw entries, i.e. every entry merged on its own, as if Deserialize
    kept an element's highest prio instead of its last."""
    for kind, elems, prios in segments:
        for e, p in zip(np.asarray(elems, np.uint32).tolist(), np.asarray(prios, np.int8).tolist()):
            one = O.deserialize(np.array([e], np.uint32), np.array([p], np.int8))
            max_signal.Merge(one)
            if kind == SEG_INPUT:
                corpus_signal.Merge(one)

