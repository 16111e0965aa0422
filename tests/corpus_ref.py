"""syz-manager/manager.go:976-1025 Manager.NewInput restated line by line over
the oracle's Signal and Cover ops (oracle.OSig / oracle.OCover), one input
after the other, as oracle.poll restates Manager.Poll.  Test infrastructure:
the expectation for syzsig_manager_new_input_batch (csrc/corpus.hip).

A row is (key, (elems, prios), cover, present): key stands for
hash.String(a.Prog) (:999), (elems, prios) is a.Signal, cover is a.Cover.  A
`present` row is not an RPC: it is mgr.corpus[sig] as it was before the batch
(its stored Signal and Cover), handed over so that :1000-1008 can merge into it.
Entries are compared as sets: a corpus entry is kept here as its Deserialized
Signal and its Cover as a set, which is what :1002-1007 make of it.
"""
import numpy as np

from oracle import oracle as O


class Manager:
    """The fields of Manager that NewInput touches."""

    def __init__(self, corpus_signal=None, corpus_cover=None):
        self.corpusSignal = corpus_signal if corpus_signal is not None else O.OSig()  # nil until a Merge
        self.corpusCover = corpus_cover if corpus_cover is not None else O.OCover()   # nil until a Merge
        self.corpus = {}  # sig -> [Signal as OSig, Cover as OCover]

    def put_present(self, key, serial, cover):
        """mgr.corpus[sig] from before the batch.  Should the key already hold
        an entry (a present row after its inputs), the two are merged: a
        present row counts as accepted for its key's merge."""
        sig = O.deserialize(*serial)
        if key in self.corpus:
            self.corpus[key][0].Merge(sig)
            self.corpus[key][1].Merge(cover)
            return
        cov = O.OCover()
        cov.Merge(cover)
        self.corpus[key] = [sig, cov]

    def NewInput(self, key, serial, cover):
        """Returns (accepted, new): accepted = the input passed :993,
        new = it took the else branch at :1009."""
        inputSignal = O.deserialize(*serial)                    # :977 (a later duplicate wins, signal.go:59-71)
        if self.corpusSignal.Diff(inputSignal).Len() == 0:      # :993 (Diff of an empty Signal is nil)
            return False, False                                 # :994
        self.corpusSignal.Merge(inputSignal)                    # :997
        self.corpusCover.Merge(cover)                           # :998 (allocates a nil Cover, cover.go:9-18)
        if key in self.corpus:                                  # :999-1000
            inp = self.corpus[key]
            inputSignal.Merge(inp[0])                           # :1002
            inp[0] = inputSignal                                # :1003
            inputCover = O.OCover()                             # :1004
            inputCover.Merge(inp[1].Serialize())                # :1005
            inputCover.Merge(cover)                             # :1006
            inp[1] = inputCover                                 # :1007
            self.corpus[key] = inp                              # :1008 (Call and Prog stay the old entry's)
            return True, False
        cov = O.OCover()
        cov.Merge(cover)
        self.corpus[key] = [inputSignal, cov]                   # :1010 (saved and queued for the other fuzzers, :1011-1022)
        return True, True


def new_input_batch(mgr, rows):
    """The rows in arrival order.  Returns (accepted, new_key, entries):
    uint8 arrays over the rows (a present row: accepted 1, new_key 0) and
    {key: (Signal as dict, Cover as set)} for every key an accepted input
    touched."""
    accepted = np.zeros(len(rows), np.uint8)
    new_key = np.zeros(len(rows), np.uint8)
    touched = set()
    for i, row in enumerate(rows):
        key, serial, cover = row[0], row[1], row[2]
        if len(row) > 3 and row[3]:
            mgr.put_present(key, serial, cover)
            accepted[i] = 1
            continue
        acc, new = mgr.NewInput(key, serial, cover)
        accepted[i], new_key[i] = acc, new
        if acc:
            touched.add(key)
    entries = {k: (mgr.corpus[k][0].to_dict(), set(mgr.corpus[k][1].Serialize())) for k in touched}
    return accepted, new_key, entries


def ser(pairs):
    """[(elem, prio), ...] -> (elems u32[], prios i8[])"""
    return (np.array([e for e, _ in pairs], np.uint32), np.array([p for _, p in pairs], np.int8))


# Hand-derived cases: (name, corpusSignal before ([(e, p)] or None = nil), corpusCover before (list or None = nil),
# rows, expected accepted, expected new_key, expected entries, expected corpusSignal (None = nil), expected corpusCover)
HAND_CASES = [
    ("equal_prio_rejected_nothing_leaks",
     [(5, 2)], [100],
     [(0, ser([(5, 2), (6, 1)]), [200], False),     # 6 is new: accepted
      (1, ser([(5, 2), (6, 1)]), [300, 301], False)],  # equal prios everywhere: rejected, 300/301 go nowhere
     [1, 0], [1, 0], {0: ({5: 2, 6: 1}, {200})}, {5: 2, 6: 1}, {100, 200}),
    ("later_duplicate_wins_then_lower_beats_corpus",
     [(7, 1)], [],
     [(0, ser([(7, 3), (7, 0)]), [1], False),       # Deserialize keeps (7,0): 0 <= 1, rejected
      (1, ser([(7, 2)]), [2], False)],              # 2 > 1 (the rejected 3 never reached corpusSignal): accepted
     [0, 1], [0, 1], {1: ({7: 2}, {2})}, {7: 2}, {2}),
    ("two_identical_inputs",
     None, None,
     [(0, ser([(9, 0), (10, -1)]), [5, 5, 4], False),
      (1, ser([(9, 0), (10, -1)]), [6], False)],
     [1, 0], [1, 0], {0: ({9: 0, 10: -1}, {4, 5})}, {9: 0, 10: -1}, {4, 5}),
    ("int8_min_on_absent_element",
     [(1, 0)], None,
     [(0, ser([(2, -128)]), [], False)],
     [1], [1], {0: ({2: -128}, set())}, {1: 0, 2: -128}, set()),
    ("empty_serial_rejected",
     None, None,
     [(0, ser([]), [7, 8], False)],
     [0], [0], {}, None, None),
    ("same_key_twice_max_merge_and_union",
     None, None,
     [(3, ser([(1, 1), (2, 4)]), [10, 11], False),
      (3, ser([(1, 3), (2, 0), (4, -2)]), [11, 12], False)],  # 1 rises, 4 is new: accepted; 2 keeps its max 4
     [1, 1], [1, 0], {3: ({1: 3, 2: 4, 4: -2}, {10, 11, 12})}, {1: 3, 2: 4, 4: -2}, {10, 11, 12}),
    ("present_row_merges_but_stays_out_of_corpus_sets",
     [(1, 0)], [50],
     [(0, ser([(1, 4), (8, 2)]), [60, 61], True),   # the old entry: not in corpusSignal / corpusCover
      (0, ser([(1, 2), (9, 1)]), [62], False),      # 1: 2 > 0 accepted (the present row's 4 plays no part); not new
      (1, ser([(8, 3)]), [63], False)],             # 8 absent from corpusSignal: accepted and new
     [1, 1, 1], [0, 0, 1], {0: ({1: 4, 8: 2, 9: 1}, {60, 61, 62}), 1: ({8: 3}, {63})},
     {1: 2, 9: 1, 8: 3}, {50, 62, 63}),
    ("present_row_alone_touches_nothing",
     [(1, 0)], [50],
     [(0, ser([(1, 4)]), [60], True), (0, ser([(1, 0)]), [61], False)],
     [1, 0], [0, 0], {}, {1: 0}, {50}),
    ("nil_sets_accepted_empty_cover",
     None, None,
     [(0, ser([(3, 1)]), [], False)],
     [1], [1], {0: ({3: 1}, set())}, {3: 1}, set()),   # corpusCover: non-nil and empty
]
