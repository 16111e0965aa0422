"""Hand-derived Save / Delete sequences for pkg/db's write side (db.go:55-74):
per case the database's records before, the ops in order, the indices of the
ops that reach the log, and the records afterwards in file order of the last
write.  Every expectation is worked out by hand from db.go, none by running
code.  A key is hash.String's form of a 20-byte Sig; seq ^0 makes an op a
Delete.  Below them the Flush / compact / BumpVersion cases."""
DEL = (1 << 64) - 1


def key(i):
    """a Sig whose bytes are all i, as the 40 hex characters of hash.String"""
    return (b"%02x" % i) * 20


KA, KB, KC = key(0xA1), key(0xB2), key(0xC3)

# name: (live [(key, val, seq)], ops [(key, val, seq)], written op indices, records after [(key, val, seq)])
APPLY = {
    # the same (key, val, seq) twice in one batch: the second Save sees the first (:59-61)
    "same_twice": ([], [(KA, b"prog", 0), (KA, b"prog", 0)], [0], [(KA, b"prog", 0)]),
    # the same value with another seq is a change
    "same_val_other_seq": ([], [(KA, b"prog", 0), (KA, b"prog", 1)], [0, 1], [(KA, b"prog", 1)]),
    "save_delete_save": ([], [(KA, b"v", 3), (KA, b"", DEL), (KA, b"v", 3)], [0, 1, 2], [(KA, b"v", 3)]),
    "delete_absent": ([(KB, b"b", 1)], [(KA, b"", DEL)], [], [(KB, b"b", 1)]),
    "delete_twice": ([(KA, b"a", 1), (KB, b"b", 1)], [(KA, b"", DEL), (KA, b"", DEL)], [0], [(KB, b"b", 1)]),
    # a Save equal to the database's record: nothing, and the record keeps its place
    "save_equal_to_db": ([(KA, b"a", 1), (KB, b"b", 2)], [(KA, b"a", 1)], [], [(KA, b"a", 1), (KB, b"b", 2)]),
    # ... and a changed one moves behind the others, as the log's replay has it
    "save_changed_moves_last": ([(KA, b"a", 1), (KB, b"b", 2)], [(KA, b"a2", 1)], [0], [(KB, b"b", 2), (KA, b"a2", 1)]),
    "last_byte_differs": ([(KA, b"abcdefgh", 5)], [(KA, b"abcdefgX", 5)], [0], [(KA, b"abcdefgX", 5)]),
    "length_differs_by_one": ([(KA, b"abcdefgh", 5)], [(KA, b"abcdefg", 5), (KA, b"abcdefgh", 5), (KA, b"abcdefghi", 5)],
                              [0, 1, 2], [(KA, b"abcdefghi", 5)]),
    # Save(sig, nil, 0) twice (syz-hub/state/state.go:335): one record of 60 bytes
    "nil_value_twice": ([], [(KA, b"", 0), (KA, b"", 0)], [0], [(KA, b"", 0)]),
    "empty_over_nonempty": ([(KA, b"prog", 0)], [(KA, b"", 0)], [0], [(KA, b"", 0)]),
    "nonempty_over_empty": ([(KA, b"", 0)], [(KA, b"prog", 0)], [0], [(KA, b"prog", 0)]),
    # a no-op Save after a written one does not take the record's place in the order
    "noop_after_write_keeps_order": ([(KA, b"a", 1)], [(KB, b"b", 1), (KA, b"a", 1)], [0], [(KA, b"a", 1), (KB, b"b", 1)]),
    # a Delete between two equal Saves makes the second one a change again; other keys interleaved
    "interleaved": ([(KA, b"a", 1), (KB, b"b", 1)],
                    [(KC, b"c", 1), (KA, b"", DEL), (KB, b"b", 1), (KA, b"a", 1), (KC, b"c", 1), (KB, b"", DEL), (KB, b"", DEL)],
                    [0, 1, 3, 5], [(KC, b"c", 1), (KA, b"a", 1)]),
    # a delete at the tail of a run of no-ops: the key is gone
    "delete_last": ([(KA, b"a", 1)], [(KA, b"a", 1), (KA, b"", DEL)], [1], []),
    "only_noop_deletes": ([], [(KA, b"", DEL), (KB, b"", DEL), (KA, b"", DEL)], [], []),
}


def boundary_db(n, unc):
    """n records and `unc` records in the file: db.go:77's uncompacted / 10 * 9 > len(Records)"""
    return [(key(i), b"v%d" % i, i) for i in range(n)], unc


# (len(Records), uncompacted) -> does Flush compact?  20 / 10 * 9 = 18
FLUSH_BOUNDARY = [(18, 20, False), (17, 20, True), (18, 29, False), (18, 30, True), (9, 10, False), (8, 10, True),
                  (0, 9, False), (0, 10, True), (0, 0, False)]
