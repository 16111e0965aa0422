"""Hand-derived cases for fileSet and the line walk (syz-manager/cover.go:129-193):
each expected result was worked out by hand from the Go text, not produced by
any implementation.

FILE_SET: (name, covered frames, uncovered frames, {file: nlines}, fileSet's
map, {file: (entries the walk consumes, Coverage)}).  A frame is (File, Line,
Func).  FILE_ORDER: (names, the names as sort.Sort(templateFileArray) leaves
them)."""

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

FILE_SET = [
    # line 7 is covered and also uncovered: files[a][7] is true when the second loop reads it, and stays
    ("covered_wins",
     [("a.c", 7, "f")], [("a.c", 7, "f"), ("a.c", 9, "f")], {"a.c": 20},
     {"a.c": [(7, True), (9, False)]}, {"a.c": (2, 1)}),
    # g has no covered frame: funcs[g] is false, its uncovered frame is skipped
    ("uncovered_func_dropped",
     [("a.c", 3, "f")], [("a.c", 4, "g"), ("a.c", 5, "f")], {"a.c": 10},
     {"a.c": [(3, True), (5, False)]}, {"a.c": (2, 1)}),
    # funcs is keyed by the name alone: static `init` covered in a.c keeps the uncovered frame of b.c's `init`
    ("same_name_other_file",
     [("a.c", 1, "init")], [("b.c", 2, "init")], {"a.c": 5, "b.c": 5},
     {"a.c": [(1, True)], "b.c": [(2, False)]}, {"a.c": (1, 1), "b.c": (1, 0)}),
    # an uncovered frame creates a file that has no covered line (an inlined callee's header)
    ("uncovered_creates_file",
     [("a.c", 10, "f")], [("inc.h", 30, "f"), ("inc.h", 31, "f")], {"a.c": 10, "inc.h": 30},
     {"a.c": [(10, True)], "inc.h": [(30, False), (31, False)]}, {"a.c": (1, 1), "inc.h": (1, 0)}),
    # repeats of one frame in both lists, in any order
    ("repeats",
     [("a.c", 2, "f"), ("a.c", 2, "f"), ("a.c", 1, "f"), ("a.c", 2, "f")],
     [("a.c", 3, "f"), ("a.c", 3, "f"), ("a.c", 2, "f"), ("a.c", 3, "f")], {"a.c": 3},
     {"a.c": [(1, True), (2, True), (3, False)]}, {"a.c": (3, 2)}),
    # addr2line's "?:0": line 0 sorts first, is never equal to i + 1, and blocks every entry behind it
    ("head_line_zero",
     [("a.c", 0, "f"), ("a.c", 1, "f"), ("a.c", 2, "f")], [("a.c", 3, "f")], {"a.c": 10},
     {"a.c": [(0, True), (1, True), (2, True), (3, False)]}, {"a.c": (0, 0)}),
    ("head_line_negative",
     [("a.c", 5, "f"), ("a.c", -4, "f")], [("a.c", 6, "f")], {"a.c": 10},
     {"a.c": [(-4, True), (5, True), (6, False)]}, {"a.c": (0, 0)}),
    # lines 4, 5, 6 against files of 5, 4 and 0 lines: line == nlines is consumed, nlines + 1 is not
    # and does not hide the entries before it
    ("line_at_nlines",
     [("a.c", 4, "f"), ("a.c", 5, "f"), ("a.c", 6, "f")], [], {"a.c": 5},
     {"a.c": [(4, True), (5, True), (6, True)]}, {"a.c": (2, 2)}),
    ("line_at_nlines_plus_one",
     [("a.c", 4, "f"), ("a.c", 5, "f"), ("a.c", 6, "f")], [], {"a.c": 4},
     {"a.c": [(4, True), (5, True), (6, True)]}, {"a.c": (1, 1)}),
    ("nlines_zero",
     [("a.c", 1, "f")], [("a.c", 2, "f")], {"a.c": 0},
     {"a.c": [(1, True), (2, False)]}, {"a.c": (0, 0)}),
    # Go's int orders signed: INT32_MIN first (and it blocks the walk), INT32_MAX last
    ("int32_extremes",
     [("a.c", I32_MAX, "f"), ("a.c", 1, "f")], [("a.c", I32_MIN, "f"), ("a.c", -1, "f")], {"a.c": 100},
     {"a.c": [(I32_MIN, False), (-1, False), (1, True), (I32_MAX, True)]}, {"a.c": (0, 0)}),
    ("int32_max_alone",
     [("a.c", 1, "f")], [("a.c", I32_MAX, "f")], {"a.c": 100},
     {"a.c": [(1, True), (I32_MAX, False)]}, {"a.c": (1, 1)}),
    # no covered frame: funcs is empty, every uncovered frame is dropped, the map is empty
    ("ncov_zero",
     [], [("a.c", 1, "f"), ("b.c", 2, "g")], {"a.c": 5, "b.c": 5},
     {}, {}),
    ("nunc_zero",
     [("b.c", 2, "g"), ("a.c", 1, "f"), ("b.c", 1, "g")], [], {"a.c": 5, "b.c": 1},
     {"a.c": [(1, True)], "b.c": [(1, True), (2, True)]}, {"a.c": (1, 1), "b.c": (1, 1)}),
    ("both_empty", [], [], {}, {}, {}),
]

FILE_ORDER = [
    (["b.c", "a.c"], ["a.c", "b.c"]),
    # include files (a leading '.') go below the others; among themselves '/' (0x2f) sorts before 'c'
    ([".config", "kernel/a.c", "./include/x.h", "arch/b.c"], ["arch/b.c", "kernel/a.c", "./include/x.h", ".config"]),
    # the empty name skips the '.' rule and compares as a string: below everything
    (["a", "", ".z"], ["", "a", ".z"]),
    (["", ".a"], ["", ".a"]),
    ([".b", "", "b", ".a", "a"], ["", "a", "b", ".a", ".b"]),
    ([], []),
]
