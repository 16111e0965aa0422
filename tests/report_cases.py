"""Hand-derived cases of the coverage-report loops, shared by
tests/test_report_ref_cpu.py (the Python restatement) and
tests/test_gpu_report.py (the device).  Every expected value below was worked
out by hand from the Go source, step by step in the comments; none comes from
running either implementation."""

M64 = (1 << 64) - 1

# (name, symbols sorted by start [(start, end)], allCoverPCs ascending, pcs in loop order, expected keys ascending)
A, B = (10, 20), (20, 30)
UNCOVERED = [
    # pc 12: probes h=1 (12<30), h=0 (12<20) -> A; adds {12,20}, deletes 12.  pc 20: h=1 (20<30), h=0 (20<20 false)
    # -> B; adds {20,25}, deletes 20 -> {25}
    ("two_order_ab", [A, B], [12, 20, 25], [12, 20], [25]),
    # pc 20 -> B first: adds {20,25}, deletes 20 -> {25}; pc 12 -> A: re-adds {12,20}, deletes 12 -> {20,25}
    ("two_order_ba", [A, B], [12, 20, 25], [20, 12], [20, 25]),
    # pc == end: 20<20 is false, the search runs off the end -> idx == len(symbols), skipped, nothing handled
    ("pc_eq_end_alone", [A], [10, 15, 20], [20], []),
    ("pc_eq_end_plus_1", [A], [10, 15, 20], [21], []),
    # pc 19 -> A handled: the range is start <= pc1 up to the first end < pc1, so site 20 == end is added
    ("end_is_inclusive", [A], [10, 15, 20], [19], [10, 15, 20]),
    # pc == end of (10,20) found through the next symbol: h=1 (20<40), h=0 (20<20 false) -> (15,40); 15<=20<=40
    ("pc_eq_end_next_symbol", [(10, 20), (15, 40)], [12, 18, 30], [20], [18, 30]),
    # 5<20 -> idx 0, but pc < start: skipped
    ("pc_below_start", [A], [10, 15, 20], [5], []),
    # aliases (10,20) and (10,30) in the caller's order.  pc 12: h=1 (12<30), h=0 (12<20) -> idx 0, handled[10]
    # with end 20: adds {12,15}, deletes 12.  pc 25: h=1 (25<30), h=0 (25<20 false) -> idx 1, start 10 already
    # handled: no add; deletes 25 (absent) -> {15}
    ("alias_short_first", [(10, 20), (10, 30)], [12, 15, 25, 28], [12, 25], [15]),
    # pc 25 first -> idx 1, handled[10] with end 30: adds {12,15,25,28}, deletes 25; pc 12 -> idx 0: deletes 12
    ("alias_long_first", [(10, 20), (10, 30)], [12, 15, 25, 28], [25, 12], [15, 28]),
    # nested: pc 25 lies in (20,30) but the probes are h=1 (25<30) then h=0 (25<100) -> the outer (10,100):
    # adds {25,45,60}, deletes 25
    ("nested_missed", [(10, 100), (20, 30), (40, 50)], [25, 45, 60], [25], [45, 60]),
    # pc 45: h=1 (45<30 false), h=2 (45<50) -> (40,50): adds {45}, deletes it
    ("nested_inner_hit", [(10, 100), (20, 30), (40, 50)], [25, 45, 60], [45], []),
    # pc 60 lies in the outer symbol only: h=1 false, h=2 (60<50 false) -> idx == 3, skipped
    ("nested_outer_lost", [(10, 100), (20, 30), (40, 50)], [25, 45, 60], [60], []),
    # 20 -> B: {25}; 12 -> A re-adds 20: {20,25}; 20 again -> B handled, deletes 20 -> {25}
    ("repeat_after_readd", [A, B], [12, 20, 25], [20, 12, 20], [25]),
    # both 20s come before A's add: {25}, {25}, then 12 -> A adds {12,20}, deletes 12 -> {20,25}
    ("repeat_before_readd", [A, B], [12, 20, 25], [20, 20, 12], [20, 25]),
    # pc 11 is in A but no site: A is handled all the same, nothing to delete
    ("pc_is_no_site", [A], [12, 15], [11], [12, 15]),
    ("nall_zero", [A], [], [12], []),
    # a zero-size symbol is never found: pc<end and pc>=start cannot both hold.  Alone: 10<10 false -> idx 1 == len
    ("zero_size_alone", [(10, 10)], [10], [10], []),
    # ... h=1 (10<40), h=0 (10<10 false) -> (30,40), pc < start: skipped
    ("zero_size_then_other", [(10, 10), (30, 40)], [10, 35], [10], []),
    # ... as an alias of a real symbol: h=1 (12<20), h=0 (12<10 false) -> idx 1, handled[10] with end 20
    ("zero_size_alias", [(10, 10), (10, 20)], [10, 15], [12], [10, 15]),
    ("no_symbols", [], [10], [10], []),
    ("no_pcs", [A], [12], [], []),
]

# (name, arch, base, pcs in map order, expected in order, expected sorted)
H = 0xFFFFFFFF00000000
REPORT_PCS = [
    ("amd64", "amd64", 0xFFFFFFFF, [0x81000005], [H + 0x81000000], [H + 0x81000000]),
    ("386", "386", 0xFFFFFFFF, [0x81000005], [H + 0x81000004], [H + 0x81000004]),
    ("arm64", "arm64", 0xFFFFFFFF, [0x81000005], [H + 0x81000001], [H + 0x81000001]),
    # (..05 - 3) = ..02, & ~1 = ..02
    ("arm", "arm", 0xFFFFFFFF, [0x81000005], [H + 0x81000002], [H + 0x81000002]),
    ("ppc64le", "ppc64le", 0xFFFFFFFF, [0x81000005], [H + 0x81000001], [H + 0x81000001]),
    # 0x1005 - 3 = 0x1002; 0x1006 - 3 = 0x1003, & ~1 = 0x1002: the list keeps both; 0x1009 - 3 = 0x1006
    ("arm_collide", "arm", 0, [0x1006, 0x1009, 0x1005], [0x1002, 0x1006, 0x1002], [0x1002, 0x1002, 0x1006]),
    # base 0: 3 - 5 wraps to 2^64 - 2 and sorts last; the sorted input [3, 5, 10] maps to an unsorted list
    ("wrap", "amd64", 0, [3, 10, 5], [M64 - 1, 5, 0], [0, 5, M64 - 1]),
    # arm at base 0: 2 - 3 wraps to 2^64 - 1, & ~1 = 2^64 - 2; 3 - 3 = 0; 4 - 3 = 1, & ~1 = 0
    ("wrap_arm", "arm", 0, [2, 3, 4], [M64 - 1, 0, 0], [0, 0, M64 - 1]),
    ("empty", "amd64", 0xFFFFFFFF, [], [], []),
]

# a corpus and collectSyscallInfo's sizes: "write" has one input with an empty cover, "open" none at all
CORPUS = {"a": ("read", [1, 2, 2]), "b": ("read", [2, 3]), "c": ("write", []), "d": ("mmap", [9, 1])}
SYSCALL_INFO = {"read": (2, 3), "write": (1, 0), "mmap": (1, 2)}
