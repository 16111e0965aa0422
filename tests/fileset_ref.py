"""fileSet, generateCoverHTML's line walk, parseFile's line count and
templateFileArray.Less (syz-manager/cover.go:129-148, :162-214, :427-440)
restated in plain Python, statement by statement.  Frames are (File, Line,
Func) tuples; Go's maps are dicts and sets."""
import functools


def file_set(covered, uncovered):
    """cover.go:162-193.  {file: [(line, covered), ...]}, each list sorted by line."""
    files = {}                                   # map[string]map[int]bool
    funcs = set()                                # map[string]bool (only ever set to true)
    for file, line, func in covered:             # :165-171
        if file not in files:
            files[file] = {}
        files[file][line] = True
        funcs.add(func)
    for file, line, func in uncovered:           # :172-182
        if func not in funcs:
            continue
        if file not in files:
            files[file] = {}
        if not files[file].get(line, False):     # a missing key reads as false
            files[file][line] = False
    res = {}
    for f, lines in files.items():               # :184-191
        res[f] = sorted(lines.items(), key=lambda e: e[0])  # coverageArray orders by line; lines are distinct
    return res


def walk(nlines, covered):
    """cover.go:129-148 over a file of `nlines` lines and its sorted list:
    (entries consumed, coverage).  The loop, not its closed form."""
    covered = list(covered)
    coverage = 0
    shown = 0
    for i in range(nlines):                      # for i, ln := range lines
        if len(covered) > 0 and covered[0][0] == i + 1:
            if covered[0][1]:
                coverage += 1
            covered = covered[1:]
            shown += 1
    return shown, coverage


def walk_closed(nlines, covered):
    """The same in closed form: nothing when the list is empty or its head is
    below line 1, else the entries with line <= nlines."""
    if not covered or covered[0][0] < 1:
        return 0, 0
    shown = sum(1 for ln, _ in covered if ln <= nlines)
    return shown, sum(1 for _, c in covered[:shown] if c)


def parse_file_nlines(data):
    """len(parseFile) (cover.go:195-214), by its loop over IndexByte."""
    n = 0
    while True:
        idx = data.find(b"\n")
        if idx == -1:
            break
        n += 1
        data = data[idx + 1:]
    if len(data) != 0:
        n += 1
    return n


def less(n1, n2):
    """templateFileArray.Less (cover.go:427-440) over the names."""
    if len(n1) != 0 and len(n2) != 0:
        if n1[0] != "." and n2[0] == ".":
            return True
        if n1[0] == "." and n2[0] != ".":
            return False
    return n1 < n2


def file_order(names):
    return sorted(names, key=functools.cmp_to_key(lambda a, b: -1 if less(a, b) else (1 if less(b, a) else 0)))


def cover_files(covered, uncovered, nlines):
    """generateCoverHTML's d.Files after the sort: [(name, coverage, shown, list)]."""
    out = {}
    for f, lst in file_set(covered, uncovered).items():
        shown, cov = walk(nlines.get(f, 0), lst)
        out[f] = (f, cov, shown, lst)
    return [out[f] for f in file_order(list(out))]
