"""The manager's coverage-page loops restated line by line in plain Python:
collectSyscallInfo and httpCover's selection (syz-manager/html.go:135-149,
:202-212), RestorePC / previousInstructionPC / httpRawCover's sort
(pkg/cover/cover.go:28-30, syz-manager/cover.go:394-411, html.go:323-338) and
uncoveredPcsInFuncs (cover.go:254-304) with sort.Search's own loop and Go's
map semantics, the order of `pcs` being a parameter.  There is no Go toolchain
here, so tests/test_report_ref_cpu.py holds this restatement to hand-derived
cases; tests/test_gpu_report.py holds the device to it."""

M64 = (1 << 64) - 1


def sort_search(n, f):
    """sort.Search (sort/search.go): the probe sequence matters when f is not
    monotone."""
    i, j = 0, n
    while i < j:
        h = (i + j) >> 1
        if not f(h):
            i = h + 1
        else:
            j = h
    return i


# ---- html.go:135-149, :202-212 ----

def collect_syscall_info(corpus):
    """corpus: {sig: (call, cover list)}.  Returns {call: [count, cov set]}."""
    calls = {}
    for _, (call, cover) in corpus.items():
        if call not in calls:
            calls[call] = [0, set()]
        cc = calls[call]
        cc[0] += 1
        cc[1].update(int(pc) for pc in cover)  # cov.Merge(inp.Cover)
    return calls


def http_cover(corpus, call="", input=""):
    """httpCover's cov: None is Go's nil Cover (never merged into)."""
    cov = None
    if input != "":
        cov = set(int(pc) for pc in corpus[input][1])  # a missing sig: KeyError, Go's nil dereference
    else:
        for _, (c, cover) in corpus.items():
            if call == "" or call == c:
                if cov is None:
                    cov = set()
                cov.update(int(pc) for pc in cover)
    return cov


# ---- cover.go:28-30, :394-411; html.go:323-338 ----

def restore_pc(pc, base):
    return ((base << 32) + pc) & M64


def previous_instruction_pc(arch, pc):
    if arch == "amd64":
        return (pc - 5) & M64
    if arch == "386":
        return (pc - 1) & M64
    if arch == "arm64":
        return (pc - 4) & M64
    if arch == "arm":
        return ((pc - 3) & M64) & (M64 ^ 1)
    if arch == "ppc64le":
        return (pc - 4) & M64
    raise RuntimeError("unknown arch")  # panic("unknown arch")


def report_pcs(cov, base, arch):
    """cov: the PCs in the order the map iteration gives them.  Returns
    (generateCoverHTML's pcs, httpRawCover's sorted pcs)."""
    pcs = []
    for pc in cov:
        pcs.append(previous_instruction_pc(arch, restore_pc(int(pc), base)))
    return pcs, sorted(pcs)


def raw_cover_text(cov, base, arch):
    return "".join("0x%x\n" % pc for pc in report_pcs(cov, base, arch)[1])


# ---- cover.go:254-304 ----

def uncovered_pcs_in_funcs(symbols, all_cover_pcs, pcs):
    """symbols: [(start, end)] already sorted by start (cover.go:265);
    all_cover_pcs ascending; pcs in the loop's order.  Returns the keys of
    `uncovered`, sorted (Go returns them in map order)."""
    if len(all_cover_pcs) == 0:
        return []
    handled = set()
    uncovered = {}
    for pc in pcs:
        idx = sort_search(len(symbols), lambda i: pc < symbols[i][1])
        if idx == len(symbols):
            continue
        start, end = symbols[idx]
        if pc < start or pc > end:
            continue
        if start not in handled:
            handled.add(start)
            start_pc = sort_search(len(all_cover_pcs), lambda i: start <= all_cover_pcs[i])
            end_pc = sort_search(len(all_cover_pcs), lambda i: end < all_cover_pcs[i])
            for pc1 in all_cover_pcs[start_pc:end_pc]:
                uncovered[pc1] = True
        uncovered.pop(pc, None)
    return sorted(uncovered)
