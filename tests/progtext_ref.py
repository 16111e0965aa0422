"""The heads of program-text lines, restated from the reference in plain Python:
what syzkaller_amd/progtext.py computes on the device.

Lines follow bufio.Scanner with ScanLines and Buffer(nil, 1 << 20): the maximal
runs between b"\\n" inside the program, a last run without "\\n" if it is not
empty, one trailing "\\r" dropped.  A line of 2^20 bytes or more before its
"\\n" ("\\r" counted) fails the program with LINE_TOO_LONG: this is DERIVED from
bufio.Scanner's source (the split function runs before the buffer-full check, so
2^20 - 1 bytes plus "\\n" still scan), not observed -- no Go toolchain was at hand.
The line's number is then the one it would have had.

Deserialize mode (prog/encoding.go:159-180 over the parser of :740-828): a line
is I W* ( '=' W* I W* )? '(' from its first byte, W = space or tab, I = one or
more of [a-zA-Z0-9_$]; the name is the last I.  In the parser's order:
BAD_IDENT (no identifier at position 0, or none after '='), BAD_HEAD (the line
ends where '=' or '(' is expected: Char() at EOF), UNKNOWN_CALL (the lookup
comes before Parse('(')), BAD_HEAD (the next byte is not '(', or the line ends
there).  So "foo" alone is BAD_HEAD whether or not foo is known, and "r0 = foo"
alone is UNKNOWN_CALL for an unknown foo.  The program's status is its first
failing line's and err_line that line's 1-based number, skipped lines counted.
No call lines: OK with no calls (validate, which would object, is out of scope:
arguments are not parsed, validate() and SanitizeCall do not run).

CallSet mode (prog/encoding.go:841-860, byte for byte): the first '(' or
NO_BRACKET; the name is the line before it, restarted after its first '=' and
the SPACES (not tabs) behind it; empty: EMPTY_NAME; no calls at all: NO_CALLS
(err_line 0).
"""
OK, LINE_TOO_LONG, BAD_IDENT, BAD_HEAD, UNKNOWN_CALL, NO_BRACKET, EMPTY_NAME, NO_CALLS = range(8)
MAX_LINE = 1 << 20
IDENT = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_$")
WS = b" \t"


def lines(prog):
    """[(line without its "\\n" and "\\r", length before the "\\n")] of one program."""
    parts = prog.split(b"\n")
    if parts[-1] == b"":
        parts.pop()  # the program ends in "\n" (or is empty): no extra line
    return [(ln[:-1] if ln.endswith(b"\r") else ln, len(ln)) for ln in parts]


def skipped(ln):
    return len(ln) == 0 or ln[:1] == b"#"


def head_deserialize(ln):
    """(status, name) of a line that is not skipped: the parser's walk."""
    i, n = 0, len(ln)

    def ident():
        nonlocal i
        a = i
        while i < n and ln[i] in IDENT:
            i += 1
        s = ln[a:i]
        ws()
        return s

    def ws():
        nonlocal i
        while i < n and ln[i] in WS:
            i += 1

    name = ident()
    if not name:
        return BAD_IDENT, None
    if i == n:
        return BAD_HEAD, None
    if ln[i] == ord("="):
        i += 1
        ws()
        name = ident()
        if not name:
            return BAD_IDENT, None
    return (OK if i < n and ln[i] == ord("(") else BAD_HEAD), name


def head_callset(ln):
    """(status, name) of a line that is not skipped."""
    bracket = ln.find(b"(")
    if bracket == -1:
        return NO_BRACKET, None
    call = ln[:bracket]
    eq = call.find(b"=")
    if eq != -1:
        eq += 1
        while eq < len(call) and call[eq] == ord(" "):
            eq += 1
        call = call[eq:]
    if len(call) == 0:
        return EMPTY_NAME, None
    return OK, call


def prog_calls(prog, table, enabled=None):
    """Deserialize mode: (status, err_line, ids in line order, disabled)."""
    ids = []
    for no, (ln, raw) in enumerate(lines(prog), 1):
        if raw >= MAX_LINE:
            return LINE_TOO_LONG, no, [], 0
        if skipped(ln):
            continue
        st, name = head_deserialize(ln)
        if name is None:
            return st, no, [], 0
        if name not in table:
            return UNKNOWN_CALL, no, [], 0
        if st != OK:
            return st, no, [], 0
        ids.append(table[name])
    dis = int(enabled is not None and any(not enabled[i] for i in ids))
    return OK, 0, ids, dis


def call_set(prog, table, enabled=None):
    """CallSet mode: (status, err_line, sorted distinct known ids, supported, has_unknown)."""
    known, unknown, any_call = set(), False, False
    for no, (ln, raw) in enumerate(lines(prog), 1):
        if raw >= MAX_LINE:
            return LINE_TOO_LONG, no, [], 0, 0
        if skipped(ln):
            continue
        st, name = head_callset(ln)
        if st != OK:
            return st, no, [], 0, 0
        any_call = True
        if name in table:
            known.add(table[name])
        else:
            unknown = True
    if not any_call:
        return NO_CALLS, 0, [], 0, 0
    sup = int(not unknown and (enabled is None or all(enabled[i] for i in known)))
    return OK, 0, sorted(known), sup, int(unknown)


def table_of(names):
    return {bytes(n): i for i, n in enumerate(names)}


def batch(progs, names, mode, enabled=None):
    """A whole batch as the device returns it: (off, ids, status, err_line, flag) as lists."""
    t = table_of(names)
    off, ids, status, err, flag = [0], [], [], [], []
    for p in progs:
        if mode == 0:
            st, el, i, f = prog_calls(p, t, enabled)
        else:
            st, el, i, sup, unk = call_set(p, t, enabled)
            f = sup | unk << 1
        ids += i
        off.append(len(ids))
        status.append(st)
        err.append(el)
        flag.append(f)
    return off, ids, status, err, flag


def load_corpus(progs, names, enabled):
    """loadCorpus's split (syz-manager/manager.go:209-240) without the shuffle:
    the indices of the broken, the disabled and the candidate programs."""
    t = table_of(names)
    broken, disabled, cand = [], [], []
    for i, p in enumerate(progs):
        st, _, _, dis = prog_calls(p, t, enabled)
        (broken if st != OK else disabled if dis else cand).append(i)
    return broken, disabled, cand


def gen_program(rng, names, ncalls):
    """A program in the shape Serialize writes: rN = name(0x..., &(0x7f0000000000)=...)."""
    out = []
    for k in range(ncalls):
        nm = names[int(rng.integers(0, len(names)))]
        head = (b"r%d = " % k if rng.integers(0, 2) else b"") + nm
        out.append(head + b"(0x%x, &(0x7f0000000000)={0x%x, 0x0, @void}, 0x%x)\n"
                   % (int(rng.integers(0, 1 << 31)), int(rng.integers(0, 1 << 16)), int(rng.integers(0, 4096))))
    return b"".join(out)
