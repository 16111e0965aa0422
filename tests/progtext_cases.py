"""Hand-derived program-text cases: every expected result below was written out
by hand from prog/encoding.go (the parser of :740-828, Deserialize's loop head
:159-180, CallSet :836-869), not produced by tests/progtext_ref.py.

A case is (name, text, des, cs): des = (status, err_line, ids) in Deserialize
mode, cs = (status, err_line, sorted distinct known ids, has_unknown) in CallSet
mode.  Ids are indices into NAMES.
"""
from tests.progtext_ref import (BAD_HEAD, BAD_IDENT, EMPTY_NAME, LINE_TOO_LONG, MAX_LINE, NO_BRACKET, NO_CALLS, OK,
                                UNKNOWN_CALL)

NAMES = [b"open", b"close", b"close$foo", b"getpid", b"read", b"foo", b"$", b"0day", b"getpi", b"getpid2"]
OPEN, CLOSE, CLOSE_FOO, GETPID, READ, FOO, DOLLAR, ZDAY, GETPI, GETPID2 = range(10)

SIX = (b"getpid()\n"
       b"open(0x1, something that this package may not understand)\n"
       b"getpid()\n"
       b"#read()\n"
       b"\n"
       b"close$foo(&(0x0000) = {})\n")

CASES = [
    # the five inputs of the reference's TestCallSet
    ("empty", b"", (OK, 0, []), (NO_CALLS, 0, [], 0)),
    # "r0 =  (foo)": no identifier after the '='; CallSet: the name before '(' is empty once the spaces go
    ("eq-then-bracket", b"r0 =  (foo)", (BAD_IDENT, 1, []), (EMPTY_NAME, 1, [], 0)),
    ("getpid", b"getpid()", (OK, 0, [GETPID]), (OK, 0, [GETPID], 0)),
    ("r11-getpid", b"r11 =  getpid()", (OK, 0, [GETPID]), (OK, 0, [GETPID], 0)),
    ("six-lines", SIX, (OK, 0, [GETPID, OPEN, GETPID, CLOSE_FOO]), (OK, 0, [OPEN, CLOSE_FOO, GETPID], 0)),
    # line splitting
    ("no-final-newline", b"getpid()\nopen()", (OK, 0, [GETPID, OPEN]), (OK, 0, [OPEN, GETPID], 0)),
    ("crlf", b"getpid()\r\nopen()\r\n", (OK, 0, [GETPID, OPEN]), (OK, 0, [OPEN, GETPID], 0)),
    # a line that is just "\r" is empty after the drop: skipped, but counted (the error is on line 3)
    ("just-cr", b"getpid()\n\r\n(\n", (BAD_IDENT, 3, []), (EMPTY_NAME, 3, [], 0)),
    ("cr-at-program-end", b"getpid()\r", (OK, 0, [GETPID]), (OK, 0, [GETPID], 0)),
    ("only-newlines", b"\n\n\r\n", (OK, 0, []), (NO_CALLS, 0, [], 0)),
    # '#' not in column 0 is no comment: ' ' is no identifier; CallSet finds no bracket
    ("hash-col-1", b" #x", (BAD_IDENT, 1, []), (NO_BRACKET, 1, [], 0)),
    ("hash-col-1-bracket", b" #getpid()", (BAD_IDENT, 1, []), (OK, 0, [], 1)),
    # "\r" before '(': not a line end, so it stays in the line; the parser wants '(' there
    ("cr-before-bracket", b"getpid\r()", (BAD_HEAD, 1, []), (OK, 0, [], 1)),
    # heads: a tab after '=' is skipped by the parser's SkipWs, kept by CallSet (its loop skips ' ' only)
    ("tab-after-eq", b"r0 =\tgetpid()", (OK, 0, [GETPID]), (OK, 0, [], 1)),
    ("space-before-bracket", b"getpid ()", (OK, 0, [GETPID]), (OK, 0, [], 1)),
    ("no-spaces", b"r0=getpid(", (OK, 0, [GETPID]), (OK, 0, [GETPID], 0)),
    # two '=': after "r0 = r1" the parser is at '=' where it wants '(' -- but r1 is looked up first
    ("two-eq", b"r0 = r1 = getpid()", (UNKNOWN_CALL, 1, []), (OK, 0, [], 1)),
    ("two-eq-known", b"r0 = foo = getpid()", (BAD_HEAD, 1, []), (OK, 0, [], 1)),
    ("eq-after-bracket", b"close$foo(&(0x0000) = {})", (OK, 0, [CLOSE_FOO]), (OK, 0, [CLOSE_FOO], 0)),
    ("digit-ident", b"0day()", (OK, 0, [ZDAY]), (OK, 0, [ZDAY], 0)),
    ("dollar", b"$()", (OK, 0, [DOLLAR]), (OK, 0, [DOLLAR], 0)),
    ("non-ascii", b"\xc3\xa9getpid()", (BAD_IDENT, 1, []), (OK, 0, [], 1)),
    ("only-spaces", b"   ", (BAD_IDENT, 1, []), (NO_BRACKET, 1, [], 0)),
    ("name-alone", b"foo", (BAD_HEAD, 1, []), (NO_BRACKET, 1, [], 0)),
    ("name-alone-unknown", b"bar", (BAD_HEAD, 1, []), (NO_BRACKET, 1, [], 0)),
    ("eq-alone", b"r0 =", (BAD_IDENT, 1, []), (NO_BRACKET, 1, [], 0)),
    ("eq-name-alone", b"r0 = foo", (BAD_HEAD, 1, []), (NO_BRACKET, 1, [], 0)),
    ("eq-unknown-alone", b"r0 = bar", (UNKNOWN_CALL, 1, []), (NO_BRACKET, 1, [], 0)),
    ("unknown-then-junk", b"nosuch junk", (UNKNOWN_CALL, 1, []), (NO_BRACKET, 1, [], 0)),
    ("known-then-junk", b"getpid junk(", (BAD_HEAD, 1, []), (OK, 0, [], 1)),
    ("unknown-call", b"nosuch()", (UNKNOWN_CALL, 1, []), (OK, 0, [], 1)),
    ("prefix-names", b"getpi()\ngetpid()\ngetpid2()\n", (OK, 0, [GETPI, GETPID, GETPID2]),
     (OK, 0, [GETPID, GETPI, GETPID2], 0)),
    # the first error: on line 1, in the middle, last; later errors do not matter
    ("err-first", b"(\ngetpid()\nnosuch()\n", (BAD_IDENT, 1, []), (EMPTY_NAME, 1, [], 0)),
    ("err-middle", b"getpid()\nfoo\n(\n", (BAD_HEAD, 2, []), (NO_BRACKET, 2, [], 0)),
    ("err-last", b"getpid()\nopen()\n=", (BAD_IDENT, 3, []), (NO_BRACKET, 3, [], 0)),
    # err_line counts the skipped lines: comment, empty, "\r", then the bad line is number 5
    ("err-line-counts-skipped", b"getpid()\n#c\n\n\r\nfoo\n", (BAD_HEAD, 5, []), (NO_BRACKET, 5, [], 0)),
    ("known-and-unknown", b"getpid()\nr1 = nosuch$x(0x0)\n", (UNKNOWN_CALL, 2, []), (OK, 0, [GETPID], 1)),
    ("eq-spaces-only-name", b"r0 =   (", (BAD_IDENT, 1, []), (EMPTY_NAME, 1, [], 0)),
    ("eq-first", b"=getpid()", (BAD_IDENT, 1, []), (OK, 0, [GETPID], 0)),
]


def long_line_cases():
    """The 2^20 boundary (built, not listed: a megabyte each).  'x' * k + '(' is
    an unknown name in both modes when it scans."""
    fits = b"getpid(" + b"x" * (MAX_LINE - 1 - 7)  # 2^20 - 1 bytes
    return [
        ("max-line-fits", b"open()\n" + fits + b"\nclose()\n", (OK, 0, [OPEN, GETPID, CLOSE]),
         (OK, 0, [OPEN, CLOSE, GETPID], 0)),
        ("max-line-fits-cr", b"open()\n" + fits[:-1] + b"\r\nclose()\n", (OK, 0, [OPEN, GETPID, CLOSE]),
         (OK, 0, [OPEN, CLOSE, GETPID], 0)),
        ("line-too-long", b"open()\n" + fits + b"x\nclose()\n", (LINE_TOO_LONG, 2, []), (LINE_TOO_LONG, 2, [], 0)),
        ("line-too-long-cr", b"open()\n" + fits + b"\r\nclose()\n", (LINE_TOO_LONG, 2, []), (LINE_TOO_LONG, 2, [], 0)),
        ("line-too-long-at-end", b"open()\n" + fits + b"x", (LINE_TOO_LONG, 2, []), (LINE_TOO_LONG, 2, [], 0)),
        ("line-fits-at-end", b"open()\n" + fits, (OK, 0, [OPEN, GETPID]), (OK, 0, [OPEN, GETPID], 0)),
        # an earlier error wins over the long line; the long line wins over a later one
        ("error-before-long", b"(\n" + fits + b"x\n", (BAD_IDENT, 1, []), (EMPTY_NAME, 1, [], 0)),
        ("long-before-error", b" " * MAX_LINE + b"\n(\n", (LINE_TOO_LONG, 1, []), (LINE_TOO_LONG, 1, [], 0)),
    ]
