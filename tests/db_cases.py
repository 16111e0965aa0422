"""Hand-derived database files for pkg/db's replay (pkg/db/db.go:177-265), as
byte literals: stored blocks only, so that no compressor stands between a case
and its expected map.  CASES: name -> (file, version, records {key: (val, seq)},
uncompacted, ended), `ended` in tests/db_ref.py's words."""

HDR2 = b"\xdb\xad\x0b\x00" b"\x02\x00\x00\x00" b"\x07\x00\x00\x00\x00\x00\x00\x00"  # magic, version 2, user version 7
HDR1 = b"\xdb\xad\x0b\x00" b"\x01\x00\x00\x00"  # version 1: no user version
REC = b"\xad\x1b\xee\x0f"  # 0xfee1bad
K40 = b"\x28\x00\x00\x00"  # key length 40
KA = b"aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa"
KB = b"0123456789abcdef0123456789abcdef01234567"
KC = b"ffffffffffffffffffffffffffffffffffffff00"
SEQ1 = b"\x01\x00\x00\x00\x00\x00\x00\x00"
SEQ2 = b"\x02\x00\x00\x00\x00\x00\x00\x00"
SEQ3 = b"\x03\x00\x00\x00\x00\x00\x00\x00"
SEQ5 = b"\x05\x00\x00\x00\x00\x00\x00\x00"
DEL = b"\xff\xff\xff\xff\xff\xff\xff\xff"  # seqDeleted: no valLen follows
FLUSH_CLOSE = b"\x00\x00\x00\xff\xff" b"\x01\x00\x00\xff\xff"  # the empty stored block of Flush, the final one of Close
# valLen + the stream: one stored block (LEN, ~LEN, bytes), then Flush and Close
V_ABC = b"\x12\x00\x00\x00" b"\x00\x03\x00\xfc\xff" b"abc" + FLUSH_CLOSE
V_XY = b"\x11\x00\x00\x00" b"\x00\x02\x00\xfd\xff" b"xy" + FLUSH_CLOSE
V_Q = b"\x06\x00\x00\x00" b"\x01\x01\x00\xfe\xff" b"q"  # one final stored block, no Flush / Close blocks
V_EMPTY = b"\x00\x00\x00\x00"  # valLen 0: no stream at all
V_TYPE3 = b"\x12\x00\x00\x00" b"\x06\x03\x00\xfc\xff" b"abc" + FLUSH_CLOSE  # block type 3
V_NLEN = b"\x12\x00\x00\x00" b"\x00\x03\x00\xfd\xff" b"abc" + FLUSH_CLOSE  # LEN != ~NLEN
V_CUT = b"\x0d\x00\x00\x00" b"\x00\x03\x00\xfc\xff" b"abc" b"\x00\x00\x00\xff\xff"  # no final block inside valLen
V_TRAIL = b"\x13\x00\x00\x00" b"\x00\x03\x00\xfc\xff" b"abc" + FLUSH_CLOSE + b"\x00"  # a byte after the final block

A1 = REC + K40 + KA + SEQ1 + V_ABC
A2 = REC + K40 + KA + SEQ2 + V_XY
A3 = REC + K40 + KA + SEQ3 + V_XY
B1 = REC + K40 + KB + SEQ1 + V_ABC
B2 = REC + K40 + KB + SEQ2 + V_Q
C3 = REC + K40 + KC + SEQ3 + V_XY

CASES = {
    "overwrite": (HDR2 + A1 + A2, 7, {KA: (b"xy", 2)}, 2, "eof"),
    "delete_then_readd": (HDR2 + A1 + REC + K40 + KA + DEL + A3, 7, {KA: (b"xy", 3)}, 3, "eof"),
    "delete_only": (HDR2 + A1 + REC + K40 + KA + DEL, 7, {}, 2, "eof"),
    "delete_absent": (HDR2 + REC + K40 + KB + DEL + A1, 7, {KA: (b"abc", 1)}, 2, "eof"),
    "same_twice": (HDR2 + A1 + A1, 7, {KA: (b"abc", 1)}, 2, "eof"),
    "empty_value": (HDR2 + REC + K40 + KA + SEQ5 + V_EMPTY + B1, 7, {KA: (b"", 5), KB: (b"abc", 1)}, 2, "eof"),
    "three_keys": (HDR2 + A1 + B2 + C3, 7, {KA: (b"abc", 1), KB: (b"q", 2), KC: (b"xy", 3)}, 3, "eof"),
    "version1_header": (HDR1 + A1 + B2, 0, {KA: (b"abc", 1), KB: (b"q", 2)}, 2, "eof"),
    "header_only": (HDR2, 7, {}, 0, "eof"),
    "empty_file": (b"", 0, {}, 0, "eof"),
    "bad_magic": (b"\xdc\xad\x0b\x00" + HDR2[4:] + A1, 0, {}, 0, "bad_header"),
    "version0": (HDR2[:4] + b"\x00\x00\x00\x00" + HDR2[8:] + A1, 0, {}, 0, "bad_header"),
    "version3": (HDR2[:4] + b"\x03\x00\x00\x00" + HDR2[8:] + A1, 0, {}, 0, "bad_header"),
    "header_cut": (HDR2[:11], 0, {}, 0, "bad_header"),
    "error_first": (HDR2 + REC + K40 + KA + SEQ1 + V_TYPE3 + B2 + C3, 7, {}, 0, "inflate"),
    "error_middle": (HDR2 + A1 + REC + K40 + KB + SEQ2 + V_NLEN + C3, 7, {KA: (b"abc", 1)}, 1, "inflate"),
    "error_last": (HDR2 + A1 + B2 + REC + K40 + KC + SEQ3 + V_CUT, 7, {KA: (b"abc", 1), KB: (b"q", 2)}, 2, "inflate"),
    "error_hides_delete": (HDR2 + A1 + REC + K40 + KB + SEQ2 + V_TYPE3 + REC + K40 + KA + DEL, 7, {KA: (b"abc", 1)}, 1,
                           "inflate"),
    "trailing_middle": (HDR2 + A1 + REC + K40 + KB + SEQ2 + V_TRAIL + C3, 7, {KA: (b"abc", 1)}, 1, "trailing"),
    "bad_record_magic": (HDR2 + A1 + b"\xae\x1b\xee\x0f" + B2[4:], 7, {KA: (b"abc", 1)}, 1, "bad_magic"),
    "cut_in_key": (HDR2 + A1 + B2[:20], 7, {KA: (b"abc", 1)}, 1, "truncated"),
    "cut_in_value": (HDR2 + A1 + C3[:-3], 7, {KA: (b"abc", 1)}, 1, "truncated"),
    "huge_key_length": (HDR2 + A1 + REC + b"\xff\xff\xff\xff" + KB + SEQ2 + V_Q, 7, {KA: (b"abc", 1)}, 1, "truncated"),
}

# a non-hex key: the same answers through the host replay
NONHEX = (HDR2 + A1 + REC + b"\x03\x00\x00\x00" + b"Key" + SEQ2 + V_XY + A2 + REC + b"\x03\x00\x00\x00" + b"Key" + DEL + B1,
          7, {KA: (b"xy", 2), KB: (b"abc", 1)}, 5, "eof")
