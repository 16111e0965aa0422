"""The inner half of generateHints restated in plain Python: the checker of
syzsig_hint_mutants_dev.

A line-by-line restatement of the cited Go on top of comps_ref.shrink_expand
(prog/hints.go:164-218), kept to outcomes worked out by hand in
tests/test_hints_ref_cpu.py:
  check_const_arg   prog/hints.go:105-112
  check_data_arg    prog/hints.go:114-132 (maxDataLength :38)
  apply             the copy() of :126-127 on its own
  hint_mutants      generateHints' switch (:97-102) over a batch of args
Go ranges over a uint64Set in map order; here a window's replacers come
ascending (as comps_ref.shrink_expand returns them): one fixed instance of
that order.
"""
import numpy as np

from tests import comps_ref as R

MAX_DATA_LENGTH = 100                                                # :38


def check_const_arg(val, comp_map, special_ints=()):
    """-> [(at, nb, rep)]: exec() runs once per replacer with arg.Val = rep."""
    original = val                                                   # :106
    return [(0, 8, replacer)
            for replacer in R.shrink_expand(original, comp_map, special_ints)]  # :107-109


def check_data_arg(data, comp_map, special_ints=()):
    """-> [(at, nb, rep)]: exec() runs once per entry with data[at:at + nb] set
    to the low nb bytes of rep (apply)."""
    out = []
    data = bytes(data)                                               # :116
    size = len(data)                                                 # :117
    if size > MAX_DATA_LENGTH:                                       # :118-120
        size = MAX_DATA_LENGTH
    for i in range(size):                                            # :121
        original = bytearray(8)                                      # :122
        src = data[i:i + 8]                                          # :123 copy(): min(8, len(data) - i) bytes
        original[:len(src)] = src
        val = int.from_bytes(original, "little")                     # :124
        for replacer in R.shrink_expand(val, comp_map, special_ints):  # :125
            nb = min(8, len(data) - i)                               # :127 copy(data[i:], bytes) stops at the arg's end
            out.append((i, nb, replacer))                            # :126-128
    return out


def apply(data, at, nb, rep):
    """:126-127: bytes := LittleEndian(rep); copy(data[at:], bytes)."""
    data = bytearray(data)
    b = (rep & R.M64).to_bytes(8, "little")                          # :126
    n = min(8, len(data) - at)                                       # :127
    assert n == nb
    data[at:at + n] = b[:n]
    return bytes(data)


def hint_mutants(maps, arg_call, arg_kind, arg_val, arg_off, data, special_ints=()):
    """A batch: arg a is a ConstArg (kind 0, arg_val[a]) or a DataArg (kind 1,
    data[arg_off[a]:arg_off[a + 1]]) matched against maps[arg_call[a]] (:97-102)
    -> (mut_off u64[narg + 1], at u32[], nb u8[], rep u64[])."""
    data = bytes(data)
    off, at, nb, rep = [0], [], [], []
    for a in range(len(arg_call)):
        m = maps[int(arg_call[a])]
        if int(arg_kind[a]) == 0:                                    # :98-99
            r = check_const_arg(int(arg_val[a]), m, special_ints)
        else:                                                        # :100-101
            r = check_data_arg(data[int(arg_off[a]):int(arg_off[a + 1])], m, special_ints)
        at += [x[0] for x in r]
        nb += [x[1] for x in r]
        rep += [x[2] for x in r]
        off.append(off[-1] + len(r))
    return np.array(off, np.uint64), np.array(at, np.uint32), np.array(nb, np.uint8), np.array(rep, np.uint64)
