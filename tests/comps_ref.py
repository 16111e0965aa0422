"""Restatement of the comparison-hints half of the per-execution path, the
checker of syzsig_exec_comps_dev, syzsig_comp_map_dev and
syzsig_shrink_expand_dev.

ignore, write_comp, call_comps / exec_comps and MAX_COMPS are pinned to the
compiled reference: the harness (oracle/ref_harness.cc, comps mode) runs the
reference's own handle_completion with flag_collect_comps on, its output
region mapped at a given address, and tests/test_golden_cover_comps_cpu.py
holds this file word for word to what it wrote (tests/golden/comps, and a
live run on fresh records where the harness is built); parse_comps is run on
the regions the reference wrote, which pins the framing it reads.  What
parse_comps makes of the records, swap_int and shrink_expand restate Go
(ipc.go, mutation.go, hints.go; no Go toolchain) and stay restatement-only:
tests/test_comps_ref_cpu.py holds them to hand-derived cases.  Plain Python
integers throughout: every step is written as the reference writes it, one
record at a time.

  ignore                executor/executor_linux.cc:221-253
  write_comp            executor/executor.h:823-859
  call_comps/exec_comps executor/executor.h:576-593, :861-875
  parse_comps           pkg/ipc/ipc.go:420-465, prog/hints.go:43-48
  swap_int              prog/mutation.go:566-579
  shrink_expand         prog/hints.go:164-218
"""
import numpy as np

M64 = (1 << 64) - 1
KCOV_CMP_CONST, KCOV_CMP_SIZE1, KCOV_CMP_SIZE2, KCOV_CMP_SIZE4, KCOV_CMP_SIZE8 = 1, 0, 2, 4, 6  # executor.h:147-151
KCOV_CMP_SIZE_MASK = 6                                                                             # executor.h:152
K_MAX_OUTPUT = 16 << 20                                                                            # executor.h kMaxOutput
MAX_COMPS = 65535  # executor.h:581-582 with kCoverSize = 256 << 10: 8 + 32 n <= 8 kCoverSize
INGEST_OK, INGEST_ECOMPS, INGEST_ECOMPTYPE = 0, 8, 9  # include/syzsig.h


def ignore(typ, arg1, arg2, out_start):
    """executor_linux.cc:221-253, the x86_64 branch included."""
    if arg1 == 0 and (arg2 == 0 or (typ & KCOV_CMP_CONST)):          # :224
        return True
    if (typ & KCOV_CMP_SIZE_MASK) == KCOV_CMP_SIZE8:                 # :226
        out_end = (out_start + K_MAX_OUTPUT) & M64                   # :231
        if out_start <= arg1 <= out_end:                             # :232
            return True
        if out_start <= arg2 <= out_end:                             # :234
            return True
        kmem_start, kmem_end = 0xffff880000000000, 0xffff890000000000  # :240-241
        kptr1 = kmem_start <= arg1 <= kmem_end
        kptr2 = kmem_start <= arg2 <= kmem_end
        if kptr1 and kptr2:                                          # :244
            return True
        if kptr1 and arg2 == 0:                                      # :246
            return True
        if kptr2 and arg1 == 0:                                      # :248
            return True
    return False


def _sext(v, bits):
    v &= (1 << bits) - 1
    return (v | (M64 ^ ((1 << bits) - 1))) if v >> (bits - 1) else v


def write_comp(typ, arg1, arg2):
    """executor.h:823-859: the words one record writes."""
    words = [typ & 0xffffffff]                                       # :826
    size = typ & KCOV_CMP_SIZE_MASK
    if size == KCOV_CMP_SIZE1:                                       # :835-838
        arg1, arg2 = _sext(arg1, 8), _sext(arg2, 8)
    elif size == KCOV_CMP_SIZE2:                                     # :839-842
        arg1, arg2 = _sext(arg1, 16), _sext(arg2, 16)
    elif size == KCOV_CMP_SIZE4:                                     # :843-846
        arg1, arg2 = _sext(arg1, 32), _sext(arg2, 32)
    if size != KCOV_CMP_SIZE8:                                       # :849-853
        return words + [arg1 & 0xffffffff, arg2 & 0xffffffff]
    return words + [arg1 & 0xffffffff, arg1 >> 32, arg2 & 0xffffffff, arg2 >> 32]  # :855-858


def call_comps(recs, out_start):
    """One call's comps output: executor.h:583-591.  recs = rows of (type, arg1,
    arg2, pc).  Returns (words list, comps_size)."""
    recs = [(int(r[0]), int(r[1]), int(r[2])) for r in recs]
    if len(recs) > MAX_COMPS:                                        # :581-582
        raise ValueError("too many comparisons")
    recs.sort()                                                      # :583, operator< :867-875
    uniq = [r for i, r in enumerate(recs) if i == 0 or r != recs[i - 1]]  # :584, operator== :861-865
    words, comps_size = [], 0
    for t, a1, a2 in uniq:                                           # :586
        if ignore(t, a1, a2, out_start):                             # :587
            continue
        comps_size += 1                                              # :589
        words += write_comp(t, a1, a2)                               # :590
    return words, comps_size


def exec_comps(comps, call_start, call_len, out_start, fill=0):
    """Every call of a batch, in the layout of syzsig_exec_comps_dev: call c's
    words at out[5 * call_start[c] ..].  Returns (out u32[5 * ncmp], `fill`
    wherever nothing is written, out_words u32[], comps_cnt u32[])."""
    comps = np.asarray(comps, np.uint64).reshape(-1, 4)
    out = np.full(5 * comps.shape[0], fill, np.uint32)
    nw = np.zeros(len(call_len), np.uint32)
    cnt = np.zeros(len(call_len), np.uint32)
    for c in range(len(call_len)):
        s, n = int(call_start[c]), int(call_len[c])
        w, k = call_comps(comps[s:s + n].tolist(), out_start)
        out[5 * s:5 * s + len(w)] = np.array(w, np.uint32) if w else np.empty(0, np.uint32)
        nw[c], cnt[c] = len(w), k
    return out, nw, cnt


def parse_comps(words, start, comps_size, end=None):
    """ipc.go:420-465 for one call: comps_size records from words[start] on,
    inside words[:end].  Returns (status, CompMap as {key: set(values)}); the
    map is empty where the Go returns an error."""
    end = len(words) if end is None else end
    pos, m = start, {}

    def add(a1, a2):                                                 # hints.go:43-48
        m.setdefault(a1, set()).add(a2)

    for _ in range(comps_size):                                      # :422
        if pos >= end:                                               # :424-428
            return INGEST_ECOMPS, {}
        typ = int(words[pos])
        pos += 1
        if typ > (1 | 6):                                            # :429-433
            return INGEST_ECOMPTYPE, {}
        if (typ & 6) == 6:                                           # :438-442
            if end - pos < 4:
                return INGEST_ECOMPS, {}
            op1 = int(words[pos]) | int(words[pos + 1]) << 32
            op2 = int(words[pos + 2]) | int(words[pos + 3]) << 32
            pos += 4
        else:                                                        # :443-451
            if end - pos < 2:
                return INGEST_ECOMPS, {}
            op1, op2 = int(words[pos]), int(words[pos + 1])          # uint64(tmp): zero-extended
            pos += 2
        if op1 == op2:                                               # :452-454
            continue
        add(op2, op1)                                                # :455
        if typ & 1:                                                  # :456-462
            continue
        add(op1, op2)                                                # :463
    return INGEST_OK, m


def map_pairs(m):
    """A CompMap's (key, value) pairs sorted by key, then value: u64[n, 2]."""
    p = sorted((k, v) for k, vs in m.items() for v in vs)
    return np.array(p, np.uint64).reshape(-1, 2)


def comp_map(words, comps_start, comps_cnt, comps_end=None):
    """Every call of a batch -> (status i32[], map_off u64[ncalls + 1], pairs
    u64[n, 2], maps list of dicts)."""
    st, off, pairs, maps = [], [0], [], []
    for c in range(len(comps_cnt)):
        s, m = parse_comps(words, int(comps_start[c]), int(comps_cnt[c]),
                           None if comps_end is None else int(comps_end[c]))
        p = map_pairs(m)
        st.append(s)
        maps.append(m)
        pairs.append(p)
        off.append(off[-1] + p.shape[0])
    allp = np.concatenate(pairs) if pairs else np.empty((0, 2), np.uint64)
    return np.array(st, np.int32), np.array(off, np.uint64), allp, maps


def swap_int(v, size):
    """prog/mutation.go:566-579: truncates to the size, swaps, zero-extends."""
    if size == 1:
        return v
    return int.from_bytes((v & ((1 << (8 * size)) - 1)).to_bytes(size, "little"), "big")


def shrink_expand(v, comp_map_, special_ints=()):
    """prog/hints.go:164-218.  Returns the replacers as a sorted list."""
    special = set(int(x) for x in special_ints)
    replacers = set()
    for iwidth in (8, 4, 2, 1, -4, -2, -1):                          # :165
        width = abs(iwidth)
        size = width * 8
        mask = ((1 << size) - 1) & M64                               # (1 << 64) - 1 wraps to all ones in Go
        mutant = (v & mask) if iwidth > 0 else (v | (M64 ^ mask))    # :171 / :175
        for bigendian in (False, True):                              # :185
            if bigendian:
                if width == 1:                                       # :187-189
                    continue
                mutant = swap_int(mutant, width)                     # :190
            for new_v in comp_map_.get(mutant, ()):                  # :192
                new_hi = new_v & (M64 ^ mask)                        # :194
                new_v = new_v & mask                                 # :195
                if new_hi != 0 and (new_hi ^ (M64 ^ mask)) != 0:     # :196-198
                    continue
                if bigendian:
                    new_v = swap_int(new_v, width)                   # :199-201
                if new_v in special:                                 # :202-204
                    continue
                replacers.add((v & (M64 ^ mask)) | new_v)            # :207, :213
    return sorted(replacers)


def shrink_expand_batch(maps, calls, values, special_ints=()):
    """-> (rep_off u64[nq + 1], rep u64[])"""
    off, rep = [0], []
    for c, v in zip(calls, values):
        r = shrink_expand(int(v), maps[int(c)], special_ints)
        rep += r
        off.append(off[-1] + len(r))
    return np.array(off, np.uint64), np.array(rep, np.uint64)
