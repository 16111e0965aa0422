"""Restatement of write_coverage_signal<cover_t> for the three KCOV targets of
include/syzsig.h, the checker of Device.edge_derive / Device.edge_cover with a
target: executor/executor.h:492-528 and :677-706 written out line by line, with
cover_t (pc32) and the body of cover_check (check_x86) as the two parameters the
reference fixes at run time (:595-598) and at build time
(executor_linux.cc:191-204 and the other executors' `return true`).

The compiled reference harness hard-codes is_kernel_64_bit = true on x86_64, so
it reaches the CHECK_X86 target only.  tests/test_target_ref_cpu.py therefore
holds this file to it where it can -- CHECK_X86 word for word against the
oracle and the goldens -- and carries the other two targets over by the
low-word identity (a signal depends on the PC's low 32 bits alone) and by
hand-derived cases.
"""
import numpy as np

M32 = 0xFFFFFFFF
DEDUP_TABLE_SIZE = 8 << 10                                    # :687

PC32, CHECK_X86 = 1, 2                                        # syzsig.h SYZSIG_TARGET_*


def flags_of(target):
    """(pc32, check_x86) of a valid target word."""
    assert target in (0, PC32, CHECK_X86), target
    return bool(target & PC32), bool(target & CHECK_X86)


def hash32(a):                                                # :677 static uint32 hash(uint32 a)
    a = ((a ^ 61) ^ (a >> 16)) & M32                          # :679
    a = (a + (a << 3)) & M32                                  # :680
    a = a ^ (a >> 4)                                          # :681
    a = (a * 0x27d4eb2d) & M32                                # :682
    a = a ^ (a >> 15)                                         # :683
    return a                                                  # :684


def dedup(table, sig):                                        # :693 static bool dedup(uint32 sig)
    for i in range(4):                                        # :695
        pos = (sig + i) % DEDUP_TABLE_SIZE                    # :696
        if table[pos] == sig:                                 # :697
            return True                                       # :698
        if table[pos] == 0:                                   # :699
            table[pos] = sig                                  # :700
            return False                                      # :701
    table[sig % DEDUP_TABLE_SIZE] = sig                       # :704
    return False                                              # :705


def cover_check(pc, pc32, check_x86):
    if pc32:                                                  # executor_linux.cc:191-194 cover_check(uint32)
        return True
    if check_x86:                                             # :198 #if defined(__i386__) || defined(__x86_64__)
        return 0xffffffff80000000 <= pc < 0xffffffffff000000  # :200
    return True                                               # :202


def write_coverage_signal(pcs, pc32, check_x86, table=None, collect_cover=False, dedup_cover=False):
    """One call.  pcs: the call's cover_data as Python ints or an array (below
    2^32 when pc32).  table: the child's dedup_table, updated in place (None: a
    fresh one).  Returns (signals, cover), both lists of u32 as write_output
    saw them, cover None without collect_cover; or None where the reference
    takes doexit(0) (:503) -- the call publishes nothing and the program ends."""
    if table is None:
        table = [0] * DEDUP_TABLE_SIZE
    mask = M32 if pc32 else 0xFFFFFFFFFFFFFFFF                # cover_t
    cover_data = [int(x) for x in pcs]
    assert all(0 <= x <= mask for x in cover_data)
    out = []
    prev = 0                                                  # :499 cover_t prev = 0
    for pc in cover_data:                                     # :500-501
        if not cover_check(pc, pc32, check_x86):              # :502
            return None                                       # :503 doexit(0)
        sig = pc ^ prev                                       # :504 cover_t sig = pc ^ prev
        prev = hash32(pc & M32)                               # :505 hash(uint32): the argument is truncated
        if dedup(table, sig & M32):                           # :506 dedup(uint32)
            continue                                          # :507
        out.append(sig & M32)                                 # :508 write_output(uint32)
    if not collect_cover:                                     # :514
        return out, None
    if dedup_cover:                                           # :518
        cover_data.sort()                                     # :520 std::sort over cover_t
        uniq = []                                             # :521 std::unique
        for x in cover_data:
            if not uniq or uniq[-1] != x:
                uniq.append(x)
        cover_data = uniq
    return out, [x & M32 for x in cover_data]                 # :525-526 write_output(cover_data[i])


def exec_batch(pcs, call_start, call_len, prog_call, target):
    """Every program of a batch, each with a fresh dedup table (one forked
    child), in the shape of oracle.exec_batch: (sigs u32[npc] in pcs indexing,
    zero where nothing is written; sig_cnt per call; completed per program)."""
    pc32, check = flags_of(target)
    pcs = np.asarray(pcs)
    sigs = np.zeros(pcs.size, np.uint32)
    cnt = np.zeros(len(call_len), np.uint32)
    comp = np.zeros(len(prog_call) - 1, np.uint32)
    for p in range(len(prog_call) - 1):
        table = [0] * DEDUP_TABLE_SIZE
        a, b = int(prog_call[p]), int(prog_call[p + 1])
        comp[p] = b - a
        for c in range(a, b):
            s, n = int(call_start[c]), int(call_len[c])
            r = write_coverage_signal(pcs[s:s + n].tolist(), pc32, check, table)
            if r is None:
                comp[p] = c - a
                break
            sigs[s:s + len(r[0])] = r[0]
            cnt[c] = len(r[0])
    return sigs, cnt, comp


def edge_cover(pcs, call_start, call_len, prog_call, completed, target, dedup=True, fill=0):
    """The cover half for every call with a record (c - prog_call[p] <
    completed[p]) in the shape of cover_ref.edge_cover: (cover u32[npc], `fill`
    wherever nothing is written; cover_cnt per call)."""
    pc32, check = flags_of(target)
    pcs = np.asarray(pcs)
    cover = np.full(pcs.size, fill, np.uint32)
    cnt = np.zeros(len(call_len), np.uint32)
    for p in range(len(prog_call) - 1):
        cb = int(prog_call[p])
        for c in range(cb, min(int(prog_call[p + 1]), cb + int(completed[p]))):
            s, n = int(call_start[c]), int(call_len[c])
            r = write_coverage_signal(pcs[s:s + n].tolist(), pc32, check, None, True, dedup)
            assert r is not None, "a completed call passed cover_check"
            cover[s:s + len(r[1])] = r[1]
            cnt[c] = len(r[1])
    return cover, cnt
