"""Executor output regions written by hand, word by word, for
k_ingest_exec_output (csrc/ingest.hip), each with the status
pkg/ipc/ipc.go:328-468 readOutCoverage must give it (no GPU use).

A region is  ncmd, then per record  callIndex, callNum, errno, faultInjected,
signalSize, coverSize, compsSize, signal words, cover words, comparisons
(type, then 2 operand words, or 4 if type & 6 == 6).  The boundary regions
come in pairs: the last region a length or range check of ipc.go accepts and
the first it rejects.  The long programs pass kSeenCalls = 256 calls, where the
kernel keeps "this call has a record" in call_len itself (the sentinel
0xFFFFFFFF) and no longer in LDS.  batch() spreads both among 600 short
programs, three workgroups of 256 threads."""
import functools
from typing import NamedTuple

import numpy as np

OK, ENCMD, EHEADER, EINDEX, ECALLNUM, EDOUBLE, ESIGNAL, ECOVER, ECOMPS, ECOMPTYPE = range(10)
SEEN_CALLS = 256   # kSeenCalls
THREADS = 256      # kIngestThreads: programs per workgroup
NIL_LEN = 0xFFFFFFFF  # kNilLen
NPROG = 600


class Region(NamedTuple):
    name: str
    words: tuple      # u32 words
    ncalls: int       # len(p.Calls)
    status: int       # by hand, with callNum checked
    status_nonum: int  # and without (call_num = NULL skips ipc.go:389-395)


def call_num(i):
    """c.Meta.ID of call i of every program here"""
    return 100 + i % 50


def call_nums(ncalls):
    return np.array([call_num(i) for i in range(ncalls)], np.uint32)


def rec(idx, sig=(), cover=(), comps=(), errno=0, num=None, nsig=None, ncover=None, ncomps=None):
    """one record; comps = the comparison words as written; the three sizes may lie"""
    return [idx, call_num(idx) if num is None else num, errno & 0xFFFFFFFF, 0,
            len(sig) if nsig is None else nsig, len(cover) if ncover is None else ncover,
            len(comps) if ncomps is None else ncomps, *sig, *cover, *[w for c in comps for w in c]]


def _region(name, ncalls, status, *records, ncmd=None, status_nonum=None):
    words = [len(records) if ncmd is None else ncmd] + [w for r in records for w in r]
    return Region(name, tuple(words), ncalls, status, status if status_nonum is None else status_nonum)


@functools.lru_cache(maxsize=None)
def boundaries():
    r = [
        Region("empty", (), 2, ENCMD, ENCMD),                                    # ipc.go:356-359
        _region("ncmd0", 2, OK),
        Region("hdr6", (1, 0, call_num(0), 0, 0, 0, 0), 2, EHEADER, EHEADER),     # :378-383, 6 words left
        _region("hdr7", 2, OK, rec(0)),                                          # 7 words left
        _region("ncmd2_one_record", 2, EHEADER, rec(1, sig=[5, 6]), ncmd=2),     # 0 words left for record 2
        _region("nsig_exact", 2, OK, rec(1, sig=[7, 8, 9])),                     # :403-407
        _region("nsig_plus1", 2, ESIGNAL, rec(1, sig=[7, 8, 9], nsig=4)),
        _region("nsig_exact_after_record", 3, OK, rec(2, sig=[1]), rec(0, sig=[7, 8, 9])),
        _region("ncover_exact", 2, OK, rec(0, sig=[1, 2], cover=[3, 4, 5])),     # :411-415
        _region("ncover_plus1", 2, ECOVER, rec(0, sig=[1, 2], cover=[3, 4, 5], ncover=4)),
        _region("ncover_exact_no_signal", 2, OK, rec(1, cover=[3])),
        _region("comp_type7", 2, OK, rec(0, sig=[1], comps=[[7, 1, 2, 3, 4]])),  # :429-433
        _region("comp_type8", 2, ECOMPTYPE, rec(0, sig=[1], comps=[[8, 1, 2, 3, 4]])),
        _region("comp8_4left", 2, OK, rec(1, sig=[1], comps=[[6, 1, 2, 3, 4]])),  # :434-445, 8-byte operands
        _region("comp8_3left", 2, ECOMPS, rec(1, sig=[1], comps=[[6, 1, 2, 3]])),
        _region("comp4_2left", 2, OK, rec(1, cover=[9], comps=[[4, 1, 2]])),      # 4-byte operands
        _region("comp4_1left", 2, ECOMPS, rec(1, cover=[9], comps=[[4, 1]])),
        _region("comp_second_exact", 2, OK, rec(0, comps=[[0, 1, 2], [5, 1, 2]])),
        _region("comp_no_type_word", 2, ECOMPS, rec(0, comps=[[0, 1, 2]], ncomps=2)),  # :421-424
        _region("idx_last", 4, OK, rec(3, sig=[1])),                             # :384-388
        _region("idx_ncalls", 4, EINDEX, rec(4, sig=[1], num=call_num(3))),
        _region("idx_ncalls_after_record", 4, EINDEX, rec(0, sig=[1, 2]), rec(4)),
        _region("double_after_empty", 2, EDOUBLE, rec(1), rec(0, sig=[4]), rec(1, sig=[5])),  # :396-400
        _region("double", 2, EDOUBLE, rec(0, sig=[4]), rec(0, sig=[5])),
        _region("callnum", 2, ECALLNUM, rec(0, sig=[4]), rec(1, sig=[5], num=call_num(1) + 1), status_nonum=OK),
        _region("errno_negative", 2, OK, rec(0, sig=[4], errno=-1), rec(1, sig=[5], errno=14)),
    ]
    assert len({x.name for x in r}) == len(r)
    return tuple(r)


def _long_records(nc, missing, seed):
    """one record for every call but `missing`, shuffled; signal of idx % 3 words, cover of idx % 2"""
    idx = [i for i in range(nc) if i not in missing]
    order = np.random.default_rng(seed).permutation(len(idx))
    return [rec(idx[j], sig=[idx[j] * 8 + k for k in range(idx[j] % 3)], cover=[0xC0000000 + idx[j]] * (idx[j] % 2),
                errno=11 if idx[j] % 5 == 0 else 0) for j in order]


@functools.lru_cache(maxsize=None)
def long_programs():
    r = []
    for nc in (256, 257, 300):
        missing = {3, 254, 258, 270} & set(range(nc - 1))  # calls 255, 256 and the last one have a record
        r.append(_region(f"long{nc}", nc, OK, *_long_records(nc, missing, nc)))
        r.append(_region(f"long{nc}_no_record", nc, OK))
    for nc in (257, 300):
        recs = _long_records(nc, {3, 256}, nc + 1)
        half = len(recs) // 2
        # call 256 first with an empty signal (non-nil all the same), later again
        r.append(_region(f"long{nc}_double256_empty", nc, EDOUBLE, *recs[:half], rec(256), *recs[half:],
                         rec(256, sig=[1])))
        r.append(_region(f"long{nc}_double256", nc, EDOUBLE, rec(256, sig=[1, 2]), *recs, rec(256, sig=[1, 2])))
    # records for calls 256.. are written, then the program fails
    tail = [rec(i, sig=[i, i + 1]) for i in range(256, 300)]
    r.append(_region("long300_fails_late", 300, EINDEX, rec(255, sig=[9]), *tail, rec(300)))
    r.append(_region("long300_fails_short", 300, EHEADER, *tail, ncmd=len(tail) + 1))
    r.append(_region("long257_fails_signal", 257, ESIGNAL, rec(256, sig=[1]), rec(0, sig=[1, 2], nsig=3)))
    assert len({x.name for x in r}) == len(r)
    return tuple(r)


def _short(p):
    """the 2-call programs between the special ones: good and bad alternate"""
    if p % 2 == 0:
        return _region(f"short{p}", 2, OK, rec(p % 2, sig=[p, p + 1, p + 2], errno=p % 3), rec(1 - p % 2, cover=[p]))
    bad = [(EINDEX, [rec(0, sig=[p]), rec(2)]), (ESIGNAL, [rec(1, sig=[p], nsig=2)]),
           (EDOUBLE, [rec(1, sig=[p]), rec(1)])][p // 2 % 3]
    return _region(f"short{p}", 2, bad[0], *bad[1])


@functools.lru_cache(maxsize=None)
def batch():
    """600 programs: every fifth is the next boundary region or long program, round and round"""
    special = boundaries() + long_programs()
    out, k = [], 0
    for p in range(NPROG):
        if p % 5 == 3:
            out.append(special[k % len(special)])
            k += 1
        else:
            out.append(_short(p))
    return tuple(out)


def arrays(regions, with_call_num=True):
    """(region word arrays, ncalls, call_any, call_num or None) for oracle.ingest_batch and the device"""
    regs = [np.array(r.words, np.uint32) for r in regions]
    ncalls = np.array([r.ncalls for r in regions], np.int64)
    total = int(ncalls.sum())
    call_any = (np.arange(total) % 3 == 0).astype(np.uint8)
    nums = np.concatenate([call_nums(r.ncalls) for r in regions]) if with_call_num else None
    return regs, ncalls, call_any, nums
