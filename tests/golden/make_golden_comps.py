"""Generate the comparison-output golden vectors from the REFERENCE executor itself.

Run in the build container (needs /root/reference and `make -C oracle ref`):
    python tests/golden/make_golden_comps.py [fixture names]
Inputs are synthetic KCOV_TRACE_CMP buffers; expected outputs are the records
written by the reference's own handle_completion with flag_collect_comps
(executor/executor.h:576-593: std::sort + std::unique through
kcov_comparison_t's operators :861-875, ignore() executor_linux.cc:221-253,
write() executor.h:823-859), compiled from its sources by oracle/Makefile and
run in the harness's comps mode with the output region mapped at OUT_START.
Fixtures tests/golden/comps/<name>.npz, plain arrays (allow_pickle=False):
  comps u64[n, 4] (type, arg1, arg2, pc), call_start u64[] (in records), call_len u32[],
  call_failed u8[], prog_call u32[nprog + 1], out_start u64 (scalar: the address the harness reported),
  exp_words u32[5 n] (call c's words at 5 * call_start[c]..+exp_out_words[c]; 0 elsewhere),
  exp_out_words u32[], exp_comps_cnt u32[] (the records' comps_size), exp_completed u32[nprog],
  exp_status u32[nprog] (the child's exit status: 67 = kFailStatus after fail("too many comparisons")),
  regions u32[], region_off u64[nprog + 1] (the raw output regions as the executor wrote them)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from syzkaller_amd import _lib, synth  # noqa: E402

T = _lib.SYZSIG_COMPS_TILE
# executor_linux.cc:61: the executor maps its output region at 0x1b2bc20000 + (1 << 20) * (pid % 128)
OUT_START = 0x1b2bc20000
OUT_END = OUT_START + (16 << 20)  # executor_linux.cc:231, inclusive (:232)
KM0, KM1 = 0xffff880000000000, 0xffff890000000000
PC = 0xffffffff81000000
LENGTHS = [0, 1, 2, T - 1, T, T + 1, 2 * T + 3]
SIGN_VALUES = [0x7f, 0x80, 0xff, 0x7fff, 0x8000, 0x7fffffff, 0x80000000]
ABOVE_SIZE = {0: 0x100, 2: 0x10000, 4: 0x100000000}  # the lowest bit above the operand of that size


M64 = (1 << 64) - 1


def around(v):
    return [(v - 1) & M64, v, (v + 1) & M64]


POINTERS = around(OUT_START) + around(OUT_END) + around(KM0) + around(KM1)


def recs(rows):
    """rows of (type, arg1, arg2) -> u64[n, 4] with a different pc per row"""
    a = np.array([(t, a1, a2, PC + 5 * i) for i, (t, a1, a2) in enumerate(rows)], np.uint64)
    return a.reshape(-1, 4)


def edge_calls():
    """The hand-made calls, in this order (tests/test_golden_comps_cpu.py names them by index)."""
    calls = []
    # 0: every type 0..7
    calls.append([(t, 0x1234 + t, 0x77) for t in range(8)])
    # 1: bits above bit 31 of type next to the same low word without them; operator< orders on all 64 bits,
    #    write() emits the low word
    calls.append([(0x100000002, 5, 6), (2, 7, 8), (2, 5, 6), (0x8000000000000004, 9, 10), (4, 9, 10),
                  (0x100000006, 0x1122334455667788, 1), (6, 0x1122334455667788, 1), (0x700000000, 3, 4)])
    # 2: records equal except for pc (three rows, two pcs)
    calls.append([(4, 10, 11), (4, 10, 11), (4, 10, 11), (6, 10, 11), (6, 10, 11)])
    # 3: operands with bit 63 set, and operands that differ only in their high 32 bits
    calls.append([(6, 0x8000000000000001, 5), (6, 0x0000000100000001, 5), (6, 1, 5), (6, 0xffffffff00000001, 5),
                  (6, 5, 0x8000000000000001), (6, 5, 0x0000000100000001), (6, 5, 1),
                  (6, 0xffffffffffffffff, 0x8000000000000000), (7, 0x8000000000000000, 0xffffffffffffffff),
                  (4, 0x8000000000000001, 5), (4, 0x0000000100000001, 5), (4, 1, 5)])
    # 4: sizes 1, 2, 4 (with and without CONST): the values at the sign boundaries, on either side
    rows = []
    for size in (0, 2, 4):
        for t in (size, size | 1):
            for v in SIGN_VALUES:
                rows += [(t, v, 1), (t, 1, v)]
    calls.append(rows)
    # 5: pairs that differ only in bits above the operand size: std::unique keeps both, write() makes them equal
    rows = []
    for size in (0, 2, 4):
        hi = ABOVE_SIZE[size]
        for v in (0xfe, 0x8000, 0x80000000, 0x7f):
            rows += [(size, v, 1), (size, v | hi, 1), (size, 1, v), (size, 1, v | hi), (size, v | hi << 3, v | hi)]
    calls.append(rows)
    # 6: ignore(), the zero rule: arg1 == 0 with and without CONST, for every type
    rows = []
    for t in range(8):
        rows += [(t, 0, 0), (t, 0, 5), (t, 5, 0)]
    calls.append(rows)
    # 7: ignore(), SIZE8: every pointer boundary at -1, 0, +1 in arg1 and in arg2 against a plain value, against 0
    #    (the kptr && other == 0 rules), and against each other (kptr1 && kptr2; out region first)
    rows = []
    for t in (6, 7):
        for v in POINTERS:
            rows += [(t, v, 1), (t, 1, v), (t, v, 0), (t, 0, v)]
        for v in around(KM0) + around(KM1):
            for w in around(KM0) + around(KM1):
                rows.append((t, v, w))
    calls.append(rows)
    # 8: the same operands under the sizes 1, 2, 4: none of the pointer rules apply
    rows = []
    for t in (0, 1, 2, 3, 4, 5):
        for v in POINTERS:
            rows += [(t, v, 1), (t, 1, v), (t, v, 0), (t, 0, v)]
        rows += [(t, KM0, KM1), (t, KM0 + 1, KM1 - 1)]
    calls.append(rows)
    # 9: every record ignored, past one tile: zeros, output-region addresses, kernel pointers
    pool = [(0, 0, 0), (1, 0, 9), (7, 0, 9), (6, OUT_START + 8, 3), (6, 3, OUT_END - 8), (6, KM0 + 16, KM1 - 16),
            (6, KM0 + 16, 0), (6, 0, KM1 - 16), (7, OUT_START, OUT_END)]
    calls.append([pool[(i * 7) % len(pool)] for i in range(T + 1)])
    # 10: one record repeated past one tile (the pcs differ)
    calls.append([(4, 0x11223344, 0x80000001)] * (T + 5))
    return [recs(c) for c in calls]


def bad_type_calls():
    """type's low word above 7 (the reference writes it, ipc.go:429-433 rejects it later); every call of this
    program has such a record that ignore() keeps.  Low bits 6 set: five words."""
    return [recs([(8, 1, 2)]),
            recs([(2, 1, 2), (0x10, 3, 4), (4, 5, 6)]),
            recs([(0xf, 0x1122334455667788, 2), (0xffffffff, 3, 4), (0x100000009, 5, 6), (0xfffffff8, 0x1fe, 7)])]


def small_pc(comps):
    comps[:, 3] = np.uint64(PC) + (np.arange(comps.shape[0], dtype=np.uint64) % np.uint64(13))
    return comps


def pack(programs):
    comps, cs, cl, cf, pc, pos = [], [], [], [], [0], 0
    for prog in programs:
        for failed, r in prog:
            r = np.asarray(r, np.uint64).reshape(-1, 4)
            comps.append(r)
            cs.append(pos)
            cl.append(r.shape[0])
            cf.append(int(failed))
            pos += r.shape[0]
        pc.append(pc[-1] + len(prog))
    return dict(comps=np.concatenate(comps) if comps else np.empty((0, 4), np.uint64), call_start=np.array(cs, np.uint64),
                call_len=np.array(cl, np.uint32), call_failed=np.array(cf, np.uint8), prog_call=np.array(pc, np.uint32))


def expected(fx, programs):
    kw = dict(mode="comps", out_addr=OUT_START, info=True)
    ref, inf = O.run_reference_executor(programs, **kw)
    regions, inf2 = O.run_reference_executor(programs, raw=True, **kw)
    assert inf["out_start"] == inf2["out_start"] == OUT_START and inf["status"] == inf2["status"]
    n = fx["call_len"].size
    words = np.zeros(5 * fx["comps"].shape[0], np.uint32)
    nw, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    comp = np.zeros(len(programs), np.uint32)
    for p, (completed, calls) in enumerate(ref):
        comp[p] = completed
        for idx, _e, w, k in calls:
            c = int(fx["prog_call"][p]) + idx
            s = 5 * int(fx["call_start"][c])
            assert w.size <= 5 * int(fx["call_len"][c])
            words[s: s + w.size] = w
            nw[c], cnt[c] = w.size, k
    off = np.concatenate([[0], np.cumsum([r.size for r in regions])]).astype(np.uint64)
    return dict(out_start=np.uint64(inf["out_start"]), exp_words=words, exp_out_words=nw, exp_comps_cnt=cnt,
                exp_completed=comp, exp_status=np.array(inf["status"], np.uint32),
                regions=np.concatenate(regions), region_off=off)


def main(only=None):
    out = {}
    # 1. the hand-made edges (one program), and the calls with a type above 7 (a program of their own: the
    #    parse of a region stops at the first of them)
    edges = edge_calls()
    out["edges"] = [[(i % 4 == 2, r) for i, r in enumerate(edges)], [(False, r) for r in bad_type_calls()]]
    # 2. seeded segments at every length class of the segmented sort: three programs, the lengths in two orders
    a, st = synth.comparisons(41, LENGTHS, OUT_START)
    b, st2 = synth.comparisons(42, LENGTHS[::-1], OUT_START, pool=12)
    small_pc(a), small_pc(b)
    seg_a = [(False, a[int(s): int(s) + n]) for s, n in zip(st, LENGTHS)]
    seg_b = [(i == 1, b[int(s): int(s) + n]) for i, (s, n) in enumerate(zip(st2, LENGTHS[::-1]))]
    out["segments"] = [seg_a[:4], seg_a[4:], seg_b]
    # 3. the longest call the executor takes: 65535 records (8 + 32 n == 8 kCoverSize - 24)
    c, _ = synth.comparisons(43, [65535], OUT_START)
    out["long"] = [[(False, small_pc(c))]]
    # 4. one more: fail("too many comparisons"), executor.h:581-582.  The call before it keeps its record;
    #    the next program runs.
    many = np.zeros((65536, 4), np.uint64)
    many[:, 0], many[:, 1], many[:, 2] = 4, 1 + np.arange(65536) % 5, 7
    small_pc(many)
    out["toomany"] = [[(False, recs([(4, 1, 7), (2, 3, 4)])), (False, many), (False, recs([(4, 1, 7)]))],
                      [(False, many[:65535])]]
    os.makedirs(os.path.join(HERE, "comps"), exist_ok=True)
    for name, programs in out.items():
        if only and name not in only:
            continue
        fx = pack(programs)
        fx.update(expected(fx, programs))
        path = os.path.join(HERE, "comps", name + ".npz")
        np.savez_compressed(path, **fx)
        print(f"{name}: {len(programs)} programs, {fx['call_len'].size} calls, {fx['comps'].shape[0]} records, "
              f"{int(fx['exp_comps_cnt'].sum())} written, completed {fx['exp_completed'].tolist()}, "
              f"status {fx['exp_status'].tolist()}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:] or None)
