#!/usr/bin/env python3
"""Time of one batch of poll replies on the fuzzer (syzsig_fuzzer_poll_res_dev)
beside the per-Serial way of applying it that the set operations give --
syzsig_deserialize_dev + syzsig_merge into maxSignal for a MaxSignal,
syzsig_deserialize_dev + two syzsig_merge for an input -- in one process, on
the same device data.

    python scripts/time_poll_res.py                   # the reply and the connect shape
    python scripts/time_poll_res.py --shapes reply --inputs 100

Shapes: `reply` = one PollRes: a --max-entries MaxSignal and --inputs inputs
of ~--entries entries against a --max-signal element maxSignal and a
--corpus-signal element corpusSignal; `connect` = what a fresh fuzzer (nil
sets) receives after Connect: a 10M-entry MaxSignal and 4096 inputs.
Times are HIP events around the call (the calls end synchronised, so they span
its host round trips), the median of --reps runs after one warm-up, each run
on fresh clones of the sets.  `staged_ms` is signal.fuzzer_poll_res from host
arrays (concatenation into page-locked staging and the upload included).
Algorithmic bytes: 5 B per entry in + 8 B per winner (an element's last entry
in its segment) per table it is merged into, beside a plain device copy's
bandwidth (syzsig_copy_bw_dev).  Prints one JSON line per shape.  Needs the GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from syzkaller_amd import _lib  # noqa: E402
from syzkaller_amd import signal as S  # noqa: E402
from syzkaller_amd.device import Device, _p  # noqa: E402


def achievable_bw(dev, nbytes=1 << 30, reps=5):
    src = torch.ones(nbytes // 8, dtype=torch.int64, device=dev.dev)
    dst = torch.empty_like(src)
    ms = [dev.copy_bw(dst, src, nbytes) for _ in range(reps + 1)][1:]
    return 2 * nbytes / (float(np.median(ms)) * 1e-3) / 1e9


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):
        prep = fn(None)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(prep)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms[1:])), out


def make_shape(dev, name, a):
    """(seg lengths, kinds, elems, prios on device, corpusSignal or None, maxSignal or None)"""
    g = torch.Generator(device=dev.dev)
    g.manual_seed(1)
    rng = np.random.default_rng(1)
    U = 1 << 24
    if name == "connect":
        lens = [10_000_000] + rng.integers(a.entries * 3 // 4, a.entries + 1, size=4096).tolist()
        n_max, n_corpus = 0, 0
    else:
        lens = [a.max_entries] + rng.integers(a.entries * 3 // 4, a.entries + 1, size=a.inputs).tolist()
        n_max, n_corpus = a.max_signal, a.corpus_signal
    kinds = np.array([_lib.SYZSIG_SEG_MAXSIGNAL] + [_lib.SYZSIG_SEG_INPUT] * (len(lens) - 1), np.uint8)
    n = int(sum(lens))
    elems = torch.randint(0, U, (n,), generator=g, device=dev.dev, dtype=torch.int32)
    prios = torch.randint(0, 4, (n,), generator=g, device=dev.dev, dtype=torch.int8)
    cs = ms = None
    if n_max:
        perm = torch.randperm(U, generator=g, device=dev.dev)[:n_max].to(torch.int32)
        ms = dev.deserialize(perm, torch.randint(0, 4, (n_max,), generator=g, device=dev.dev, dtype=torch.int8))
        cs = dev.deserialize(perm[:n_corpus].contiguous(),
                             torch.randint(0, 4, (n_corpus,), generator=g, device=dev.dev, dtype=torch.int8))
    return lens, kinds, elems, prios, cs, ms


def run_shape(dev, name, a, bw):
    eng, L = dev.eng, dev.eng.L
    lens, kinds, elems, prios, cs0, ms0 = make_shape(dev, name, a)
    off_h = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(np.array(lens, np.int64), out=off_h[1:])
    off, kind = torch.from_numpy(off_h).to(dev.dev), torch.from_numpy(kinds).to(dev.dev)
    n = int(off_h[-1])

    def fresh():
        return (cs0.clone() if cs0 is not None else S.Signal(None, eng),
                ms0.clone() if ms0 is not None else S.Signal(None, eng))

    def batch(prep):
        if prep is None:
            return fresh()
        cs, ms = prep
        dev.poll_res(off, kind, elems, prios, cs, ms)
        return cs.Len(), ms.Len(), dev.poll_res_stats()

    e_h, p_h = elems.cpu().numpy().view(np.uint32), prios.cpu().numpy()
    sers = [S.Serial(e_h[x:y], p_h[x:y]) for x, y in zip(off_h[:-1].tolist(), off_h[1:].tolist())]

    def staged(prep):
        if prep is None:
            return fresh()
        cs, ms = prep
        S.fuzzer_poll_res(cs, ms, sers[0], sers[1:], eng)
        return cs.Len(), ms.Len()

    def loop(prep):  # fuzzer.go:344-350 with the set operations, Serial after Serial
        if prep is None:
            return fresh()
        cs, ms = prep
        ch, mh = ctypes.c_void_p(cs.handle.value or 0), ctypes.c_void_p(ms.handle.value or 0)
        for i, (x, y) in enumerate(zip(off_h[:-1].tolist(), off_h[1:].tolist())):
            d = ctypes.c_void_p()
            S.check(L.syzsig_deserialize_dev(eng.h, _p(elems[x:y]), _p(prios[x:y]), y - x, ctypes.byref(d)))
            if L.syzsig_len(d):
                if kinds[i] == _lib.SYZSIG_SEG_INPUT:
                    S.check(L.syzsig_merge(eng.h, ctypes.byref(ch), d))
                S.check(L.syzsig_merge(eng.h, ctypes.byref(mh), d))
            L.syzsig_set_free(d)
        if ch.value and cs.is_nil():
            cs._h = ch
        if mh.value and ms.is_nil():
            ms._h = mh
        return cs.Len(), ms.Len()

    b_ms, (b_cl, b_ml, stats) = timed(batch, a.reps)
    s_ms, (s_cl, s_ml) = timed(staged, a.reps)
    l_ms, (l_cl, l_ml) = timed(loop, a.reps)
    if (b_cl, b_ml) != (l_cl, l_ml) or (s_cl, s_ml) != (l_cl, l_ml):
        raise SystemExit(f"{name}: the batch and the loop disagree: {(b_cl, b_ml)} {(s_cl, s_ml)} {(l_cl, l_ml)}")
    # winners per kind: the distinct (segment, element) pairs
    seg = torch.repeat_interleave(torch.arange(len(lens), device=dev.dev), torch.from_numpy(np.array(lens)).to(dev.dev))
    pairs = torch.unique((seg << 32) | (elems.to(torch.int64) & 0xFFFFFFFF))
    w_max = int(((pairs >> 32) == 0).sum())
    w_in = int(pairs.numel()) - w_max
    assert n - (w_max + w_in) == stats[2]
    nbytes = 5 * n + 8 * (w_max + 2 * w_in)
    gbps = nbytes / (b_ms * 1e-3) / 1e9
    return {"shape": name, "segments": len(lens), "entries": n, "max_serial_entries": lens[0],
            "max_signal": 0 if ms0 is None else len(ms0), "corpus_signal": 0 if cs0 is None else len(cs0),
            "max_signal_after": b_ml, "corpus_signal_after": b_cl, "winners": w_max + w_in,
            "paths": dict(zip(("short", "long", "losers", "scratch_bytes"), stats)), "reps": a.reps,
            "batch_ms": round(b_ms, 3), "staged_ms": round(s_ms, 3), "per_serial_loop_ms": round(l_ms, 3),
            "loop_over_batch": round(l_ms / b_ms, 2), "loop_over_staged": round(l_ms / s_ms, 2),
            "entries_per_s": round(n / (b_ms * 1e-3)), "algorithmic_bytes": nbytes, "achieved_GBps": round(gbps, 2),
            "copy_bw_GBps": round(bw, 1), "fraction_of_copy_bw": round(gbps / bw, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reply,connect")
    ap.add_argument("--inputs", type=int, default=100)
    ap.add_argument("--entries", type=int, default=2040)
    ap.add_argument("--max-entries", type=int, default=100_000)
    ap.add_argument("--max-signal", type=int, default=10_000_000)
    ap.add_argument("--corpus-signal", type=int, default=9_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = Device(0)
    bw = achievable_bw(dev)
    for name in a.shapes.split(","):
        print(json.dumps(run_shape(dev, name, a, bw)), flush=True)


if __name__ == "__main__":
    main()
