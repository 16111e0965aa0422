#!/usr/bin/env python3
"""Device time of syzsig_triage_items_dev beside syzsig_edge_cover_dev with
SYZSIG_COVER_DEDUP over the same calls' ranges (the same segmented sort-unique
without the corpusSignal probes), in one process.

    python scripts/time_triage_items.py                  # 4096 x 64 x 4096 records, 10M-element corpusSignal,
                                                         # 1 % and 100 % of the calls flagged
    python scripts/time_triage_items.py --programs 1 --calls 64 --records 262143 --rates 1.0   # the long path

The records are uniform draws from a universe of --universe elements, of which
corpusSignal holds --corpus (prios 0..3, as the calls'), so a call's records
are nearly all distinct and about corpus / universe of them are probed and
found.  Times are HIP events around the whole call (its host round trips
included): the median of --reps after a warm-up (the sizing call);
nil_corpus_ms is the same call without a corpusSignal, so without probes.  The
algorithmic traffic is 4 B per record in, 8 B per distinct element probed, 4 B
per inputSignal element out and 5 B per newSignal element out; probe_bucket_bytes
is what the probes read if each is one 16-B bucket.  Prints one JSON line.
Needs the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from syzkaller_amd import _lib  # noqa: E402
from syzkaller_amd.device import Device, call_layout  # noqa: E402
from time_cover import achievable_bw  # noqa: E402


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), r


def time_rate(dev, sigs, pcs, cs, cl, prio, pidx, completed, corpus, rate, reps, seed):
    ncalls = cl.numel()
    g = torch.Generator(device=dev.dev).manual_seed(seed)
    new = (torch.rand(ncalls, device=dev.dev, generator=g) < rate).to(torch.uint8) if rate < 1 else \
        torch.ones(ncalls, dtype=torch.uint8, device=dev.dev)
    try:  # the sizing call: the totals, and the warm-up
        dev.triage_items(sigs, cs, cl, prio, new, corpus_signal=corpus, caps=(0, 0, 0))
        caps = (0, 0, 0)
    except _lib.SyzsigError as e:
        caps = e.needed
    dev.triage_items(sigs, cs, cl, prio, new, corpus_signal=corpus, caps=caps)  # the output buffers' allocation
    ms, r = timed(lambda: dev.triage_items(sigs, cs, cl, prio, new, corpus_signal=corpus, caps=caps), reps)
    st = dev.triage_items_stats()
    # the same call against a nil corpusSignal: the sort-unique and both outputs, no probe
    nil_caps = (caps[0], caps[1], caps[1])
    dev.triage_items(sigs, cs, cl, prio, new, caps=nil_caps)
    nil_ms, _ = timed(lambda: dev.triage_items(sigs, cs, cl, prio, new, caps=nil_caps), reps)
    # the yardstick: the flagged calls' ranges alone (an unflagged call is a segment of no keys)
    ycl = cl * new.to(torch.int32)
    cover = torch.empty(pcs.numel(), dtype=torch.int32, device=dev.dev)
    dev.edge_cover(pcs, cs, ycl, pidx, completed, cover=cover)
    yms, (_, ycnt) = timed(lambda: dev.edge_cover(pcs, cs, ycl, pidx, completed, cover=cover), reps)
    recs = int(ycl.to(torch.int64).sum().item())
    n_in, n_new = r["input_elems"].numel(), r["elems"].numel()
    assert int(ycnt.to(torch.int64).sum().item()) == n_in  # the same survivors
    nbytes = 4 * recs + 8 * st[3] + 4 * n_in + 5 * n_new
    return {"flag_rate": rate, "items": st[0], "long_items": st[1], "merge_passes": st[2], "records": recs,
            "ms": round(ms, 4), "nil_corpus_ms": round(nil_ms, 4), "keys_per_s": round(recs / (ms * 1e-3), 1), "probes": st[3], "input_elems": n_in,
            "new_elems": n_new, "algorithmic_bytes": nbytes, "probe_bucket_bytes": 16 * st[3],
            "achieved_GBps": round(nbytes / (ms * 1e-3) / 1e9, 1), "edge_cover_ms": round(yms, 4),
            "ratio_to_edge_cover": round(ms / yms, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--programs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--corpus", type=int, default=10_000_000)
    ap.add_argument("--universe", type=int, default=1 << 25)
    ap.add_argument("--rates", default="0.01,1.0")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = Device(0)
    ncalls = a.programs * a.calls
    g = torch.Generator(device=dev.dev).manual_seed(1)
    cl = torch.full((ncalls,), a.records, dtype=torch.int32, device=dev.dev)
    cs = call_layout(cl)
    sigs = torch.randint(0, a.universe, (ncalls * a.records,), dtype=torch.int32, device=dev.dev, generator=g)
    pcs = sigs.to(torch.int64) | -(1 << 32)  # executor PCs: the upper word all ones
    prio = torch.randint(0, 4, (ncalls,), dtype=torch.uint8, device=dev.dev, generator=g)
    pidx = (torch.arange(a.programs + 1, dtype=torch.int32, device=dev.dev) * a.calls).contiguous()
    completed = torch.full((a.programs,), a.calls, dtype=torch.int32, device=dev.dev)
    ce = torch.randperm(a.universe, device=dev.dev, generator=g)[: a.corpus].to(torch.int32).contiguous()
    cp = torch.randint(0, 4, (a.corpus,), dtype=torch.int8, device=dev.dev, generator=g)
    corpus = dev.deserialize(ce, cp)
    del ce, cp
    res = {"shape": [a.programs, a.calls, a.records], "tile": _lib.SYZSIG_ITEMS_TILE,
           "long_segment_path": a.records > _lib.SYZSIG_ITEMS_TILE, "corpus_len": corpus.Len(),
           "universe": a.universe, "reps": a.reps, "lib": os.path.basename(_lib.LIB_PATH), "runs": []}
    for i, rate in enumerate(float(x) for x in a.rates.split(",")):
        res["runs"].append(time_rate(dev, sigs, pcs, cs, cl, prio, pidx, completed, corpus, rate, a.reps, 2 + i))
    res["achievable_bw_GBps"] = round(achievable_bw(dev), 1)
    for r in res["runs"]:
        r["fraction_of_achievable"] = round(r["achieved_GBps"] / res["achievable_bw_GBps"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
