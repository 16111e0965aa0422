#!/usr/bin/env python3
"""Time of syzkaller_amd.db.open_db (pkg/db's db.Open on device) beside the
reference's loop restated (tests/db_ref.py: one zlib inflate per record on one
core), in the same process.

    python scripts/time_db.py              # a corpus.db of 10^5 records

The database is synthetic: --n program-like records (lines of serialized
syscalls drawn from 256 templates with random hex arguments, so that DEFLATE
finds the matches it finds in real programs) whose lengths are lognormal with
median 400 bytes and sigma 0.9, clipped to [16, 16384] -- scripts/time_hash.py's
distribution, a few calls to a few hundred -- keyed by hash.String of the
program, written in the Go writer's stream shape at zlib level 9; a tenth of
the records overwrite an earlier key and a fiftieth delete one.  open_db is also
split into its steps (scan, upload, sizing pass, live set, the live values'
inflate), each timed on its own with the device synchronised; medians of --reps
runs after one warm-up.  Prints one JSON line.  Needs the GPU.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus_db(n, seed=1):
    from tests import db_ref as R

    rng = np.random.default_rng(seed)
    names = [b"openat$dir", b"mmap", b"ioctl$KVM_RUN", b"write$binfmt", b"socket$inet6", b"sendmsg$nl_route", b"close",
             b"read$FUSE", b"bpf$PROG_LOAD", b"setsockopt$inet_tcp_int", b"fcntl$dupfd", b"epoll_ctl$EPOLL_CTL_ADD"]
    templates = [b"r%d = %s(0x%x, &(0x7f0000%06x)={0x%x, 0x%x, 0x0, @local}, 0x%x)\n" %
                 (i % 7, names[i % len(names)], i, i * 64, i * 3, i * 5, i) for i in range(256)]
    lens = np.clip(rng.lognormal(np.log(400), 0.9, n), 16, 16384).astype(np.int64)
    recs, keys = [], []
    for i, k in enumerate(lens):
        lines, size = [], 0
        while size < k:
            t = templates[int(rng.integers(256))].replace(b"0x0,", b"0x%x," % int(rng.integers(1 << 16)))
            lines.append(t)
            size += len(t)
        p = b"".join(lines)[: int(k)]
        r = rng.random()
        if keys and r < 0.02:
            recs.append((keys[int(rng.integers(len(keys)))], None, R.SEQ_DELETED))
        elif keys and r < 0.12:
            recs.append((keys[int(rng.integers(len(keys)))], p, i))
        else:
            keys.append(hashlib.sha1(p).hexdigest().encode())
            recs.append((keys[-1], p, i))
    return R.serialize_db(1, recs)


def wall(reps, fn):
    t = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    from syzkaller_amd import db, hashing
    from syzkaller_amd.device import Device
    from tests import db_ref as R

    dev = Device(0)
    data = corpus_db(a.n)
    sync = torch.cuda.synchronize
    ref = []
    ms_ref = wall(1, lambda: ref.__setitem__(slice(None), [R.deserialize_db(data)]))
    version, records, unc, ended = ref[0]
    got = []
    ms_open = wall(a.reps, lambda: (got.__setitem__(slice(None), [db.open_db(dev, data)]), sync()))
    d = got[0]
    assert (d.version, d.uncompacted, d.ended, d.Len()) == (version, unc, ended, len(records))
    assert d.records() == records, "device and reference disagree"
    # the steps
    st = {}
    sc = []
    st["scan_ms"] = wall(a.reps, lambda: sc.__setitem__(slice(None), [db.scan(data)]))
    _, _, ko, kl, sq, vo, vl = sc[0]
    up = []
    st["upload_ms"] = wall(a.reps, lambda: (up.__setitem__(slice(None), [hashing._bytes_tensor(dev, data)]), sync()))
    src = up[0]
    d_vo = torch.from_numpy(vo.view(np.int64)).to(dev.dev)
    d_vl = torch.from_numpy(vl.view(np.int32)).to(dev.dev)
    st["sizing_pass_ms"] = wall(a.reps, lambda: db.inflate(dev, src, d_vo, d_vl, sizing=True))
    sizing_stats = db.inflate_stats(dev)
    sigs = torch.from_numpy(db._hex_to_sigs(data, ko, kl)).to(dev.dev)
    d_sq = torch.from_numpy(sq.view(np.int64)).to(dev.dev)
    lv = []
    st["hex_keys_ms"] = wall(a.reps, lambda: db._hex_to_sigs(data, ko, kl))
    st["live_set_ms"] = wall(a.reps, lambda: lv.__setitem__(slice(None), [db.db_live(dev, sigs, d_sq, sq.size)]))
    rows = torch.nonzero(lv[0][0]).flatten()
    l_vo, l_vl = d_vo[rows], d_vl[rows]
    out = []
    st["inflate_live_ms"] = wall(a.reps, lambda: out.__setitem__(slice(None), [db.inflate(dev, src, l_vo, l_vl)]))
    st["inflate_all_ms"] = wall(a.reps, lambda: db.inflate(dev, src, d_vo, d_vl))
    all_stats = db.inflate_stats(dev)
    st["hash_live_ms"] = wall(a.reps, lambda: hashing.hash_batch(dev, out[0][0], out[0][1]))
    inflated = sum(len(v) for v, _ in records.values())
    compressed = int(vl.sum())
    print(json.dumps({"records": int(sq.size), "live": d.Len(), "file_bytes": len(data), "compressed_bytes": compressed,
                      "live_inflated_bytes": inflated, "reps": a.reps, "db_ref_loop_ms": round(ms_ref, 2),
                      "open_db_ms": round(ms_open, 2), "ref_over_device": round(ms_ref / ms_open, 2),
                      "open_db_inflated_MBps": round(inflated / (ms_open * 1e-3) / 1e6, 1),
                      "db_ref_inflated_MBps": round(inflated / (ms_ref * 1e-3) / 1e6, 1),
                      "inflate_stats_all": dict(zip(("short", "long", "stored", "fixed", "dynamic"), all_stats)),
                      "inflate_stats_sizing": dict(zip(("short", "long", "stored", "fixed", "dynamic"), sizing_stats)),
                      **{k: round(v, 3) for k, v in st.items()}}))


if __name__ == "__main__":
    main()
