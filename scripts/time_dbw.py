#!/usr/bin/env python3
"""Time of pkg/db's write side on device (syzkaller_amd.db.DB.compact: every
live value compressed, framed and downloaded) beside the reference's loop
restated (tests/dbw_ref.py with db_ref.go_stream: zlib level 9 per record on one
core), in the same process.

    python scripts/time_dbw.py              # scripts/time_db.py's corpus.db of 10^5 records
    python scripts/time_dbw.py --sizes-only # the compressed totals alone: no device needed

The device side is compact() end to end, and split into its steps, each timed
on its own with the device synchronised: apply (every live record saved again
into an empty database: the sort and the no-op rules), deflate (the sizing call
alone, and the full call), frames, download; medians of --reps runs after one
warm-up.  The reference side runs once.  It also prints the total compressed
bytes of the live values for this library's compressor (through
syzsig_deflate_host, whose bytes are the device's), zlib level 9, zlib level 1
with Z_FIXED, and Z_HUFFMAN_ONLY.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.time_db import corpus_db, wall  # noqa: E402


def zlen(v, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return len(c.compress(v) + c.flush())


def sizes(vals):
    from syzkaller_amd import db

    raw = sum(len(v) for v in vals)
    out = {"raw_bytes": raw, "device_bytes": sum(len(db.deflate_host(v)) for v in vals),
           "zlib9_bytes": sum(zlen(v, 9, zlib.Z_DEFAULT_STRATEGY) for v in vals),
           "zlib1_fixed_bytes": sum(zlen(v, 1, zlib.Z_FIXED) for v in vals),
           "huffman_only_bytes": sum(zlen(v, 9, zlib.Z_HUFFMAN_ONLY) for v in vals)}
    out.update({k.replace("_bytes", "_ratio"): round(v / raw, 4) for k, v in out.items() if k != "raw_bytes"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes-only", action="store_true")
    a = ap.parse_args()
    from tests import db_ref as R
    from tests import dbw_ref as W

    data = corpus_db(a.n)
    version, records, unc, _ = R.deserialize_db(data)
    vals = [v for v, _ in records.values()]
    res = {"records": unc, "live": len(records), **sizes(vals)}
    if a.sizes_only:
        print(json.dumps(res))
        return
    import torch

    from syzkaller_amd import db
    from syzkaller_amd.device import Device

    dev = Device(0)
    sync = torch.cuda.synchronize
    ref = W.RefDB(version, records, unc)
    t0 = time.perf_counter()
    ref_file = ref.compact()
    ms_ref = (time.perf_counter() - t0) * 1e3
    d = db.open_db(dev, data)
    out = []
    ms_compact = wall(a.reps, lambda: out.__setitem__(slice(None), [d.compact()]))
    again = R.deserialize_db(out[0])
    assert again[:3] == (version, records, len(records)), "the compacted file does not read back"
    st = {}
    off = d.vals[1]
    lo, ln = off[:-1], (off[1:] - off[:-1]).to(torch.int32)
    seqs = d._i64(d.seqs)
    empty = db.open_db(dev, b"")
    none = (empty.keys, seqs[:0], empty.vals)
    st["apply_ms"] = wall(a.reps, lambda: db.db_apply(dev, *none, d.keys, seqs, d.vals))
    st["deflate_sizing_ms"] = wall(a.reps, lambda: db.deflate(dev, d.vals[0], lo, ln, sizing=True))
    streams = []
    st["deflate_ms"] = wall(a.reps, lambda: streams.__setitem__(slice(None), [db.deflate(dev, d.vals[0], lo, ln)]))
    stats = db.deflate_stats(dev)
    recs = []
    st["frames_ms"] = wall(a.reps, lambda: recs.__setitem__(slice(None), [db.db_records(dev, d.keys, seqs, streams[0])]))
    st["download_ms"] = wall(a.reps, lambda: (recs[0][0].cpu().numpy().tobytes(), sync()))
    assert int(streams[0][1][-1]) == res["device_bytes"], "device and host compressors disagree"
    res.update({"reps": a.reps, "file_bytes": len(out[0]), "ref_file_bytes": len(ref_file),
                "dbw_ref_compact_ms": round(ms_ref, 2), "compact_ms": round(ms_compact, 2),
                "ref_over_device": round(ms_ref / ms_compact, 2),
                "compact_raw_MBps": round(res["raw_bytes"] / (ms_compact * 1e-3) / 1e6, 1),
                "deflate_stats": dict(zip(("short", "long", "stored", "fixed"), stats)),
                **{k: round(v, 3) for k, v in st.items()}})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
