"""CPU: bench.py's measurement plumbing -- which PMC summary a line's
roofline.traffic may come from (the same workload, and a profiled chain time
within 15 % of the line's own), and the trace-distribution switch of the
headline (SURVEY.md 8(d)'s global walk by default)."""
import json
import os

import numpy as np
import pytest


def _summary(root, name, cfg, kernels, created):
    d = os.path.join(root, "profiles", name)
    os.makedirs(d)
    with open(os.path.join(d, "summary.json"), "w") as f:
        json.dump({"bench_config": cfg, "created": created, "kernels": kernels}, f)


def test_pmc_traffic_matches_workload_and_time(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    cfg = {"workload": "w1"}
    k = {"syz::k_a": {"avg_ms": 1.0, "traffic_bytes": 5e9}, "syz::k_b<4u>": {"avg_ms": 0.5, "traffic_bytes": 1e9}}
    _summary(str(tmp_path), "old", cfg, k, 1.0)
    _summary(str(tmp_path), "other", {"workload": "w2"}, k, 3.0)
    b, src, note = bench.pmc_traffic(["syz::k_a", "syz::k_b"], cfg, ("workload",), expect_ms=1.5)
    assert b == pytest.approx(6e9) and src == os.path.join("profiles", "old", "summary.json") and note is None
    # a newer summary of the same workload wins ...
    k2 = {"syz::k_a": {"avg_ms": 1.2, "traffic_bytes": 4e9}, "syz::k_b": {"avg_ms": 0.4, "traffic_bytes": 1e9}}
    _summary(str(tmp_path), "new", cfg, k2, 2.0)
    b, src, _ = bench.pmc_traffic(["syz::k_a", "syz::k_b"], cfg, ("workload",), expect_ms=1.5)
    assert b == pytest.approx(5e9) and "new" in src
    # ... unless its profiled chain is more than 15 % off the line's own time
    b, src, note = bench.pmc_traffic(["syz::k_a", "syz::k_b"], cfg, ("workload",), expect_ms=1.0)
    assert b is None and src is None and "profiled chain" in note
    # no summary of the workload at all
    b, src, note = bench.pmc_traffic(["syz::k_a"], {"workload": "w3"}, ("workload",), expect_ms=1.0)
    assert b is None and note == "no PMC summary of this workload"


def test_options_plain_and_full(monkeypatch):
    import bench

    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


class _Set:
    """What dump_outputs needs of a signal.Signal: Serialize() in table order."""

    def __init__(self, elems, prios):
        from syzkaller_amd import signal as S

        self.ser = S.Serial(elems, prios)

    def Serialize(self):
        return self.ser


def test_dump_outputs_sorted_sampled_and_repeatable(tmp_path, monkeypatch):
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_NEW_SIGNAL", 100)
    monkeypatch.setattr(bench, "DUMP_PAIRS", 50)
    rng = np.random.default_rng(5)
    e = rng.permutation(np.arange(1 << 31, (1 << 31) + 1000, dtype=np.uint64)).astype(np.uint32)  # above 2^31: no sign
    p = rng.integers(-2, 4, e.size).astype(np.int8)
    ne, npr = e[:300].copy(), p[:300].copy()
    pr = (rng.permutation(200).astype(np.int64) << 32) | 0xFFFFFFF0
    pairs = torch.from_numpy(np.concatenate([pr, np.full(20, -1, np.int64)]))  # room past the entries written
    cnew = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8)
    st = {"new_pairs": 200}
    for d in ("a", "b"):
        # the order in memory differs from run to run; what is written must not
        o = rng.permutation(e.size) if d == "b" else np.arange(e.size)
        bench.dump_outputs(str(tmp_path / d), "", _Set(e[o], p[o]), _Set(ne, npr), pairs, cnew, st)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["call_new", "counts", "max_signal_elems", "max_signal_prios", "new_pairs",
                           "new_signal_elems", "new_signal_prios"]
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64)
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))), k
    srt = np.argsort(e)
    assert np.array_equal(got["max_signal_elems"], e[srt].astype(np.float64))  # whole: under its cap, exact in f64
    assert np.array_equal(got["max_signal_prios"], p[srt].astype(np.float32))
    assert got["new_signal_elems"].size == 100 and (np.diff(got["new_signal_elems"]) > 0).all()
    by_elem = dict(zip(ne.tolist(), npr.tolist()))
    assert [by_elem[int(x)] for x in got["new_signal_elems"]] == got["new_signal_prios"].tolist()
    assert got["new_pairs"].size == 50 and (np.diff(got["new_pairs"]) > 0).all()
    assert set(got["new_pairs"].tolist()) <= set(pr.astype(np.float64).tolist())
    assert got["call_new"].tolist() == [0, 1, 1, 0, 1]
    assert got["counts"].tolist() == [1000, 300, 200, 3]


def test_dump_outputs_stay_under_64_mb():
    import bench

    calls = 4096 * 64
    worst = 4 * calls + 8 * bench.DUMP_PAIRS + 12 * (bench.DUMP_MAX_SIGNAL + bench.DUMP_NEW_SIGNAL) + 8 * 4
    assert worst + 7 * 128 <= 64 * 10 ** 6  # (128 B of .npy header per file)
    idx = bench.dump_sample(10_000_000, bench.DUMP_MAX_SIGNAL)
    assert idx.size == bench.DUMP_MAX_SIGNAL and (np.diff(idx) > 0).all() and idx[-1] < 10_000_000
    assert np.array_equal(idx, bench.dump_sample(10_000_000, bench.DUMP_MAX_SIGNAL))
    assert np.array_equal(bench.dump_sample(7, 10), np.arange(7))


def test_walk_configs():
    import bench
    from syzkaller_amd import synth

    g, r = bench.walk_cfg("global"), bench.walk_cfg("region", skew=1)
    assert g.global_walk == 1 and r.global_walk == 0 and r.skew == 1
    assert bench.KNOWN_SYS == {"global": 1, "region": 2048}
    # SURVEY 8(d)'s walk: PCs at 0xffffffff81000000 + 5 b over all 2^20 blocks,
    # each step b <- (4 b + 1 + r % 4) mod 2^20 (csrc/common.h synth_trace)
    pcs, cs, prio = synth.traces(g, 0, 2, 4, np.full(8, 512, np.uint32))
    b = (pcs - np.uint64(0xFFFFFFFF81000000)) // np.uint64(5)
    assert ((pcs - np.uint64(0xFFFFFFFF81000000)) % np.uint64(5) == 0).all() and (b < (1 << 20)).all()
    for c in range(8):
        x = b[int(cs[c]): int(cs[c]) + 512].astype(np.int64)
        d = (x[1:] - 4 * x[:-1] - 1) % (1 << 20)
        assert (d < 4).all()
    assert len(np.unique(b)) > 3000  # not confined to 256-block regions
