"""Loaders of the cover and comps fixtures the reference executor wrote
(tests/golden/cover, tests/golden/comps; generators make_golden_cover.py and
make_golden_comps.py beside them), and the framing of a comps-mode region."""
import functools
import os

import numpy as np

from tests.conftest import GOLDEN, load_golden

COVER_SETS = ["lengths", "abort", "big"]
COVER_NAMES = [f"{s}_dedup{d}" for s in COVER_SETS for d in (0, 1)]
COMPS_NAMES = ["edges", "segments", "long", "toomany"]
TRACE_KEYS = ("pcs", "call_start", "call_len", "call_failed", "prog_call")
K_FAIL_STATUS = 67  # executor/common.h:81


def _load(sub, name):
    with np.load(os.path.join(GOLDEN, sub, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def load_cover(name):
    fx = _load("cover", name)
    if name.startswith("big_"):  # the trace of executor_big.npz
        big = load_golden("executor_big")
        fx.update({k: big[k] for k in TRACE_KEYS})
    return fx


@functools.lru_cache(maxsize=None)
def load_comps(name):
    return _load("comps", name)


def comps_region_calls(fx, p):
    """Program p's region of a comps fixture, framed from the fixture's own
    per-call arrays: [(call, words_start, words_end)] for its completed calls,
    offsets into fx["regions"].  Asserts the headers (executor.h:567-574:
    callIndex, callNum, errno, faultInjected, nsig = 0, ncover = 0, comps_size)
    and that the walk ends where the region does."""
    reg = fx["regions"]
    a, b = int(fx["region_off"][p]), int(fx["region_off"][p + 1])
    c0 = int(fx["prog_call"][p])
    done = int(fx["exp_completed"][p])
    assert int(reg[a]) == done
    pos, calls = a + 1, []
    for i in range(done):
        c = c0 + i
        err = 22 if fx["call_failed"][c] else 0  # EINVAL, as the harness sets reserrno
        assert reg[pos:pos + 7].tolist() == [i, i, err, 0, 0, 0, int(fx["exp_comps_cnt"][c])], (p, i)
        pos += 7
        calls.append((c, pos, pos + int(fx["exp_out_words"][c])))
        pos = calls[-1][2]
    assert pos == b
    return calls
