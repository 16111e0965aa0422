"""GPU: syzsig_inflate_dev and db.open_db over the hand-written DEFLATE streams of
tests/inflate_cases.py -- streams shaped as no compressor shapes them, one rule
of the decoder each.  Every expected class and byte is zlib's
(tests.db_ref.inflate_class), every expected block count comes from the token
lists, the paths taken are asserted from syzsig_inflate_stats; the class
TOO_LONG, which zlib does not have, is "zlib's length is above
SYZSIG_INFLATE_MAX_OUT"."""
import ctypes
import hashlib
import time

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, db
from tests import db_ref as R
from tests import inflate_cases as IC
from tests.test_gpu_db import FILL, check_inflate, check_open, raw_inflate  # noqa: F401

pytestmark = pytest.mark.gpu

LONG = _lib.SYZSIG_INFLATE_LONG
MAX_OUT = _lib.SYZSIG_INFLATE_MAX_OUT
BASE = {c.name: c for c in IC.base_cases()}
FORMS = [(c.name, form) for c in IC.base_cases() for form in ("short", "long") if getattr(c, form) is not None]


def paths(streams):
    """(streams of the first launch, streams on the long list)"""
    return sum(1 for s in streams if 0 < len(s) <= LONG), sum(1 for s in streams if len(s) > LONG)


def block_sum(block_lists):
    return tuple(sum(IC.counts(b)[k] for b in block_lists) for k in range(3))


def test_constants():
    assert (IC.LONG, IC.MAX_OUT) == (LONG, MAX_OUT)


# ---- every base case, alone and with its derived streams ----

@pytest.mark.parametrize("name,form", FORMS)
def test_base_case_and_derived_streams(gpu, name, form):
    case = BASE[name]
    streams = IC.case_streams(case)[form]
    assert (len(streams[0]) > LONG) == (form == "long")
    st = check_inflate(gpu, streams[:1])
    assert st[:2] == paths(streams[:1])
    if case.valid:
        assert st[2:] == IC.counts(IC.form_blocks(case, form))
    else:
        assert R.inflate_class(streams[0])[0] == R.S_INVALID
    st = check_inflate(gpu, streams, lead=len(name) % 7)
    assert st[:2] == paths(streams)


# ---- 64 lanes, 64 different pairs of codes ----

def test_wave64(gpu):
    w = [s for s, _ in IC.wave64(1)]
    for s, spelled in IC.wave64(1):
        assert R.inflate_class(s) == (R.OK, spelled)
    assert check_inflate(gpu, w) == (64, 0, 0, 0, 64)  # one full wave
    assert check_inflate(gpu, w + [w[5]], lead=3) == (65, 0, 0, 0, 65)  # the last stream alone in a second wave
    # the 286 + 30 stream at lane 63, and at lane 0 of the second wave (above: lane 0)
    assert check_inflate(gpu, w[1:] + w[:1], lead=1) == (64, 0, 0, 0, 64)
    assert check_inflate(gpu, w[1:] + [w[7], w[0]] + w[2:9]) == (72, 0, 0, 0, 72)


def test_wave64_bad_and_good_tables_in_adjacent_columns(gpu):
    """every second stream replaced by one of its own header flips"""
    rng = np.random.default_rng(65)
    w = [s if i % 2 == 0 else IC.flip(s, int(rng.integers(24 * 8))) for i, (s, _) in enumerate(IC.wave64(1))]
    classes = [R.inflate_class(s)[0] for s in w]
    assert all(c == R.OK for c in classes[0::2]) and sum(1 for c in classes[1::2] if c != R.OK) >= 16
    st = check_inflate(gpu, w, lead=2)
    assert st[:2] == (64, 0)


# ---- one wave, every block kind at once ----

def test_one_wave_of_all_block_kinds(gpu):
    stored_only = [("stored", IC.NOISE[:300]), ("stored", b""), ("stored", IC.NOISE[300:700])]
    kinds = [BASE["deep_short"].blocks, BASE["bomb"].blocks, BASE["single_dist"].blocks, BASE["len284_31"].blocks, stored_only]
    lanes = list(kinds) + [None]
    while len(lanes) < 64:  # the cheap ones again, so that every lane of the wave is at work (the bomb once)
        lanes.append((kinds[0], kinds[2], kinds[3], kinds[4], None)[len(lanes) % 5])
    streams = [IC.write(b) if b else b"" for b in lanes]
    for s, b in zip(streams, lanes):
        assert not s or R.inflate_class(s) == (R.OK, IC.spelled(b))
    st = check_inflate(gpu, streams)
    assert st[:2] == (sum(1 for b in lanes if b), 0) and st[2:] == block_sum([b for b in lanes if b])


# ---- the output cap, through the sizing call ----

def sizing_call(gpu, streams):
    """syzsig_inflate_dev with d_out = NULL -> (rc, out_bytes, off, status, stats, seconds)"""
    n = len(streams)
    src = torch.from_numpy(np.frombuffer(b"".join(streams), np.uint8).copy()).to(gpu.dev)
    lens = np.array([len(s) for s in streams], np.int64)
    soff = torch.from_numpy(np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)).to(gpu.dev)
    slen = torch.from_numpy(lens.astype(np.int32)).to(gpu.dev)
    off = torch.full((n + 2,), -1, dtype=torch.int64, device=gpu.dev)
    status = torch.full((n + 1,), FILL, dtype=torch.uint8, device=gpu.dev)
    total = ctypes.c_uint64(12345)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = gpu.L.syzsig_inflate_dev(gpu.eng.h, p(src), src.numel(), p(soff), p(slen), n, None, 0, p(off), p(status),
                                  ctypes.byref(total))
    dt = time.perf_counter() - t0
    return rc, total.value, off.cpu().numpy(), status.cpu().numpy(), db.inflate_stats(gpu), dt


def test_output_cap(gpu):
    """Four streams of one-bit codes around 2^28 bytes of output in one counting
    call, then 17 copies of the one that gives exactly 2^28: a total above 2^32.
    (A counting pass of 2^28 bytes on one lane: the two calls print their time.)"""
    S = IC.cap_streams()
    names = ["literal_over", "exact", "match_over", "stored_over"]
    zl = {k: IC.zlib_length(S[k][0]) for k in names}
    assert all(ok for ok, _ in zl.values())
    exp_status = [_lib.SYZSIG_INFLATE_TOO_LONG if zl[k][1] > MAX_OUT else _lib.SYZSIG_INFLATE_OK for k in names]
    exp_len = [0 if zl[k][1] > MAX_OUT else zl[k][1] for k in names]
    assert exp_len == [0, MAX_OUT, 0, 0]
    streams = [S[k][0] for k in names]
    assert all(len(s) > LONG for s in streams)
    rc, total, off, status, st, dt = sizing_call(gpu, streams)
    print("output cap: four streams, one counting call: %.3f s" % dt)
    assert rc == 0, gpu.L.syzsig_last_error()
    assert status[:4].tolist() == exp_status and status[4] == FILL
    assert off[:5].tolist() == [0] + np.cumsum(exp_len).tolist() and off[5] == -1
    assert total == MAX_OUT
    # block headers met before the end or the cap: a stored one and a dynamic one each, and the final block's
    # (a fixed one in literal_over and exact, a stored one in stored_over; match_over ends in its dynamic block)
    assert st == (0, 4, 5, 2, 4)
    rc, total, off, status, st, dt = sizing_call(gpu, [S["exact"][0]] * 17)
    print("output cap: 17 streams of 2^28 bytes, one counting call: %.3f s" % dt)
    assert rc == 0, gpu.L.syzsig_last_error()
    assert status[:17].tolist() == [0] * 17 and status[17] == FILL
    assert off[:18].tolist() == [i * MAX_OUT for i in range(18)] and off[18] == -1
    assert total == 17 * MAX_OUT and total > 1 << 32
    assert st == (0, 17, 17, 17, 17)


# ---- a database file whose values are the base cases ----

def case_records():
    """[(key, value, seq)] and value -> stream: every valid base case, short forms and long forms"""
    recs, stream_of = [], {}
    for c in IC.base_cases():
        if not c.valid:
            continue
        for form in ("short", "long"):
            s = getattr(c, form)
            if s is None or (form == "long" and c.name not in ("deep_all", "fixed_reuse", "rep16_cross")):
                continue
            v = IC.spelled(IC.form_blocks(c, form))
            assert v and v not in stream_of
            stream_of[v] = s
            recs.append((hashlib.sha1(v).hexdigest().encode(), v, len(recs)))
    return recs, stream_of


def test_open_db_over_the_base_cases(gpu):
    recs, stream_of = case_records()
    data = R.serialize_db(5, recs, stream=lambda v: stream_of[v])
    d = check_open(gpu, data)
    assert d.Len() == len(recs) and d.ended == "eof"
    assert d.records() == {k: (v, s) for k, v, s in recs}
    # ... and a second file with no_dist_needed in the middle: the replay ends there
    bad = b"a value that is never seen"
    stream_of[bad] = BASE["no_dist_needed"].short
    mid = len(recs) // 2
    recs2 = recs[:mid] + [(hashlib.sha1(bad).hexdigest().encode(), bad, 99)] + recs[mid:]
    d = check_open(gpu, R.serialize_db(5, recs2, stream=lambda v: stream_of[v]))
    assert (d.ended, d.uncompacted, d.Len()) == ("inflate", mid, mid)
