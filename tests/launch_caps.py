"""The launch caps of the text, database and hash entry points as data, and the
expectations of batches large enough to pass them.

Every kernel behind syzsig_prog_calls_dev, the pkg/db entry points,
syzsig_hash_dev and the Sig sets runs on a capped grid: past the cap a
workgroup, a wave or a lane goes on to a second element.  The constants below
are those caps, SOURCES the text they were read from (tests/test_launch_caps_cpu.py
holds the two together), and the helpers build a batch of cap + a few elements
from a small pool of distinct ones:

  place         which pool element stands at which index, so that the element a
                workgroup serves second never has the outcome of its first
  ragged_take   the pool's byte strings (or id lists) laid out over the batch
  *_expect      the reference (tests/progtext_ref.py, tests/db_ref.py, hashlib)
                run once per distinct element, taken by kind index
  sig_runs ...  for the keyed operations, whose elements are not independent:
                fuzzer.go:447-452, numberSigs, db.go:185-200 and db.go:55-74
                restated over the whole batch by one sort of (Sig, row)

No device and no library here."""
import hashlib

import numpy as np

from tests import db_ref as R
from tests import progtext_ref as P

# internal.h: grid_for(n, 256) with max_blocks = 2048, an element per thread.  k_pc_prep, k_pc_seglens (calls.hip);
# k_inf_prep, k_def_prep, k_rec_len (db.hip); k_hash_prep, every k_sg_* / k_ap_* row kernel, k_sg_pack / k_ap_pack (sigs.hip)
CAP_GRID_FOR = 2048 * 256
# calls.hip: pgrid = min((nprog + 3) / 4, 1 << 16) workgroups of four waves, a wave per program: k_pc_reduce, k_pc_write
CAP_PC_WAVES = (1 << 16) * 4
# calls.hip: k_pc_long on min((list_cap + 63) / 64, 1024) workgroups of 64, a lane per listed head
CAP_PC_LONG = 1024 * 64
# calls.hip: k_su_gather (segsort.h) on grid_cap(nprog, 1 << 16), a workgroup per program, CallSet mode
CAP_SU_GATHER = 1 << 16
# db.hip: k_rec_write on grid_cap(n, 1 << 16) workgroups of one wave, a wave per record
CAP_REC_WRITE = 1 << 16

# (file under syzkaller_amd/csrc, text): compared with runs of white space taken as one blank
SOURCES = [
    ("internal.h", "inline int grid_for(uint64_t n, int block, int max_blocks = 2048)"),
    ("internal.h", "if (g > (uint64_t)max_blocks) g = max_blocks;"),
    ("segsort.h", "inline int grid_cap(uint64_t n, uint64_t cap = 1u << 20) "
                  "{ return (int)std::min<uint64_t>(std::max<uint64_t>(n, 1), cap); }"),
    ("segsort.h", "constexpr uint32_t kSuThreads = 256;"),
    ("segsort.h", "for (uint64_t i = blockIdx.x; i < nseg; i += gridDim.x) { const uint64_t a = off[i], n = (off[i + 1] - a) * W;"),
    ("calls.hip", "k_pc_prep<<<grid_for(nprog, 256), 256, 0, s>>>"),
    ("calls.hip", "k_pc_seglens<<<grid_for(nprog, 256), 256, 0, s>>>"),
    ("calls.hip", "const unsigned pgrid = (unsigned)std::min<uint64_t>((nprog + 3) / 4, 1u << 16);"),
    ("calls.hip", "k_pc_reduce<<<pgrid, 256, 0, s>>>"),
    ("calls.hip", "k_pc_write<<<pgrid, 256, 0, s>>>(nprog, first_line, rec, seg_len, coff,"),
    ("calls.hip", "k_pc_write<<<pgrid, 256, 0, s>>>(nprog, first_line, rec, seg_len, roff,"),
    ("calls.hip", "const uint64_t W = (uint64_t)gridDim.x * 4;"),
    ("calls.hip", "k_pc_long<<<(unsigned)std::min<uint64_t>((list_cap + 63) / 64, 1024), 64, 0, s>>>"),
    ("calls.hip", "k_su_gather<uint32_t><<<grid_cap(nprog, 1u << 16), kSuThreads, 0, s>>>"),
    ("db.hip", "k_inf_prep<<<grid_for(n, 256), 256, 0, s>>>"),
    ("db.hip", "k_def_prep<<<grid_for(n, 256), 256, 0, s>>>"),
    ("db.hip", "k_rec_len<<<grid_for(n, 256), 256, 0, s>>>"),
    ("db.hip", "k_rec_write<<<grid_cap(n, 1u << 16), 64, 0, s>>>"),
    ("db.hip", "for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) { const uint64_t sq = seq[i]"),
    ("sigs.hip", "k_hash_prep<<<grid_for(nmsg, 256), 256, 0, s>>>"),
    ("sigs.hip", "k_sg_pack<<<grid_for(std::max(n, nt), 256), 256, 0, s>>>"),
    ("sigs.hip", "k_ap_pack<<<grid_for(std::max(n, nt), 256), 256, 0, s>>>"),
]
# every launch of these kernels is grid_for(<rows>, 256) on 256 threads, whatever its rows are called
GRID_FOR_KERNELS = {
    "sigs.hip": ["k_sg_mark", "k_sg_compact", "k_sg_merge", "k_sg_contains", "k_sg_export", "k_sg_heads", "k_sg_number",
                 "k_sg_absent", "k_sg_last", "k_ap_check", "k_ap_written", "k_ap_keep"],
}

DEL = R.SEQ_DELETED


# ---- placement ----

def crosses(kind, cap):
    """the element a capped grid serves at index i never has the class of the one it served a sweep earlier"""
    kind = np.asarray(kind)
    return kind.size > cap and bool((kind[cap:] != kind[:-cap]).all())


def place(n, nclass, caps, rare):
    """kind[i] < nclass for the n elements of a batch: the classes in turn, moved on by one with every sweep of the
    smallest cap; then a rare class at cap - 1, cap, cap + 1 of every cap and at n - 1.  kind[i] != kind[i - cap] for
    every cap and every i >= cap (asserted)."""
    caps = sorted(caps)
    i = np.arange(n, dtype=np.int64)
    kind = (i + i // caps[0]) % nclass
    spots = [c + d for c in caps for d in (-1, 0, 1)] + [n - 1]
    for t, at in enumerate(spots):
        near = {int(kind[at + s * c]) for c in caps for s in (-1, 1) if 0 <= at + s * c < n}
        kind[at] = next(r for r in (rare[(t + k) % len(rare)] for k in range(len(rare))) if r not in near)
    for c in caps:
        assert n > c and crosses(kind, c), c
    assert set(kind.tolist()) == set(range(nclass))
    return kind


def ragged_take(items, kind, dtype=np.uint8):
    """items[kind[0]] + items[kind[1]] + ... as one array, and the offsets int64[n + 1] of the parts"""
    parts = [np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype) for x in items]
    lens = np.array([p.size for p in parts], np.int64)
    flat = np.concatenate(parts).astype(dtype) if lens.sum() else np.zeros(0, dtype)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    kind = np.asarray(kind, np.int64)
    off = np.zeros(kind.size + 1, np.int64)
    np.cumsum(lens[kind], out=off[1:])
    # element k of the output: its part's first element in flat, plus its place inside the part
    idx = np.repeat(start[kind] - off[:-1], lens[kind])
    idx += np.arange(int(off[-1]), dtype=np.int64)
    return flat[idx], off


# ---- program text ----

def listed(ln, window):
    """Is the head of this line (tests/progtext_ref.lines' form) left to the long list in either mode?  calls.hip:
    a head that does not end within the `window` bytes from its line's start.  Decided here for the two forms the
    pools use: a line shorter than the window by two, its end and a '\\r' before it in sight, is not; one whose first
    `window` bytes are identifier characters and then blanks alone is."""
    if P.skipped(ln):
        return False
    if len(ln) + 2 <= window:
        return False
    w = ln[:window]
    body = w.rstrip(b" ")
    if len(w) == window and body and all(c in P.IDENT for c in body):
        return True
    raise ValueError("a line of neither form")


def prog_calls_expect(pool, kind, names, mode, enabled=None, window=256):
    """The batch pool[kind[0]], pool[kind[1]], ... and what syzsig_prog_calls_dev returns for it, the reference run
    once per pool element: a dict of blob uint8[], off, call_off, ids, status, err_line, flag and stats (the four of
    syzsig_prog_calls_stats: lines, skipped, heads decided in the window, heads listed)."""
    one = [P.batch([p], names, mode, enabled) for p in pool]
    kind = np.asarray(kind, np.int64)
    ids, call_off = ragged_take([o[1] for o in one], kind, np.int32)
    blob, off = ragged_take(pool, kind)
    per = np.zeros((len(pool), 4), np.int64)
    for k, p in enumerate(pool):
        lns = [ln for ln, _ in P.lines(p)]
        nskip, nlist = sum(P.skipped(ln) for ln in lns), sum(listed(ln, window) for ln in lns)
        per[k] = (len(lns), nskip, len(lns) - nskip - nlist, nlist)
    count = np.bincount(kind, minlength=len(pool))
    return {"blob": blob, "off": off, "call_off": call_off, "ids": ids,
            "status": np.array([o[2][0] for o in one], np.uint8)[kind],
            "err_line": np.array([o[3][0] for o in one], np.int32)[kind],
            "flag": np.array([o[4][0] for o in one], np.uint8)[kind],
            "stats": tuple(int(x) for x in count @ per)}


# ---- DEFLATE streams and record frames ----

def stream_form(s):
    """'stored' or 'fixed': BTYPE of the stream's first block (RFC 1951 3.2.3)"""
    return {0: "stored", 1: "fixed", 2: "dynamic"}[(s[0] >> 1) & 3]


def checked_streams(vals, stream):
    """stream(v) of every value, each held to zlib: it inflates back to v"""
    out = [stream(v) if v else b"" for v in vals]
    for v, s in zip(vals, out):
        assert not v or R.inflate_class(s) == (R.OK, v)
    return out


def deflate_expect(vals, kind, stream, long_bytes=4096):
    """The values vals[kind[i]] as (src uint8[], src_off, src_len) and their streams as (out, out_off), stream() run
    once per distinct value and checked by zlib; stats = syzsig_deflate_stats' (short, long, stored, fixed)."""
    kind = np.asarray(kind, np.int64)
    streams = checked_streams(vals, stream)
    src, off = ragged_take(vals, kind)
    out, out_off = ragged_take(streams, kind)
    count = np.bincount(kind, minlength=len(vals))
    pick = lambda f: int(sum(c for c, v, s in zip(count, vals, streams) if v and f(v, s)))  # noqa: E731
    stats = (pick(lambda v, s: len(v) <= long_bytes), pick(lambda v, s: len(v) > long_bytes),
             pick(lambda v, s: stream_form(s) == "stored"), pick(lambda v, s: stream_form(s) == "fixed"))
    return {"src": src, "src_off": off[:-1].copy(), "src_len": np.diff(off).astype(np.int32), "out": out,
            "out_off": out_off, "stats": stats}


def hex_of(sigs):
    """hash.String of Sigs uint8[n, 20]: uint8[n, 40], lower-case hex"""
    digits = np.frombuffer(b"0123456789abcdef", np.uint8)
    out = np.empty((sigs.shape[0], 40), np.uint8)
    out[:, 0::2] = digits[sigs >> 4]
    out[:, 1::2] = digits[sigs & 15]
    return out


def records_expect(vals, kind, sigs, seqs, stream):
    """serializeRecord's bytes of the records (sigs[i], vals[kind[i]], seqs[i]), kind[i] == len(vals) being a delete:
    db_ref.serialize_record once per kind under a stand-in key and seq, laid out over the batch, then every record's
    own key and seq written into their fields (bytes 8-47 and 48-55 of a frame).  -> (data uint8[], off)."""
    kind = np.asarray(kind, np.int64)
    key0 = b"0" * 40
    frames = [R.serialize_record(key0, v, 0, stream) for v in vals] + [R.serialize_record(key0, None, DEL)]
    data, off = ragged_take(frames, kind)
    seqs = np.asarray(seqs, np.uint64)
    assert ((kind == len(vals)) == (seqs == np.uint64(DEL))).all()
    at = off[:-1, None]
    data[at + np.arange(8, 48)] = hex_of(np.asarray(sigs, np.uint8))
    data[at + np.arange(48, 56)] = seqs.astype("<u8").view(np.uint8).reshape(-1, 8)
    return data, off


def stream_pair(vals, kind, stream):
    """the streams of the records' values as db_records takes them: (data, off); a delete (kind len(vals)) has none"""
    return ragged_take(checked_streams(vals, stream) + [b""], kind)


# ---- hashes ----

def hash_expect(base, kind, counter):
    """Messages base[kind[i]], those with counter[i] set carrying i as their first four bytes (little-endian);
    -> (data uint8[], off, digests uint8[n, 20]): hashlib.sha1 once per base message and once per counted one."""
    kind, counter = np.asarray(kind, np.int64), np.asarray(counter, bool)
    data, off = ragged_take(base, kind)
    assert (np.diff(off)[counter] >= 4).all()
    rows = np.flatnonzero(counter)
    data[off[rows, None] + np.arange(4)] = rows.astype("<u4").view(np.uint8).reshape(-1, 4)
    dig = np.frombuffer(b"".join(hashlib.sha1(m).digest() for m in base), np.uint8).reshape(-1, 20)[kind].copy()
    raw = data.tobytes()
    if rows.size:
        dig[rows] = np.frombuffer(b"".join(hashlib.sha1(raw[a:b]).digest() for a, b in zip(off[rows].tolist(),
                                                                                          off[rows + 1].tolist())),
                                  np.uint8).reshape(-1, 20)
    return data, off, dig


# ---- the keyed operations over a whole batch ----

def sig_runs(sigs):
    """The rows sorted by (Sig, row), the Sig as memcmp orders it: three big-endian words of 8, 8 and 4 bytes.
    -> (order int64[n], run int64[n]: the number of the run of equal Sigs each sorted row lies in)."""
    sigs = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 20)
    w0, w1 = (sigs[:, a:a + 8].copy().view(">u8")[:, 0] for a in (0, 8))
    w2 = sigs[:, 16:20].copy().view(">u4")[:, 0]
    order = np.lexsort((w2, w1, w0))  # (stable: equal Sigs stay in row order)
    if order.size == 0:
        return order, order
    s = sigs[order]
    head = np.concatenate([[True], (s[1:] != s[:-1]).any(axis=1)])
    return order, np.cumsum(head) - 1


def first_rows(sigs):
    """bool[n]: the row is the first one of its Sig"""
    order, run = sig_runs(sigs)
    out = np.zeros(order.size, bool)
    if order.size:
        out[order[np.concatenate([[True], run[1:] != run[:-1]])]] = True
    return out


def member(sigs, set_sigs):
    """bool[n]: the row's Sig is among set_sigs"""
    sigs, set_sigs = np.asarray(sigs, np.uint8).reshape(-1, 20), np.asarray(set_sigs, np.uint8).reshape(-1, 20)
    m = set_sigs.shape[0]
    order, run = sig_runs(np.concatenate([set_sigs, sigs]))
    has = np.zeros(int(run[-1]) + 1 if run.size else 0, bool)
    has[run[order < m]] = True
    out = np.zeros(m + sigs.shape[0], bool)
    out[order] = has[run]
    return out[m:]


def sigset_add(set_sigs, sigs):
    """fuzzer.go:447-452 over a batch: is_new bool[n], and the set's size afterwards"""
    new = first_rows(sigs) & ~member(sigs, set_sigs)
    return new, np.asarray(set_sigs).reshape(-1, 20).shape[0] + int(new.sum())


def number_sigs(sigs, known):
    """numberSigs: (key int64[n] in order of first appearance, first int64[nkeys], is_known bool[nkeys])"""
    order, run = sig_runs(sigs)
    n = order.size
    head = np.concatenate([[True], run[1:] != run[:-1]]) if n else np.zeros(0, bool)
    first_of_run = order[head]                      # (the head of a run is its smallest row)
    rank = np.argsort(np.argsort(first_of_run))     # the run's key: its first row's rank among the first rows
    key = np.zeros(n, np.int64)
    key[order] = rank[run]
    first = np.sort(first_of_run)
    return key, first, member(np.asarray(sigs, np.uint8).reshape(-1, 20)[first], known)


def db_live(sigs, seqs, nvalid):
    """db.go:185-200 over the first nvalid records: live bool[n] = the last record of its key and no delete"""
    seqs = np.asarray(seqs, np.uint64)
    order, run = sig_runs(np.asarray(sigs, np.uint8).reshape(-1, 20)[:nvalid])
    live = np.zeros(seqs.size, bool)
    if order.size:
        tail = np.concatenate([run[1:] != run[:-1], [True]])
        live[order[tail]] = seqs[order[tail]] != np.uint64(DEL)
    return live


def db_apply(live_sigs, live_seqs, live_vid, op_sigs, op_seqs, op_vid):
    """db.go:55-74 over a batch: Save / Delete (seq ^0) of the ops in order against the live records.  *_vid: a
    number per value, equal numbers for equal bytes and no others.  What an op meets is what the row before it in its
    key's run left.  -> (written bool[m], keep_live bool[nl], keep_op bool[m]): the ops that reach the log, and the
    rows that are their key's record afterwards (the last written row of the run, unless it is a delete)."""
    nl = len(live_seqs)
    sigs = np.concatenate([np.asarray(live_sigs, np.uint8).reshape(-1, 20), np.asarray(op_sigs, np.uint8).reshape(-1, 20)])
    seq = np.concatenate([np.asarray(live_seqs, np.uint64), np.asarray(op_seqs, np.uint64)])
    vid = np.concatenate([np.asarray(live_vid, np.int64), np.asarray(op_vid, np.int64)])
    n = seq.size
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, bool), np.zeros(0, bool)
    order, run = sig_runs(sigs)
    sq, vd, dele = seq[order], vid[order], seq[order] == np.uint64(DEL)
    present = np.concatenate([[False], (run[1:] == run[:-1]) & ~dele[:-1]])
    same = np.concatenate([[False], (sq[1:] == sq[:-1]) & (vd[1:] == vd[:-1])])
    wr = np.where(order < nl, True, np.where(dele, present, ~(present & same)))
    last = np.full(int(run[-1]) + 1, -1, np.int64)
    j = np.flatnonzero(wr)
    last[run[j]] = j                                # (ascending: the last written row of each run stays)
    keep_sorted = (last[run] == np.arange(n)) & ~dele
    written, keep = np.zeros(n, bool), np.zeros(n, bool)
    written[order], keep[order] = wr, keep_sorted
    return written[nl:], keep[:nl], keep[nl:]


def value_ids(*lists):
    """a number per value over several lists of byte strings: equal bytes, equal number"""
    ids = {}
    return [np.array([ids.setdefault(bytes(v or b""), len(ids)) for v in vals], np.int64) for vals in lists]


def sigs_of_keys(keys):
    """hash.String keys (40 hex characters each) -> uint8[n, 20]"""
    return np.frombuffer(b"".join(bytes.fromhex(k.decode()) for k in keys), np.uint8).reshape(-1, 20).copy()

