"""pkg/db's db.Open on device (pkg/db/db.go:39-53, :177-265): from the bytes of
a corpus.db to the live records' values as the (data, off) pair that
hashing.hash_batch and hashing.new_input_keys take.

The frames are walked on the host (syzsig_db_scan), the file is uploaded once,
the values are inflated by libsyzsig's batched RFC 1951 decoder
(syzsig_inflate_dev, csrc/db.hip) and the map's last-write-wins is one sort of
(Sig, index) (syzsig_db_live_dev).

The write side (db.go:55-132, :147-175) runs there too: DB.save / delete /
apply decide which ops reach the log (syzsig_db_apply_dev), compress the written
values (syzsig_deflate_dev) and frame them (syzsig_db_records_dev) into device
buffers; DB.flush / compact / bump_version return the bytes to append to the
file or to replace it with.  File I/O stays with the caller, as open_db takes
bytes rather than a path."""
import ctypes
import struct

import numpy as np
import torch

from . import _lib, hashing
from ._lib import check

__all__ = ["open_db", "scan", "inflate", "inflate_stats", "db_live", "deflate", "deflate_stats", "deflate_host",
           "db_records", "db_apply", "serialize_header", "DB", "ENDED"]

SEQ_DELETED = (1 << 64) - 1
ENDED = {_lib.SYZSIG_DB_END_EOF: "eof", _lib.SYZSIG_DB_END_BAD_HEADER: "bad_header",
         _lib.SYZSIG_DB_END_BAD_MAGIC: "bad_magic", _lib.SYZSIG_DB_END_TRUNCATED: "truncated"}


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if (t is not None and t.numel()) else 0)


def scan(data):
    """syzsig_db_scan of the file's bytes (host only).  Returns (version, ended,
    key_off u64[n], key_len u32[n], seq u64[n], val_off u64[n], val_len u32[n])."""
    data = bytes(data)
    L = _lib.lib()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    ver, n, ended = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
    rc = L.syzsig_db_scan(buf, len(data), 0, ctypes.byref(ver), ctypes.byref(n), ctypes.byref(ended), None, None, None,
                          None, None)
    if rc != _lib.SYZSIG_ERANGE:
        check(rc)
    cap = n.value
    ko, sq, vo = (np.zeros(cap, np.uint64) for _ in range(3))
    kl, vl = (np.zeros(cap, np.uint32) for _ in range(2))
    check(L.syzsig_db_scan(buf, len(data), cap, ctypes.byref(ver), ctypes.byref(n), ctypes.byref(ended), ko.ctypes.data,
                           kl.ctypes.data, sq.ctypes.data, vo.ctypes.data, vl.ctypes.data))
    return int(ver.value), int(ended.value), ko, kl, sq, vo, vl


def inflate(dev, src, src_off, src_len, out=None, sizing=False):
    """syzsig_inflate_dev: stream i is src[src_off[i] : src_off[i] + src_len[i]]
    (src uint8 on the device; src_off int64 / src_len int32 tensors on the
    device).  Returns (data uint8[total], off int64[n + 1], status uint8[n]) on
    the device; sizing=True stops after the lengths and statuses (data is None).
    A given `out` that is too small raises SyzsigError(SYZSIG_ERANGE) with the
    needed bytes in .needed."""
    n = src_len.numel()
    off = torch.empty(n + 1, dtype=torch.int64, device=dev.dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev.dev)
    total = ctypes.c_uint64()

    def call(o):
        try:
            check(dev.L.syzsig_inflate_dev(dev.eng.h, _p(src), src.numel(), _p(src_off), _p(src_len), n, _p(o),
                                           o.numel() if o is not None else 0, _p(off), _p(status), ctypes.byref(total)))
        except _lib.SyzsigError as e:
            e.needed = int(total.value)
            raise

    if out is None:
        call(None)  # the sizing call
        if sizing:
            return None, off, status
        out = torch.empty(int(total.value), dtype=torch.uint8, device=dev.dev)
    call(out)
    return out[: total.value], off, status


def inflate_stats(dev):
    """(streams of the first launch, streams on the long list, stored, fixed,
    dynamic blocks) of the last inflate call's counting pass."""
    out = (ctypes.c_uint64 * 4)()
    check(dev.L.syzsig_inflate_stats(dev.eng.h, out))
    return int(out[0]), int(out[1]), int(out[2]), int(out[3]) & 0xFFFFFFFF, int(out[3]) >> 32


def db_live(dev, sigs, seqs, nvalid):
    """syzsig_db_live_dev -> (live uint8[n] on the device, nlive, uncompacted)."""
    n = sigs.shape[0]
    live = torch.empty(n, dtype=torch.uint8, device=dev.dev)
    nlive, unc = ctypes.c_uint64(), ctypes.c_uint64()
    check(dev.L.syzsig_db_live_dev(dev.eng.h, _p(sigs), _p(seqs), n, nvalid, _p(live), ctypes.byref(nlive),
                                   ctypes.byref(unc)))
    return live, int(nlive.value), int(unc.value)


def deflate(dev, src, src_off, src_len, out=None, sizing=False):
    """syzsig_deflate_dev: value i is src[src_off[i] : src_off[i] + src_len[i]]
    (src uint8 on the device; src_off int64 / src_len int32 tensors on the
    device).  Returns (data uint8[total], off int64[n + 1]) on the device: stream
    i is data[off[i]:off[i + 1]]; sizing=True stops after the lengths (data is
    None).  A given `out` that is too small raises SyzsigError(SYZSIG_ERANGE)
    with the needed bytes in .needed."""
    n = src_len.numel()
    off = torch.empty(n + 1, dtype=torch.int64, device=dev.dev)
    total = ctypes.c_uint64()

    def call(o):
        try:
            check(dev.L.syzsig_deflate_dev(dev.eng.h, _p(src), src.numel(), _p(src_off), _p(src_len), n, _p(o),
                                           o.numel() if o is not None else 0, _p(off), ctypes.byref(total)))
        except _lib.SyzsigError as e:
            e.needed = int(total.value)
            raise

    if out is None:
        call(None)  # the sizing call
        if sizing:
            return None, off
        out = torch.empty(int(total.value), dtype=torch.uint8, device=dev.dev)
    call(out)
    return out[: total.value], off


def deflate_stats(dev):
    """(values of the first launch, values on the long list, streams written
    stored, streams written fixed) of the last deflate call's counting pass."""
    out = (ctypes.c_uint64 * 4)()
    check(dev.L.syzsig_deflate_stats(dev.eng.h, out))
    return tuple(int(x) for x in out)


def deflate_host(val):
    """syzsig_deflate_host: the device's compressor on the host (no device, no
    context) -> the stream's bytes, equal to the device's for the same value."""
    val = bytes(val)
    L = _lib.lib()
    src = ctypes.create_string_buffer(val, max(len(val), 1))
    n = ctypes.c_uint64()
    check(L.syzsig_deflate_host(src, len(val), None, 0, ctypes.byref(n)))
    out = ctypes.create_string_buffer(max(n.value, 1))
    check(L.syzsig_deflate_host(src, len(val), out, n.value, ctypes.byref(n)))
    return out.raw[: n.value]


def db_records(dev, sigs, seqs, streams, out=None):
    """syzsig_db_records_dev: serializeRecord's bytes of the records (sigs
    uint8[n, 20], seqs int64[n] holding the uint64 bits, streams = (data, off)
    from deflate), all on the device -> (data uint8[total], off int64[n + 1])."""
    n = seqs.numel()
    sdata, soff = streams
    off = torch.empty(n + 1, dtype=torch.int64, device=dev.dev)
    total = ctypes.c_uint64()

    def call(o):
        try:
            check(dev.L.syzsig_db_records_dev(dev.eng.h, _p(sigs), _p(seqs), n, _p(sdata), sdata.numel(), _p(soff), _p(o),
                                              o.numel() if o is not None else 0, _p(off), ctypes.byref(total)))
        except _lib.SyzsigError as e:
            e.needed = int(total.value)
            raise

    if out is None:
        call(None)
        out = torch.empty(int(total.value), dtype=torch.uint8, device=dev.dev)
    call(out)
    return out[: total.value], off


def db_apply(dev, live_sigs, live_seqs, live_vals, op_sigs, op_seqs, op_vals):
    """syzsig_db_apply_dev: Save / Delete (an op seq of ^0) of the m ops in order
    against the nl live records; Sigs uint8[., 20], seqs int64 (the uint64 bits),
    values (data, off), all on the device -> (written uint8[m], keep_live
    uint8[nl], keep_op uint8[m] on the device, (nwritten, nkeep_live, nkeep_op))."""
    nl, m = live_seqs.numel(), op_seqs.numel()
    written, keep_op = (torch.empty(m, dtype=torch.uint8, device=dev.dev) for _ in range(2))
    keep_live = torch.empty(nl, dtype=torch.uint8, device=dev.dev)
    c = [ctypes.c_uint64() for _ in range(3)]
    check(dev.L.syzsig_db_apply_dev(dev.eng.h, _p(live_sigs), _p(live_seqs), nl, _p(live_vals[0]), live_vals[0].numel(),
                                    _p(live_vals[1]), _p(op_sigs), _p(op_seqs), m, _p(op_vals[0]), op_vals[0].numel(),
                                    _p(op_vals[1]), _p(written), _p(keep_live), _p(keep_op), *(ctypes.byref(x) for x in c)))
    return written, keep_live, keep_op, tuple(int(x.value) for x in c)


def serialize_header(version):
    """serializeHeader (db.go:141-145)."""
    return struct.pack("<IIQ", 0xBADDB, 2, version)


def _frame_host(key, seq, stream):
    """serializeRecord's bytes around a ready stream, for a key of any form"""
    out = struct.pack("<II", 0xFEE1BAD, len(key)) + key + struct.pack("<Q", seq)
    return out if seq == SEQ_DELETED else out + struct.pack("<I", len(stream)) + stream


def _gather(dev, parts):
    """The values picked from several (data, off) pairs, in order, as one pair:
    parts = [((data, off), rows int64 on the device), ...]."""
    lens, idx = [], []
    for (data, off), rows in parts:
        ln = off[rows + 1] - off[rows]
        excl = torch.cumsum(ln, 0) - ln
        # byte k of the part: its value's first byte in data, plus its place inside the value
        idx.append(data[torch.repeat_interleave(off[rows] - excl, ln) + torch.arange(int(ln.sum()), device=dev.dev)])
        lens.append(ln)
    off = torch.zeros(sum(x.numel() for x in lens) + 1, dtype=torch.int64, device=dev.dev)
    if off.numel() > 1:
        torch.cumsum(torch.cat(lens), 0, out=off[1:])
    data = torch.cat(idx) if idx else torch.empty(0, dtype=torch.uint8, device=dev.dev)
    return data, off


def _hex_to_sigs(data, key_off, key_len):
    """The keys as Sigs uint8[n, 20], or None when one is not 40 lower-case hex
    characters (hash.String's form; the bytes-to-Sig map is then exact and
    injective)."""
    n = key_len.size
    if n == 0:
        return np.zeros((0, 20), np.uint8)
    if (key_len != 40).any():
        return None
    raw = np.frombuffer(data, np.uint8)
    c = raw[key_off.astype(np.int64)[:, None] + np.arange(40)].astype(np.int16)
    digit, lower = (c >= 48) & (c <= 57), (c >= 97) & (c <= 102)
    if not (digit | lower).all():
        return None
    v = np.where(digit, c - 48, c - 87).astype(np.uint8)
    return np.ascontiguousarray(v[:, 0::2] << 4 | v[:, 1::2])


class DB:
    """What db.Open leaves: Version, Records and uncompacted (db.go:25-32).
    keys: the live records' keys in file order of their last write -- Sigs
    uint8[n, 20] on the device, or a list of bytes when the file has a key that
    is not hash.String's; seqs uint64[n] (host); vals = (data, off) on the
    device: value i is data[off[i]:off[i + 1]]; ended: how the replay ended
    ("eof", "bad_header", "bad_magic", "truncated", "inflate", "trailing").
    pending: what Save / Delete wrote since the last flush (db.pending)."""

    def __init__(self, dev, version, keys, seqs, vals, uncompacted, ended):
        self.dev, self.version, self.keys, self.seqs, self.vals = dev, version, keys, seqs, vals
        self.uncompacted, self.ended = uncompacted, ended
        self.pending = []  # db.pending: the framed records not yet handed out by flush, device buffers (or bytes)

    def Len(self):
        return int(self.seqs.size)

    __len__ = Len

    def needs_compact(self):
        """db.go:49"""
        return self.Len() == 0 or self.uncompacted // 10 * 9 > self.Len()

    def hashes(self):
        """hash.Hash of every live value, uint8[n, 20] on the device."""
        return hashing.hash_batch(self.dev, *self.vals)

    def records(self):
        """{key bytes (as in the file): (val, seq)}, downloaded (tests, tools)."""
        data, off = self.vals[0].cpu().numpy().tobytes(), self.vals[1].cpu().numpy()
        keys = self.keys if isinstance(self.keys, list) else [bytes(k).hex().encode() for k in self.keys.cpu().numpy()]
        return {k: (data[int(off[i]):int(off[i + 1])], int(self.seqs[i])) for i, k in enumerate(keys)}

    # ---- the write side (db.go:55-132) over batches ----

    def _i64(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(self.dev.dev)

    def _streams(self, vals, rows=None):
        """the DEFLATE streams of the values `rows` of vals (all of them: None), as (data, off)"""
        off = vals[1]
        lo, hi = (off[:-1], off[1:]) if rows is None else (off[rows], off[rows + 1])
        return deflate(self.dev, vals[0], lo, (hi - lo).to(torch.int32))

    def apply(self, keys, vals, seqs):
        """Save (db.go:55-65) and Delete (:67-74) of a batch of ops in order: keys
        as Sigs uint8[m, 20] on the device (a list of bytes for a DB whose keys
        are a list), vals = (data, off) on the device, seqs uint64[m] where ^0
        makes the op a Delete (its value must be empty).  The ops that are no
        no-ops are compressed and framed into `pending`, keys / seqs / vals
        become the new live set and `uncompacted` grows by their number, which is
        returned."""
        seqs = np.ascontiguousarray(seqs, np.uint64)
        if seqs.size == 0:
            return 0
        if isinstance(self.keys, list):
            return self._apply_on_host(list(keys), vals, seqs)
        dev = self.dev
        d_seq = self._i64(seqs)
        written, keep_live, keep_op, (nw, _, _) = db_apply(dev, self.keys, self._i64(self.seqs), self.vals, keys, d_seq, vals)
        if nw:
            w = torch.nonzero(written).flatten()
            self.pending.append(db_records(dev, keys[w], d_seq[w], self._streams(vals, w))[0])
        kl, ko = torch.nonzero(keep_live).flatten(), torch.nonzero(keep_op).flatten()
        self.vals = _gather(dev, [(self.vals, kl), (vals, ko)])
        self.keys = torch.cat([self.keys[kl], keys[ko]])
        self.seqs = np.concatenate([self.seqs[kl.cpu().numpy()], seqs[ko.cpu().numpy()]])
        self.uncompacted += nw
        return nw

    def _apply_on_host(self, keys, vals, seqs):
        """A DB with a key that is not hash.String's: the no-op rules and the
        frames by the reference's loop, the values still compressed on the device."""
        data, off = vals[0].cpu().numpy().tobytes(), vals[1].cpu().numpy()
        cur, log = self.records(), []
        for j, key in enumerate(keys):
            val, seq = data[int(off[j]):int(off[j + 1])], int(seqs[j])
            if seq == SEQ_DELETED:
                if val:
                    raise ValueError("deleting record with value")
                if key not in cur:
                    continue
                del cur[key]
            else:
                if cur.get(key) == (val, seq):
                    continue
                cur.pop(key, None)  # (re-inserted at the end: the order of the last writes)
                cur[key] = (val, seq)
            log.append(j)
        if log:
            sdata, soff = self._streams(vals, torch.tensor(log, dtype=torch.int64, device=self.dev.dev))
            sdata, soff = sdata.cpu().numpy().tobytes(), soff.cpu().numpy()
            self.pending.append(b"".join(_frame_host(keys[j], int(seqs[j]), sdata[int(soff[i]):int(soff[i + 1])])
                                         for i, j in enumerate(log)))
        voff = np.zeros(len(cur) + 1, np.int64)
        np.cumsum([len(v) for v, _ in cur.values()], out=voff[1:])
        self.keys, self.seqs = list(cur), np.array([s for _, s in cur.values()], np.uint64)
        self.vals = (hashing._bytes_tensor(self.dev, b"".join(v for v, _ in cur.values())),
                     torch.from_numpy(voff).to(self.dev.dev))
        self.uncompacted += len(log)
        return len(log)

    def save(self, keys, vals, seqs):
        """db.Save of every (key, value, seq) in order; the reserved seq ^0 raises (:56-58)."""
        seqs = np.ascontiguousarray(seqs, np.uint64)
        if (seqs == np.uint64(SEQ_DELETED)).any():
            raise ValueError("reserved seq")
        return self.apply(keys, vals, seqs)

    def delete(self, keys):
        """db.Delete of every key in order."""
        m = len(keys)
        none = (torch.empty(0, dtype=torch.uint8, device=self.dev.dev),
                torch.zeros(m + 1, dtype=torch.int64, device=self.dev.dev))
        return self.apply(keys, none, np.full(m, SEQ_DELETED, np.uint64))

    def compact(self):
        """db.compact (:104-125) -> the whole file's bytes: the header and every
        live record, in the order of keys.  uncompacted = Len(), pending dropped.
        Writing the file (the reference's .tmp and rename) is the caller's."""
        out = serialize_header(self.version)
        if self.Len():
            streams = self._streams(self.vals)
            if isinstance(self.keys, list):
                sdata, soff = streams[0].cpu().numpy().tobytes(), streams[1].cpu().numpy()
                out += b"".join(_frame_host(k, int(self.seqs[i]), sdata[int(soff[i]):int(soff[i + 1])])
                                for i, k in enumerate(self.keys))
            else:
                out += db_records(self.dev, self.keys, self._i64(self.seqs), streams)[0].cpu().numpy().tobytes()
        self.uncompacted, self.pending = self.Len(), []
        return out

    def flush(self):
        """db.Flush (:76-94): ("replace", the compacted file) when uncompacted / 10 * 9 >
        len(Records); else ("append", the pending records' bytes); None with nothing pending."""
        if self.uncompacted // 10 * 9 > self.Len():
            return "replace", self.compact()
        if not self.pending:
            return None
        out = b"".join(p if isinstance(p, bytes) else p.cpu().numpy().tobytes() for p in self.pending)
        self.pending = []
        return "append", out

    def bump_version(self, version):
        """db.BumpVersion (:96-102): a flush for the same version, else the compacted file under the new one."""
        if self.version == version:
            return self.flush()
        self.version = version
        return "replace", self.compact()


def open_db(dev, data):
    """db.Open's deserializeDB over the file's bytes; see DB."""
    data = bytes(data)
    version, ended, ko, kl, sq, vo, vl = scan(data)
    n = sq.size
    i64 = lambda a: torch.from_numpy(a.view(np.int64)).to(dev.dev)  # noqa: E731
    src = hashing._bytes_tensor(dev, data)
    d_vo, d_vl = i64(vo), torch.from_numpy(vl.view(np.int32)).to(dev.dev)
    _, _, status = inflate(dev, src, d_vo, d_vl, sizing=True)
    bad = torch.nonzero(status).flatten()
    nvalid = int(bad[0]) if bad.numel() else n
    if nvalid < n:
        ended = "trailing" if int(status[nvalid]) == _lib.SYZSIG_INFLATE_TRAILING else "inflate"
    else:
        ended = ENDED[ended]
    sigs = _hex_to_sigs(data, ko[:nvalid], kl[:nvalid])
    if sigs is None:
        return _open_on_host(dev, data, version, ended, nvalid, ko, kl, sq, src, d_vo, d_vl)
    d_sigs = torch.from_numpy(sigs).to(dev.dev)
    live, nlive, unc = db_live(dev, d_sigs, i64(sq[:nvalid]), nvalid)
    # the live values alone are decoded, straight into the compact pair: no gather of bytes
    rows = torch.nonzero(live).flatten()
    vals = inflate(dev, src, d_vo[rows], d_vl[rows])[:2]
    assert rows.numel() == nlive
    return DB(dev, version, d_sigs[rows], sq[rows.cpu().numpy()], vals, unc, ended)


def _open_on_host(dev, data, version, ended, nvalid, ko, kl, sq, src, d_vo, d_vl):
    """A key that is not hash.String's: the values are inflated on the device
    all the same, the map is replayed by the reference's loop (db.go:185-200)."""
    out, off, _ = inflate(dev, src, d_vo[:nvalid], d_vl[:nvalid])
    out, off = out.cpu().numpy().tobytes(), off.cpu().numpy()
    last = {}
    for i in range(nvalid):
        key = data[int(ko[i]):int(ko[i]) + int(kl[i])]
        last.pop(key, None)  # (re-inserted at the end: the order of the last writes)
        if int(sq[i]) != SEQ_DELETED:
            last[key] = i
    rows = np.fromiter(last.values(), np.int64, len(last))
    vals = [out[int(off[i]):int(off[i + 1])] for i in rows]
    voff = np.zeros(len(vals) + 1, np.int64)
    np.cumsum([len(v) for v in vals], out=voff[1:])
    return DB(dev, version, list(last), sq[rows], (hashing._bytes_tensor(dev, b"".join(vals)),
                                                    torch.from_numpy(voff).to(dev.dev)), nvalid, ended)
