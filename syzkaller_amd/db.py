"""pkg/db's db.Open on device (pkg/db/db.go:39-53, :177-265): from the bytes of
a corpus.db to the live records' values as the (data, off) pair that
hashing.hash_batch and hashing.new_input_keys take.

The frames are walked on the host (syzsig_db_scan), the file is uploaded once,
the values are inflated by libsyzsig's batched RFC 1951 decoder
(syzsig_inflate_dev, csrc/db.hip) and the map's last-write-wins is one sort of
(Sig, index) (syzsig_db_live_dev).  The write side (Save, Delete, Flush, compact)
stays with the caller."""
import ctypes

import numpy as np
import torch

from . import _lib, hashing
from ._lib import check

__all__ = ["open_db", "scan", "inflate", "inflate_stats", "db_live", "DB", "ENDED"]

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
    ("eof", "bad_header", "bad_magic", "truncated", "inflate", "trailing")."""

    def __init__(self, dev, version, keys, seqs, vals, uncompacted, ended):
        self.dev, self.version, self.keys, self.seqs, self.vals = dev, version, keys, seqs, vals
        self.uncompacted, self.ended = uncompacted, ended

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
