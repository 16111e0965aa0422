"""Corpus identity on device: pkg/hash (pkg/hash/hash.go) over a batch of
programs and the sets keyed by hash.Sig -- fuzzer.corpusHashes (syz-fuzzer/
fuzzer.go:447-452), mgr.hubCorpus (syz-manager/manager.go:1110-1113,
:1142-1158) and the keys of mgr.corpus.

A batch of Sigs is a uint8[n, 20] tensor on the device: row i is hash.Hash of
message i, the bytes Sig.String prints as hex.  Everything is computed by
libsyzsig's kernels (csrc/sigs.hip); torch owns the buffers.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check

__all__ = ["SIG_BYTES", "hash_batch", "hash_stats", "to_string", "from_string", "SigSet", "number_sigs",
           "new_input_keys"]

SIG_BYTES = _lib.SYZSIG_SIG_BYTES


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if (t is not None and t.numel()) else 0)


def _bytes_tensor(dev, data):
    if torch.is_tensor(data):
        if data.dtype != torch.uint8:
            raise ValueError("data is uint8")
        return data.to(dev.dev).contiguous()
    a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    return torch.from_numpy(a.copy()).to(dev.dev) if a.size else torch.empty(0, dtype=torch.uint8, device=dev.dev)


def _sigs_tensor(dev, sigs):
    """uint8[n, 20] on the device from a tensor, an array or a list of 20-byte strings."""
    if torch.is_tensor(sigs):
        t = sigs
    else:
        if not isinstance(sigs, np.ndarray):
            sigs = list(sigs)
            sigs = np.frombuffer(b"".join(bytes(s) for s in sigs), np.uint8) if sigs else np.empty(0, np.uint8)
        t = torch.from_numpy(np.ascontiguousarray(sigs, np.uint8).copy())
    if t.dtype != torch.uint8 or t.numel() % SIG_BYTES:
        raise ValueError("Sigs are uint8[n, 20]")
    return _rows(t.to(dev.dev).contiguous())


def _rows(t):
    """a flat or [n, 20] uint8 tensor as [n, 20] (n = 0 included, which view(-1, 20) refuses)"""
    return t.view(t.numel() // SIG_BYTES, SIG_BYTES)


def hash_batch(dev, data, off, out=None):
    """hash.Hash of data[off[i]:off[i + 1]] for every i (syzsig_hash_dev):
    data uint8[nbytes] (a tensor on the device, or bytes to upload), off
    int64[n + 1].  Returns the Sigs as uint8[n, 20] on the device."""
    data = _bytes_tensor(dev, data)
    off = torch.as_tensor(off, dtype=torch.int64).to(dev.dev).contiguous()
    n = max(off.numel() - 1, 0)
    if out is None:
        out = torch.empty((n, SIG_BYTES), dtype=torch.uint8, device=dev.dev)
    if out.device != dev.dev or out.dtype != torch.uint8 or out.numel() < n * SIG_BYTES or not out.is_contiguous():
        raise ValueError("out is a contiguous uint8[n, 20] on the device")
    check(dev.L.syzsig_hash_dev(dev.eng.h, _p(data), _p(off), n, data.numel(), _p(out)))
    return out


def hash_stats(dev):
    """(messages hashed from LDS staging, read directly from global memory, on
    the long list, 64-byte blocks compressed) of the last hash_batch
    (syzsig_hash_stats)."""
    out = (ctypes.c_uint64 * 4)()
    check(dev.L.syzsig_hash_stats(dev.eng.h, out))
    return tuple(int(x) for x in out)


def to_string(sig):
    """Sig.String, hash.go:33-35: lower-case hex."""
    if torch.is_tensor(sig):
        sig = sig.cpu().numpy()
    b = bytes(sig) if isinstance(sig, (bytes, bytearray)) else np.asarray(sig, np.uint8).tobytes()
    if len(b) != SIG_BYTES:
        raise ValueError("a Sig has 20 bytes")
    return b.hex()


def from_string(s):
    """hash.FromString, hash.go:46-58: the Sig of a hex string; a string that
    is not hex, or not of 20 bytes ("bad len", :51-53), raises ValueError."""
    try:
        b = bytes.fromhex(s)
    except (ValueError, TypeError) as e:
        raise ValueError(f"failed to decode sig '{s}': {e}") from None
    if any(c.isspace() for c in s):  # (hex.DecodeString takes no blanks; bytes.fromhex skips them)
        raise ValueError(f"failed to decode sig '{s}': invalid byte")
    if len(b) != SIG_BYTES:
        raise ValueError(f"failed to decode sig '{s}': bad len")
    return b


class SigSet:
    """A device-resident map[hash.Sig]struct{} (syzsig_sigset): the Sigs sorted
    ascending.  A fresh SigSet is the nil map until something is added."""

    def __init__(self, dev):
        self.dev = dev
        self._h = ctypes.c_void_p()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                self.dev.L.syzsig_sigset_free(h)
            except Exception:
                pass

    @property
    def handle(self):
        return self._h

    def is_nil(self):
        return not self._h.value

    def Len(self):
        return int(self.dev.L.syzsig_sigset_len(self._h))

    __len__ = Len

    def add(self, sigs):
        """fuzzer.go:447-452 over a batch in arrival order
        (syzsig_sigset_add_dev): returns is_new uint8[n] on the device, 1 where
        the Sig was neither in the set nor at an earlier row; the set then
        holds the union."""
        sigs = _sigs_tensor(self.dev, sigs)
        n = sigs.shape[0]
        is_new = torch.empty(n, dtype=torch.uint8, device=self.dev.dev)
        check(self.dev.L.syzsig_sigset_add_dev(self.dev.eng.h, ctypes.byref(self._h), _p(sigs), n, _p(is_new)))
        return is_new

    def contains(self, sigs):
        """uint8[n] on the device: 1 where the Sig is in the set."""
        sigs = _sigs_tensor(self.dev, sigs)
        n = sigs.shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=self.dev.dev)
        check(self.dev.L.syzsig_sigset_contains_dev(self.dev.eng.h, self._h, _p(sigs), n, _p(out)))
        return out

    def export(self, out=None):
        """The set's Sigs ascending, uint8[Len, 20] on the device
        (syzsig_sigset_export_dev).  A given `out` that is too small raises
        SyzsigError(SYZSIG_ERANGE) with the needed Sigs in .needed."""
        if out is None:
            out = torch.empty((self.Len(), SIG_BYTES), dtype=torch.uint8, device=self.dev.dev)
        n = ctypes.c_uint64()
        try:
            check(self.dev.L.syzsig_sigset_export_dev(self.dev.eng.h, self._h, _p(out), out.numel() // SIG_BYTES,
                                                      ctypes.byref(n)))
        except _lib.SyzsigError as e:
            e.needed = int(n.value)
            raise
        return _rows(out)[: n.value]

    def hub_sync(self, corpus_sigs, del_out=None):
        """hubSync's diff with this set as mgr.hubCorpus (manager.go:1142-1158;
        on the nil set the Connect branch, :1110-1113).  corpus_sigs: the Sigs
        of mgr.corpus.  Returns (add uint8[n], dels uint8[ndel, 20]) on the
        device: the rows of a.Add and the Sigs of a.Del, ascending; the set is
        then the set of corpus_sigs.  A given del_out that is too small raises
        SyzsigError(SYZSIG_ERANGE) with .needed and changes nothing."""
        sigs = _sigs_tensor(self.dev, corpus_sigs)
        n = sigs.shape[0]
        add = torch.empty(n, dtype=torch.uint8, device=self.dev.dev)
        if del_out is None:  # Del is a subset of the set
            del_out = torch.empty((self.Len(), SIG_BYTES), dtype=torch.uint8, device=self.dev.dev)
        nd = ctypes.c_uint64()
        try:
            check(self.dev.L.syzsig_hub_sync_dev(self.dev.eng.h, ctypes.byref(self._h), _p(sigs), n, _p(add),
                                                 _p(del_out), del_out.numel() // SIG_BYTES, ctypes.byref(nd)))
        except _lib.SyzsigError as e:
            e.needed = int(nd.value)
            raise
        return add, _rows(del_out)[: nd.value]


def number_sigs(sigs, known=None, dev=None):
    """numberSigs (syzsig_number_sigs_dev): the dense keys of a batch's Sigs in
    order of first appearance.  known: a SigSet (the keys of mgr.corpus) or
    None, and then `dev` says where.  Returns (key int32[n], first
    int32[nkeys], is_known uint8[nkeys]) on the device: first[k] = key k's
    first row, is_known[k] = its Sig is in `known`."""
    dev = dev or (known.dev if known is not None else None)
    if dev is None:
        raise ValueError("number_sigs needs a SigSet or a Device")
    sigs = _sigs_tensor(dev, sigs)
    n = sigs.shape[0]
    key = torch.empty(n, dtype=torch.int32, device=dev.dev)
    first = torch.empty(n, dtype=torch.int32, device=dev.dev)
    is_known = torch.empty(n, dtype=torch.uint8, device=dev.dev)
    nk = ctypes.c_uint64()
    check(dev.L.syzsig_number_sigs_dev(dev.eng.h, known.handle if known is not None else None, _p(sigs), n, _p(key),
                                       _p(first), _p(is_known), ctypes.byref(nk)))
    return key, first[: nk.value], is_known[: nk.value]


def new_input_keys(dev, progs, corpus_sigset=None):
    """From the wire bytes of a batch of RPCInputs to what
    signal.manager_new_input takes: hash.Hash of every a.Prog, then numberSigs
    against the keys of mgr.corpus.  progs: a list of byte strings in arrival
    order.  Returns a dict:
      sigs       uint8[n, 20] on the device;
      input_key  uint32[n] (host): rows[i][0];
      nkeys      the distinct programs;
      first      int[nkeys] (host): key k's first row;
      present    the keys already in mgr.corpus, ascending: the caller passes
                 each one's stored entry as a present=True row before row
                 first[k] (hash.String of it is to_string(sigs[first[k]]))."""
    progs = [bytes(p) for p in progs]
    off = np.zeros(len(progs) + 1, np.int64)
    np.cumsum([len(p) for p in progs], out=off[1:])
    sigs = hash_batch(dev, b"".join(progs), off)
    key, first, is_known = number_sigs(sigs, corpus_sigset, dev)
    return {"sigs": sigs, "input_key": key.cpu().numpy().view(np.uint32), "nkeys": int(first.numel()),
            "first": first.cpu().numpy().astype(np.int64), "present": np.flatnonzero(is_known.cpu().numpy())}
