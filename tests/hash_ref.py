"""The reference of tests/test_gpu_hash.py and tests/test_hash_ref_cpu.py:
pkg/hash through hashlib.sha1 -- an implementation independent of this
project's -- and the loops over map[hash.Sig] restated line by line over
Python dicts and sets, with Go's map iteration replaced by ascending order.

A Sig is `bytes` of length 20; ascending order is bytes' own (memcmp's)."""
import hashlib

import numpy as np

SIG_BYTES = 20

# FIPS 180 example messages and their digests (checked against hashlib in test_hash_ref_cpu.py)
FIPS_VECTORS = (
    (b"", "da39a3ee5e6b4b0d3255bfef95601890afd80709"),
    (b"abc", "a9993e364706816aba3e25717850c26c9cd0d89d"),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "84983e441c3bd26ebaae4aa1f95129e5e54670f1"),
    (b"a" * 1000000, "34aa973cd4c4daa4f61eeb2bdbad27316534016f"),
)


def hash_sig(*pieces):
    """hash.Hash, pkg/hash/hash.go:18-26: the sha1 of the pieces in order."""
    h = hashlib.sha1()
    for p in pieces:
        h.update(bytes(p))
    return h.digest()


def hash_string(*pieces):
    """hash.String, hash.go:28-31."""
    return hash_sig(*pieces).hex()


def hash_messages(data, off):
    """Sig of data[off[i]:off[i + 1]] for every i -> uint8[n, 20]."""
    data = bytes(data)
    off = [int(x) for x in off]
    out = np.empty((len(off) - 1, SIG_BYTES), np.uint8)
    for i in range(len(off) - 1):
        out[i] = np.frombuffer(hashlib.sha1(data[off[i]:off[i + 1]]).digest(), np.uint8)
    return out


def pack(msgs, lead=0):
    """The messages back to back behind `lead` filler bytes -> (data uint8[], off int64[n + 1])."""
    off = np.zeros(len(msgs) + 1, np.int64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    off += lead
    buf = b"\xA5" * lead + b"".join(bytes(m) for m in msgs)
    return np.frombuffer(buf, np.uint8).copy() if buf else np.empty(0, np.uint8), off


def as_sigs(arr):
    """uint8[n, 20] (or flat) -> list of bytes."""
    a = np.asarray(arr, np.uint8).reshape(-1, SIG_BYTES)
    return [a[i].tobytes() for i in range(a.shape[0])]


def as_array(sigs):
    sigs = list(sigs)
    if not sigs:
        return np.empty((0, SIG_BYTES), np.uint8)
    return np.frombuffer(b"".join(sigs), np.uint8).reshape(-1, SIG_BYTES).copy()


def add_inputs(corpus_hashes, sigs):
    """syz-fuzzer/fuzzer.go:447-452 for every input of a batch in arrival order:
        sig := hash.Hash(data)
        if _, ok := fuzzer.corpusHashes[sig]; !ok {
            fuzzer.corpus = append(fuzzer.corpus, p)
            fuzzer.corpusHashes[sig] = struct{}{}
        }
    corpus_hashes (a set) is updated in place; returns is_new uint8[n]: the
    rows whose program was appended."""
    is_new = np.zeros(len(sigs), np.uint8)
    for i, sig in enumerate(sigs):
        if sig not in corpus_hashes:
            is_new[i] = 1
            corpus_hashes.add(sig)
    return is_new


def hub_connect(corpus_sigs):
    """syz-manager/manager.go:1110-1113, the first sync:
        mgr.hubCorpus = make(map[hash.Sig]bool)
        for _, inp := range mgr.corpus {
            mgr.hubCorpus[hash.Hash(inp.Prog)] = true
            a.Corpus = append(a.Corpus, inp.Prog)
        }
    Returns (hubCorpus, sent uint8[n]): every program is sent."""
    hub = set()
    for sig in corpus_sigs:
        hub.add(sig)
    return hub, np.ones(len(corpus_sigs), np.uint8)


def hub_sync(hub_corpus, corpus_sigs):
    """manager.go:1142-1158:
        corpus := make(map[hash.Sig]bool)
        for _, inp := range mgr.corpus {
            sig := hash.Hash(inp.Prog)
            corpus[sig] = true
            if mgr.hubCorpus[sig] { continue }
            mgr.hubCorpus[sig] = true
            a.Add = append(a.Add, inp.Prog)
        }
        for sig := range mgr.hubCorpus {
            if corpus[sig] { continue }
            delete(mgr.hubCorpus, sig)
            a.Del = append(a.Del, sig.String())
        }
    hub_corpus (a set) is updated in place; returns (add uint8[n], dels): the
    rows appended to a.Add, and a.Del's Sigs with the range over hubCorpus in
    ascending order."""
    corpus = set()
    add = np.zeros(len(corpus_sigs), np.uint8)
    for i, sig in enumerate(corpus_sigs):
        corpus.add(sig)
        if sig in hub_corpus:
            continue
        hub_corpus.add(sig)
        add[i] = 1
    dels = []
    for sig in sorted(hub_corpus):
        if sig in corpus:
            continue
        dels.append(sig)
    for sig in dels:
        hub_corpus.discard(sig)
    return add, dels


def number_sigs(sigs, known=()):
    """numberSigs: the dense keys syzsig_manager_new_input_batch takes for
    hash.String(a.Prog).  A Sig's key is the number of distinct Sigs that first
    appear before it.  Returns (key uint32[n], first list, is_known list, nkeys):
    first[k] = key k's first row, is_known[k] = its Sig is in `known`."""
    known = set(known)
    index = {}
    key = np.zeros(len(sigs), np.uint32)
    first, is_known = [], []
    for i, sig in enumerate(sigs):
        if sig not in index:
            index[sig] = len(index)
            first.append(i)
            is_known.append(1 if sig in known else 0)
        key[i] = index[sig]
    return key, first, is_known, len(index)
