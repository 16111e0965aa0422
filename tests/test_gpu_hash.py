"""GPU: pkg/hash over a batch (syzsig_hash_dev) and the Sig sets
(syzsig_sigset_*, syzsig_number_sigs_dev, syzsig_hub_sync_dev) against
tests/hash_ref.py: hashlib.sha1 and the restated loops of fuzzer.go:447-452 and
manager.go:1110-1113, :1142-1158.  Every device result is compared byte for
byte; outputs are pre-filled so that an unwritten byte shows; the paths taken
are asserted from syzsig_hash_stats."""
import ctypes

import numpy as np
import pytest
import torch

from syzkaller_amd import _lib, hashing
from tests import hash_ref as R

pytestmark = pytest.mark.gpu

STAGE, LONG, TILE = _lib.SYZSIG_HASH_STAGE, _lib.SYZSIG_HASH_LONG, _lib.SYZSIG_SIGSET_TILE
FILL = 0xCD
PAD_EDGES = (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 129)


def blocks(lens):
    return sum((int(n) + 72) // 64 for n in lens)


def dev_hash(gpu, data, off, base_shift=0):
    """hash_batch into a pre-filled output, from a data tensor that ends exactly
    at nbytes and starts base_shift bytes into its allocation; -> (uint8[n, 20], stats)."""
    data = np.ascontiguousarray(data, np.uint8)
    big = torch.full((base_shift + data.size,), 0x5A, dtype=torch.uint8, device=gpu.dev)
    d = big[base_shift:]
    if data.size:
        d.copy_(torch.from_numpy(data))
    n = len(off) - 1
    out = torch.full((n + 1, 20), FILL, dtype=torch.uint8, device=gpu.dev)
    got = hashing.hash_batch(gpu, d, torch.as_tensor(np.asarray(off, np.int64)), out=out)
    assert got.data_ptr() == out.data_ptr()
    o = out.cpu().numpy()
    assert (o[n] == FILL).all(), "wrote past the last Sig"
    return o[:n], hashing.hash_stats(gpu)


def check_hash(gpu, msgs, lead=0, base_shift=0):
    data, off = R.pack(msgs, lead)
    got, stats = dev_hash(gpu, data, off, base_shift)
    exp = R.hash_messages(data, off)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"messages {bad[:8].tolist()} of lengths {[len(msgs[i]) for i in bad[:8]]} differ"
    assert sum(stats[:3]) == len(msgs) and stats[3] == blocks(len(m) for m in msgs)
    return stats


def rand_msgs(rng, lens):
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]


# ---- hashing ----

def test_padding_edges_at_every_start_offset(gpu):
    """Each padding-edge length at each start alignment 0..15, in one buffer:
    a filler message in front of each moves its start to the wanted residue."""
    rng = np.random.default_rng(1)
    msgs, pos, want = [], 0, []
    for s in range(16):
        for n in PAD_EDGES:
            fill = (s - pos) % 16
            msgs += rand_msgs(rng, [fill, n])
            pos += fill + n
            want.append((pos - n) % 16 == s)
    assert all(want)
    st = check_hash(gpu, msgs)
    assert st[0] == len(msgs) and st[1] == 0  # every wave's span is small: all staged
    for shift in (1, 2, 3, 7):  # ... and with the data tensor itself off alignment
        check_hash(gpu, msgs[:130], base_shift=shift)


def test_padding_edges_direct_path(gpu):
    """The same lengths read from global memory: a 40000-byte message in every wave pushes its span past the stage."""
    rng = np.random.default_rng(2)
    msgs = []
    for s in range(16):
        chunk = []
        for n in PAD_EDGES:
            chunk += rand_msgs(rng, [(s + 5 * n) % 16 + (1 if n % 2 else 0), n])
        chunk = chunk[:63]
        msgs += chunk + rand_msgs(rng, [STAGE + 1000 + s]) + rand_msgs(rng, [0] * (63 - len(chunk)))
    st = check_hash(gpu, msgs, lead=0, base_shift=3)
    assert st == (0, 16 * 63, 16, st[3])


def test_known_vectors(gpu):
    msgs = [m for m, _ in R.FIPS_VECTORS]
    data, off = R.pack(msgs, lead=5)
    got, st = dev_hash(gpu, data, off)
    assert [hashing.to_string(s) for s in got] == [h for _, h in R.FIPS_VECTORS]
    assert st[2] == 1 and st[3] == blocks(len(m) for m in msgs)  # the 10^6-byte message took the long list


@pytest.mark.parametrize("nmsg", [0, 1, 63, 64, 65, 257])
def test_batch_shapes(gpu, nmsg):
    rng = np.random.default_rng(nmsg)
    check_hash(gpu, rand_msgs(rng, rng.integers(0, 300, nmsg)), lead=nmsg % 7)


def test_only_empty_messages_and_64_lengths(gpu):
    st = check_hash(gpu, [b""] * 70)
    assert st == (70, 0, 0, 70)
    rng = np.random.default_rng(3)
    st = check_hash(gpu, rand_msgs(rng, rng.permutation(64) * 3 + 1), lead=9)
    assert st[0] == 64


@pytest.mark.parametrize("span,staged", [(STAGE - 1, True), (STAGE, True), (STAGE + 1, False)])
def test_span_against_the_stage(gpu, span, staged):
    """One wave of 64 messages whose bytes together are `span`, the first at byte 15 of a 16-byte chunk."""
    rng = np.random.default_rng(span)
    lens = [span // 64] * 64
    lens[17] += span - sum(lens)
    st = check_hash(gpu, rand_msgs(rng, lens), lead=15)
    assert st[:3] == ((64, 0, 0) if staged else (0, 64, 0))


def test_long_threshold_and_list(gpu):
    rng = np.random.default_rng(4)
    st = check_hash(gpu, rand_msgs(rng, [LONG - 1, LONG, LONG + 1]), lead=1)
    assert st[:3] == (2, 0, 1)
    # one long message among 63 short ones: the span is past the stage, the short ones are read directly
    lens = list(rng.integers(0, 200, 63))
    lens.insert(31, STAGE + 5)
    st = check_hash(gpu, rand_msgs(rng, lens), lead=2)
    assert st[:3] == (0, 63, 1)
    # the list with 0, 1 and 65 entries (0: every test above whose st[2] is 0)
    st = check_hash(gpu, rand_msgs(rng, [LONG + 1 + i for i in range(65)]), lead=3)
    assert st[:3] == (0, 0, 65)


def raw_hash(gpu, data, off, nmsg, nbytes, out, null=None):
    p = lambda t, name: ctypes.c_void_p(0 if null == name else t.data_ptr())  # noqa: E731
    return gpu.L.syzsig_hash_dev(gpu.eng.h, p(data, "data"), p(off, "off"), nmsg, nbytes, p(out, "sig"))


@pytest.mark.parametrize("what", ["decreasing", "past_nbytes", "null_off", "null_sig", "null_data", "too_long"])
def test_hash_errors_write_nothing(gpu, what):
    data = torch.arange(256, dtype=torch.uint8, device=gpu.dev)
    off = [0, 10, 30, 100]
    nbytes, null, code = 256, None, _lib.SYZSIG_EINVAL
    if what == "decreasing":
        off = [0, 30, 10, 100]
    elif what == "past_nbytes":
        off = [0, 10, 30, 257]
    elif what == "too_long":  # the offsets only claim the length: the check precedes any read
        off = [0, 10, 10 + _lib.SYZSIG_HASH_MAX_MSG + 1, 20 + _lib.SYZSIG_HASH_MAX_MSG + 1]
        nbytes, code = off[-1], _lib.SYZSIG_ERANGE
    else:
        null = what[5:]
    offt = torch.tensor(off, dtype=torch.int64, device=gpu.dev)
    out = torch.full((3, 20), FILL, dtype=torch.uint8, device=gpu.dev)
    assert raw_hash(gpu, data, offt, 3, nbytes, out, null) == code
    assert b"hash" in gpu.L.syzsig_last_error()
    assert (out.cpu().numpy() == FILL).all()
    # the longest allowed length passes the check (claimed only where nothing would be read: not run)
    assert raw_hash(gpu, data, torch.tensor([0, 10, 30, 256], dtype=torch.int64, device=gpu.dev), 3, 256, out) == 0
    assert (out.cpu().numpy() != FILL).any()


# ---- Sig sets on chosen 20-byte values ----

def sig(*pairs, base=0x40):
    """a Sig of `base` bytes with sig[i] = v for every (i, v)"""
    b = bytearray([base]) * 20
    for i, v in pairs:
        b[i] = v
    return bytes(b)


SEAMS = [sig((0, 1)), sig((0, 2)), sig((19, 1)), sig((19, 2)), sig((7, 1)), sig((8, 1)), sig((7, 1), (8, 1)),
         sig((15, 1)), sig((16, 1)), sig((15, 1), (16, 1)), sig(), bytes([0] * 19 + [1]), bytes([1] + [0] * 19),
         bytes(20), b"\xff" * 20, b"\xff" * 19 + b"\xfe", b"\xfe" + b"\xff" * 19]


def check_add(gpu, s, ref, batch):
    """SigSet.add against fuzzer.go:447-452; the set's export against the reference set, ascending."""
    before = R.as_sigs(s.export().cpu().numpy())
    exp_new = R.add_inputs(ref, batch)
    got = s.add(R.as_array(batch)).cpu().numpy()
    np.testing.assert_array_equal(got, exp_new)
    after = R.as_sigs(s.export().cpu().numpy())
    assert after == sorted(ref) and s.Len() == len(ref)
    if not exp_new.any():
        assert after == before
    return got


def test_sigset_word_seams_byte_order_and_extremes(gpu):
    s, ref = hashing.SigSet(gpu), set()
    assert s.is_nil() and s.Len() == 0
    check_add(gpu, s, ref, SEAMS[::2])  # add on the nil set
    assert not s.is_nil()
    check_add(gpu, s, ref, SEAMS[::-1])  # the other half, each next to a neighbour that is present
    assert R.as_sigs(s.export().cpu().numpy()) == sorted(SEAMS)
    got = s.contains(R.as_array(SEAMS + [sig((3, 9)), sig((19, 3))])).cpu().numpy()
    np.testing.assert_array_equal(got, [1] * len(SEAMS) + [0, 0])
    check_add(gpu, s, ref, SEAMS)  # nothing new: the set and its export stay
    check_add(gpu, s, ref, [])


def test_sigset_duplicates_inside_a_batch(gpu):
    rng = np.random.default_rng(7)
    base = R.as_sigs(rng.integers(0, 256, (50, 20), dtype=np.uint8))
    batch = [base[0]] + base[1:20] + [base[5], base[5]] + base[20:] + [base[0]]  # rows (0, n - 1) and neighbours
    s, ref = hashing.SigSet(gpu), set()
    got = check_add(gpu, s, ref, batch)
    assert got[0] == 1 and got[-1] == 0 and got[20:22].tolist() == [0, 0]


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_sigset_batch_sizes_around_the_sort_tile(gpu, n):
    rng = np.random.default_rng(n)
    pool = rng.integers(0, 256, (n * 3 // 4, 20), dtype=np.uint8)
    pool[: n // 8, :16] = pool[0, :16]  # many that differ in the last word only
    s, ref = hashing.SigSet(gpu), set()
    check_add(gpu, s, ref, R.as_sigs(pool[rng.integers(0, pool.shape[0], 300)]))
    check_add(gpu, s, ref, R.as_sigs(pool[rng.integers(0, pool.shape[0], n)]))


def test_sigset_nil_forms_and_export_cap(gpu):
    s = hashing.SigSet(gpu)
    np.testing.assert_array_equal(s.contains(R.as_array(SEAMS[:3])).cpu().numpy(), [0, 0, 0])  # contains on NULL
    assert s.export().shape == (0, 20)
    assert s.add(R.as_array([])).numel() == 0 and s.is_nil()  # n = 0 allocates nothing
    s.add(R.as_array(SEAMS[:5]))
    out = torch.full((4, 20), FILL, dtype=torch.uint8, device=gpu.dev)
    with pytest.raises(_lib.SyzsigError) as e:
        s.export(out)  # cap one short
    assert e.value.code == _lib.SYZSIG_ERANGE and e.value.needed == 5 and (out.cpu().numpy() == FILL).all()
    flags = torch.full((8,), FILL, dtype=torch.uint8, device=gpu.dev)
    h = ctypes.c_void_p(s.handle.value)
    # (the count is checked before anything is read: the Sigs are only claimed)
    rc = gpu.L.syzsig_sigset_add_dev(gpu.eng.h, ctypes.byref(h), out.data_ptr(), (1 << 25) + 1, flags.data_ptr())
    assert rc == _lib.SYZSIG_ERANGE and h.value == s.handle.value and s.Len() == 5
    assert (flags.cpu().numpy() == FILL).all()
    rc = gpu.L.syzsig_sigset_add_dev(gpu.eng.h, ctypes.byref(h), None, 3, flags.data_ptr())
    assert rc == _lib.SYZSIG_EINVAL and b"sigset_add" in gpu.L.syzsig_last_error() and s.Len() == 5


# ---- number_sigs ----

def check_number(gpu, sigs, known_sigs, known):
    key, first, is_known = hashing.number_sigs(R.as_array(sigs), known, gpu)
    ekey, efirst, eknown, n = R.number_sigs(sigs, known_sigs)
    np.testing.assert_array_equal(key.cpu().numpy().view(np.uint32), ekey)
    assert first.cpu().tolist() == efirst and is_known.cpu().tolist() == eknown and first.numel() == n


def test_number_sigs(gpu):
    rng = np.random.default_rng(11)
    pool = R.as_sigs(rng.integers(0, 256, (40, 20), dtype=np.uint8)) + SEAMS
    batch = [pool[i] for i in rng.integers(0, len(pool), 300)]
    check_number(gpu, batch, (), None)  # a NULL set
    empty = hashing.SigSet(gpu)
    empty.add(R.as_array(pool[:3]))
    empty.hub_sync(R.as_array([]))  # non-NULL and empty
    assert not empty.is_nil() and empty.Len() == 0
    check_number(gpu, batch, (), empty)
    known = hashing.SigSet(gpu)
    known.add(R.as_array(pool[::3] + [sig((4, 4))]))
    check_number(gpu, batch, pool[::3], known)
    check_number(gpu, [SEAMS[3], SEAMS[1], SEAMS[3], SEAMS[3], SEAMS[0], SEAMS[1]], pool[::3], known)
    check_number(gpu, [], (), known)  # n = 0
    big = [pool[i] for i in rng.integers(0, len(pool), 2 * TILE + 5)]
    check_number(gpu, big, pool[::3], known)


# ---- hub_sync ----

def check_hub(gpu, s, ref, corpus):
    if s.is_nil():
        ref2, add = R.hub_connect(corpus)  # manager.go:1110-1113
        firsts = R.add_inputs(set(), corpus)
        ref.clear()
        ref.update(ref2)
        exp_add, exp_del = add * firsts, []  # the Prog of a repeated Sig is the same bytes: sent once
    else:
        exp_add, exp_del = R.hub_sync(ref, corpus)
    add, dels = s.hub_sync(R.as_array(corpus))
    np.testing.assert_array_equal(add.cpu().numpy(), exp_add)
    assert R.as_sigs(dels.cpu().numpy()) == exp_del
    assert R.as_sigs(s.export().cpu().numpy()) == sorted(ref)


def test_hub_sync_hand_cases(gpu):
    S = lambda x: bytes([x]) * 20  # noqa: E731
    s, ref = hashing.SigSet(gpu), set()
    check_hub(gpu, s, ref, [])  # nothing to connect with: stays nil
    assert s.is_nil()
    check_hub(gpu, s, ref, [S(5), S(2), S(8)])  # Connect
    check_hub(gpu, s, ref, [S(7), S(8), S(7), S(1)])  # Add 7 and 1, Del 2 and 5 ascending
    assert ref == {S(1), S(7), S(8)}
    check_hub(gpu, s, ref, [S(1), S(7), S(8)])  # in sync: nothing either way
    check_hub(gpu, s, ref, SEAMS)
    check_hub(gpu, s, ref, [])  # an empty corpus deletes everything
    assert s.Len() == 0 and not s.is_nil()


def test_hub_sync_random_corpus_and_del_cap(gpu):
    rng = np.random.default_rng(13)
    pool = R.as_sigs(rng.integers(0, 256, (4500, 20), dtype=np.uint8))
    s, ref = hashing.SigSet(gpu), set()
    check_hub(gpu, s, ref, pool[1500:])  # the hub's 3000
    corpus = [pool[i] for i in rng.permutation(3000)]  # 3000 Sigs, half of them the hub's
    before = R.as_sigs(s.export().cpu().numpy())
    out = torch.full((1499, 20), FILL, dtype=torch.uint8, device=gpu.dev)
    with pytest.raises(_lib.SyzsigError) as e:
        s.hub_sync(R.as_array(corpus), del_out=out)  # del_cap one short
    assert e.value.code == _lib.SYZSIG_ERANGE and e.value.needed == 1500
    assert (out.cpu().numpy() == FILL).all() and R.as_sigs(s.export().cpu().numpy()) == before
    check_hub(gpu, s, ref, corpus)
    assert s.Len() == 3000


# ---- the chain: wire bytes -> Sigs -> keys -> Manager.NewInput ----

def test_chain_programs_to_new_input(gpu):
    from syzkaller_amd import signal as S
    from tests import corpus_ref as C

    rng = np.random.default_rng(17)
    distinct = [b"r%d = openat(0x%x, &(0x7f0000000000)='./file%d')\n" % (i, int(rng.integers(1 << 30)), i) * int(rng.integers(1, 9))
                for i in range(220)]
    progs = [distinct[i] for i in rng.integers(0, len(distinct), 600)]
    rows = [(p, (rng.integers(0, 500, int(rng.integers(0, 40))).astype(np.uint32),
                 rng.integers(-2, 4, 40).astype(np.int8)), rng.integers(0, 300, int(rng.integers(0, 20))).astype(np.uint32))
            for p in progs]
    rows = [(p, (e, pr[: e.size]), c) for p, (e, pr), c in rows]
    mgr = C.Manager()  # the reference: mgr.corpus keyed by hash.String from hashlib
    cs, cc = S.Signal(None, gpu.eng), S.Cover(gpu.eng)
    corpus_keys, fuzz_hashes = hashing.SigSet(gpu), hashing.SigSet(gpu)
    stored, ref_hashes = {}, set()
    for lo in range(0, 600, 200):  # three polls' worth
        batch = rows[lo:lo + 200]
        exp = [mgr.NewInput(R.hash_string(p), ser, cov) for p, ser, cov in batch]
        k = hashing.new_input_keys(gpu, [p for p, _, _ in batch], corpus_keys)
        sig_hex = [hashing.to_string(x) for x in k["sigs"].cpu().numpy()]
        assert sig_hex == [R.hash_string(p) for p, _, _ in batch]
        present = {int(k["first"][key]): key for key in k["present"].tolist()}
        dev_rows, at = [], []
        for i, (p, ser, cov) in enumerate(batch):
            if i in present:  # the key's stored entry goes in front of its first input
                e, pr, c = stored[sig_hex[i]]
                dev_rows.append((present[i], S.Serial(e, pr), c, True))
            at.append(len(dev_rows))
            dev_rows.append((int(k["input_key"][i]), S.Serial(*ser), cov, False))
        acc, new, entries = S.manager_new_input(cs, cc, dev_rows, k["nkeys"], gpu.eng)
        assert [(bool(acc[j]), bool(new[j])) for j in at] == exp
        for key, (ser, cov) in entries.items():
            stored[sig_hex[int(k["first"][key])]] = (ser.Elems, ser.Prios, cov)
        new_rows = [i for i, j in enumerate(at) if new[j]]
        if new_rows:
            added = corpus_keys.add(k["sigs"][torch.as_tensor(new_rows, device=gpu.dev)])
            assert added.cpu().numpy().all()  # a new key is new to the keys of mgr.corpus
        # addInputToCorpus on the fuzzer that receives the batch
        np.testing.assert_array_equal(fuzz_hashes.add(k["sigs"]).cpu().numpy(),
                                      R.add_inputs(ref_hashes, [bytes.fromhex(h) for h in sig_hex]))
    assert set(stored) == set(mgr.corpus) and corpus_keys.Len() == len(mgr.corpus)
    for h, (e, pr, c) in stored.items():
        assert dict(zip(e.tolist(), pr.tolist())) == mgr.corpus[h][0].to_dict()
        assert set(c.tolist()) == set(mgr.corpus[h][1].Serialize())
    assert cs.to_dict() == mgr.corpusSignal.to_dict()
    assert R.as_sigs(fuzz_hashes.export().cpu().numpy()) == sorted(ref_hashes)
