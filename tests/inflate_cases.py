"""Hand-written DEFLATE streams for syzsig_inflate_dev and csrc/inflate_core.h:
the decoder rules that no compressor's output is known to reach, each as a named
stream built by tests/deflate_writer.py.  Deterministic.  What a stream means is
always zlib's answer (tests.db_ref.inflate_class); the token lists give, besides
the stream, the bytes they spell (the writer's own check) and the block counts."""
import functools
from collections import namedtuple

import numpy as np

from tests import db_ref as R
from tests import deflate_writer as W
from tests.deflate_writer import EOB

LONG = 4096  # SYZSIG_INFLATE_LONG
MAX_OUT = 1 << 28  # SYZSIG_INFLATE_MAX_OUT
NOISE = bytes(np.random.default_rng(1951).integers(0, 256, LONG + 200, dtype=np.uint8))

# blocks: ("stored", data) | ("fixed", tokens) | ("dynamic", tokens, dict(ll_lens=, d_lens=, cl_ops=, cl_lens=, hclen=))
Case = namedtuple("Case", "name blocks short long valid")


def write(blocks):
    w = W.BitWriter()
    for i, b in enumerate(blocks):
        final = i == len(blocks) - 1
        if b[0] == "stored":
            W.stored_block(w, final, b[1])
        elif b[0] == "fixed":
            W.fixed_block(w, final, b[1])
        else:
            W.dynamic_block(w, final, tokens=b[1], **b[2])
    return w.getvalue()


def spelled(blocks):
    """the bytes that the blocks' token lists spell"""
    out = bytearray()
    for b in blocks:
        if b[0] == "stored":
            out += b[1]
        else:
            W.spell(b[1], out)
    return bytes(out)


def counts(blocks):
    """(stored, fixed, dynamic) block headers"""
    return tuple(sum(1 for b in blocks if b[0] == k) for k in ("stored", "fixed", "dynamic"))


def long_blocks(blocks):
    """a non-final stored block of noise in front: the stream passes SYZSIG_INFLATE_LONG bytes"""
    return [("stored", NOISE)] + list(blocks)


def m(length_sym, le, ds, de):
    return (length_sym, le, ds, de)


# ---- the two deep codes ----

def deep_ll():
    lens = [1, 2, 3, 4, 5, 6] + [14] * 232 + [15] * 48
    rng = np.random.default_rng(286)
    lens = [lens[int(i)] for i in rng.permutation(286)]
    assert W.kraft(lens) == 1 << 15
    return lens


def deep_d():
    lens = [1, 2, 3] + [8] * 14 + [7] + list(range(5, 15)) + [15, 15]
    rng = np.random.default_rng(30)
    lens = [lens[int(i)] for i in rng.permutation(30)]
    assert len(lens) == 30 and W.kraft(lens) == 1 << 15
    return lens


DEEP = dict(ll_lens=deep_ll(), d_lens=deep_d())


def every_match(pos):
    """every length symbol with every distance symbol, extra bits all 0 and all 1 (pos: output so far)"""
    assert pos >= 32768
    toks = []
    for ls in range(257, 286):
        for ds in range(30):
            toks.append(m(ls, 0, ds, 0))
            toks.append(m(ls, (1 << W.LEN_EXTRA[ls - 257]) - 1, ds, (1 << W.DIST_EXTRA[ds]) - 1))
    return toks


def random_tokens(rng, nlen, ndist, count, pos=0, p_match=0.4, literals=256):
    """count tokens over the literal/length symbols below nlen and the distance
    symbols below ndist, every distance inside the output so far, then EOB"""
    toks = []
    for _ in range(count):
        ds_ok = [s for s in range(ndist) if W.DIST_BASE[s] <= pos]
        if nlen > 257 and ds_ok and rng.random() < p_match:
            ls, ds = int(rng.integers(257, nlen)), ds_ok[int(rng.integers(len(ds_ok)))]
            le = int(rng.integers(1 << W.LEN_EXTRA[ls - 257]))
            de = int(rng.integers(min(1 << W.DIST_EXTRA[ds], pos - W.DIST_BASE[ds] + 1)))
            toks.append(m(ls, le, ds, de))
            pos += W.LEN_BASE[ls - 257] + le
        else:
            toks.append(int(rng.integers(literals)))
            pos += 1
    return toks + [EOB]


def base_blocks():
    """name -> blocks"""
    rng = np.random.default_rng(2024)
    B = {}
    lits = [int(x) for x in rng.integers(0, 256, 32768)]
    B["deep_all"] = [("dynamic", lits + every_match(32768) + [EOB], DEEP)]
    B["deep_short"] = [("dynamic", random_tokens(rng, 286, 30, 400), DEEP)]
    sd = dict(ll_lens=[0] * 97 + [1] + [0] * 158 + [2, 2], d_lens=[1])
    B["single_dist"] = [("dynamic", [97, m(257, 0, 0, 0), 97, m(257, 0, 0, 0), m(257, 0, 0, 0), EOB], sd)]
    nd = dict(ll_lens=[0] * 97 + [1] + [0] * 158 + [2, 2], d_lens=[0])
    B["no_dist"] = [("dynamic", [97, 97, 97, EOB], nd)]
    B["no_dist_needed"] = [("dynamic", [97, 97, 257, ("raw", 0, 1), EOB], nd)]
    B["rle16"] = [("dynamic", random_tokens(rng, 286, 30, 300),
                   dict(DEEP, cl_ops=W.rle_ops(DEEP["ll_lens"] + DEEP["d_lens"], zeros=False)))]
    # zeros_cross: 'a' and EOB one bit each; the zeros of 257..285 and of distance 0..20 are one 18-run
    ll = [0] * 286
    ll[97] = ll[256] = 1
    zc_d = [0] * 21 + [1, 2, 3, 4, 5, 6, 7, 8, 8]
    assert W.kraft(zc_d) == 1 << 15
    ops = W.rle_ops(ll[:257]) + [(18, 29 + 21 - 11)] + W.plain_ops(zc_d[21:])
    assert W.expand_ops(ops) == ll + zc_d
    B["zeros_cross"] = [("dynamic", [97] * 9 + [EOB], dict(ll_lens=ll, d_lens=zc_d, cl_ops=ops))]
    # rep16_cross: the 16 after 257's length covers 258 (the last literal/length length) and distances 0..3
    ll = [0] * 259
    ll[97], ll[256], ll[257], ll[258] = 1, 2, 3, 3
    ops = W.rle_ops(ll[:257]) + [(3, 0), (16, 5 - 3), (16, 4 - 3)]
    assert W.expand_ops(ops) == ll + [3] * 8
    toks = [97] * 20 + [m(257, 0, s, 0) for s in range(8)] + [m(258, 0, 7, 3), m(258, 0, 4, 1), EOB]
    B["rep16_cross"] = [("dynamic", toks, dict(ll_lens=ll, d_lens=[3] * 8, cl_ops=ops))]
    # rep16_after_18: two 2-bit literals, an 18-run, then a 16: it repeats the zero, not the 2
    ll = [2, 2] + [0] * 254 + [1]
    ops = [(2, 0), (2, 0), (18, 138 - 11), (16, 6 - 3), (18, 110 - 11), (1, 0), (0, 0)]
    assert W.expand_ops(ops) == ll + [0]
    B["rep16_after_18"] = [("dynamic", [0, 1, 1, 0, EOB], dict(ll_lens=ll, d_lens=[0], cl_ops=ops))]
    # ... and after a 17
    ops = [(2, 0), (2, 0), (17, 10 - 3), (16, 6 - 3), (18, 138 - 11), (18, 100 - 11), (1, 0), (0, 0)]
    assert W.expand_ops(ops) == ll + [0]
    B["rep16_after_17"] = [("dynamic", [1, 0, 0, EOB], dict(ll_lens=ll, d_lens=[0], cl_ops=ops))]
    B["len284_31"] = [("fixed", [65, m(284, 31, 0, 0), EOB])]
    # hclen_short: 14 lengths of the code-length code (through symbol 3): 13, 2, 14, 1, 15 stay 0
    ll = [0] * 260
    for s in range(97, 101):
        ll[s] = 3
    for s in range(101, 117):
        ll[s] = 6
    for s in range(256, 260):
        ll[s] = 4
    assert W.kraft(ll) == 1 << 15
    toks = list(range(97, 117)) + [m(257 + i % 3, 0, i % 8, 0) for i in range(16)] + [EOB]
    B["hclen_short"] = [("dynamic", toks, dict(ll_lens=ll, d_lens=[3] * 8, cl_ops=W.rle_ops(ll + [3] * 8), hclen=14))]
    # ... and 5 of them (16, 17, 18, 0, 8): 256 codes of 8 bits, no distance code
    ll = [0] + [8] * 256
    B["hclen_5"] = [("dynamic", [1, 255, 128, 7, EOB], dict(ll_lens=ll, d_lens=[0], cl_ops=W.rle_ops(ll + [0]), hclen=5))]
    # fixed_reuse: a fixed block after a fixed one, after a stored one and after dynamic ones
    text = [int(c) for c in b"r0 = openat$dir(0xffffffffffffff9c, &(0x7f0000000000)='./file0\\x00', 0x0, 0x0)\n"]
    back = lambda n: m(257 + n % 20, 0, 10 + n % 4, n % 8)  # noqa: E731  (a match reaching 33..104 bytes back)
    small = dict(ll_lens=W.random_complete_lengths(np.random.default_rng(5), 280, 12),
                 d_lens=W.random_complete_lengths(np.random.default_rng(6), 20, 9))
    B["fixed_reuse"] = [
        ("fixed", text + [m(260, 0, 5, 1), EOB]),
        ("fixed", [back(1), 120, back(2), EOB]),
        ("stored", bytes(text[:33])),
        ("fixed", [back(3), 121, EOB]),
        ("dynamic", [back(4), 122, 123, back(5), EOB], DEEP),
        ("fixed", [back(6), 124, back(7), EOB]),
        ("dynamic", [back(8), 125, back(9), 7, EOB], small),
        ("fixed", [back(10), 126, EOB]),
    ]
    # alternating: 40 blocks, dynamic / fixed / stored, every block's matches reach into the one before
    blocks, pos = [], 0
    for i in range(40):
        if i % 3 == 2:
            blocks.append(("stored", NOISE[i:i + 20 + i]))
            pos += 20 + i
        else:
            toks = random_tokens(rng, 286, 12, 12, pos=pos, p_match=0.5 if pos else 0)
            blocks.append(("dynamic", toks, DEEP) if i % 3 == 0 else ("fixed", toks))
            pos = len(W.spell(toks, bytearray(pos)))
    B["alternating"] = blocks
    B["bomb"] = bomb_blocks()
    return B


# ---- one-bit codes: a lot of output from little input ----

BOMB_CODE = dict(ll_lens=[0] * 256 + [1] + [0] * 28 + [1], d_lens=[1],
                 cl_ops=[(18, 138 - 11), (18, 118 - 11), (1, 0), (18, 28 - 11), (1, 0), (1, 0)])
assert W.expand_ops(BOMB_CODE["cl_ops"]) == BOMB_CODE["ll_lens"] + BOMB_CODE["d_lens"]
MATCH_258_1 = m(285, 0, 0, 0)


def bomb_blocks(n=4000):
    return [("fixed", [48, EOB]), ("dynamic", [MATCH_258_1] * n + [EOB], BOMB_CODE)]


def cap_stream(lead, nmatch, tail):
    """a stored block of `lead` bytes, nmatch matches of length 258 at distance 1
    under one-bit codes (two bits each), then the final block `tail`; -> stream"""
    w = W.BitWriter()
    W.stored_block(w, False, NOISE[:lead])
    W.dynamic_block(w, False, tokens=[], **BOMB_CODE)
    one = W.BitWriter()
    W.put_tokens(one, W.Code(BOMB_CODE["ll_lens"]), W.Code(BOMB_CODE["d_lens"]), [MATCH_258_1])
    assert one.n == 2 and not one.out
    w.repeat(one.acc, 2, nmatch)
    W.put_tokens(w, W.Code(BOMB_CODE["ll_lens"]), W.Code(BOMB_CODE["d_lens"]), [EOB])
    if tail[0] == "stored":
        W.stored_block(w, True, tail[1])
    else:
        W.fixed_block(w, True, tail[1])
    return w.getvalue()


@functools.lru_cache(maxsize=None)
def cap_streams():
    """name -> (stream, the length that the blocks spell), around SYZSIG_INFLATE_MAX_OUT"""
    full, rest = divmod(MAX_OUT, 258)
    near, rest100 = divmod(MAX_OUT - 100, 258)
    return {
        "exact": (cap_stream(rest, full, ("fixed", [EOB])), MAX_OUT),
        "literal_over": (cap_stream(rest, full, ("fixed", [120, EOB])), MAX_OUT + 1),
        "match_over": (cap_stream(rest100, near + 1, ("fixed", [EOB])), MAX_OUT - 100 + 258),
        "stored_over": (cap_stream(rest100, near, ("stored", NOISE[:200])), MAX_OUT + 100),
    }


def zlib_length(stream):
    """(eof reached with nothing left over, output length) by zlib, without holding the output"""
    import zlib
    d, n, data = zlib.decompressobj(-15), 0, bytes(stream)
    while not d.eof:
        chunk = d.decompress(data, 1 << 24)
        n += len(chunk)
        data = d.unconsumed_tail
        if not chunk and not data:
            break
    return d.eof and not d.unused_data, n


# ---- 64 different codes ----

@functools.lru_cache(maxsize=None)
def wave64(seed):
    """64 streams, each one dynamic block under its own two random complete
    codes; stream 0 has 286 + 30 lengths, stream 1 has 257 + 1.
    -> [(stream, bytes spelled)]"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(64):
        nlen, ndist = int(rng.integers(257, 287)), int(rng.integers(1, 31))
        if i < 2:
            nlen, ndist = ((286, 30), (257, 1))[i]
        code = dict(ll_lens=W.random_complete_lengths(rng, nlen), d_lens=W.random_complete_lengths(rng, ndist))
        if rng.random() < 0.5:
            code["cl_ops"] = W.rle_ops(code["ll_lens"] + code["d_lens"])
        blocks = [("dynamic", random_tokens(rng, nlen, ndist, int(rng.integers(200, 601))), code)]
        s = write(blocks)
        assert len(s) <= LONG
        out.append((s, spelled(blocks)))
    return out


# ---- the case list ----

def form_blocks(case, form):
    """the blocks behind case.short / case.long (a case that is long by nature has no noise in front)"""
    return case.blocks if form == "short" or case.short is None else long_blocks(case.blocks)


@functools.lru_cache(maxsize=None)
def base_cases():
    """[Case]: short / long are streams (None where the form does not exist)"""
    cases = []
    for name, blocks in base_blocks().items():
        s = write(blocks)
        if name == "deep_all":
            short, long_ = None, s
        else:
            short, long_ = s, None if name == "bomb" else write(long_blocks(blocks))
        assert short is None or len(short) <= LONG, name
        assert long_ is None or len(long_) > LONG, name
        cases.append(Case(name, blocks, short, long_, name != "no_dist_needed"))
    return cases


def flip(s, bit):
    return s[:bit >> 3] + bytes([s[bit >> 3] ^ (1 << (bit & 7))]) + s[(bit >> 3) + 1:]


def derived(s, seed, header=True, nflips=30):
    """cuts, one byte more, every one-bit flip of the first 24 bytes (header), seeded flips after them"""
    out = [s[:n] for n in range(len(s))] if len(s) < 64 else [s[:-1], s[:-2], s[:-3], s[:len(s) // 2]]
    out.append(s + b"\x00")
    head = min(24, len(s)) * 8
    if header:
        out += [flip(s, b) for b in range(head)]
    if len(s) * 8 > head:
        rng = np.random.default_rng(seed)
        out += [flip(s, int(b)) for b in rng.integers(head, len(s) * 8, nflips)]
    return out


def case_streams(case):
    """form -> [the base stream, then its derived ones]"""
    forms = {}
    seed = sum(case.name.encode())
    if case.short is not None:
        forms["short"] = [case.short] + derived(case.short, seed)
    if case.long is not None:
        forms["long"] = [case.long] + derived(case.long, seed + 1, header=False)
    return forms


@functools.lru_cache(maxsize=None)
def all_cases():
    """[(label, stream, zlib's class, zlib's bytes)] over every base case, its forms and their derived streams,
    and wave64 with a few derived ones each"""
    out = []
    for c in base_cases():
        for form, streams in case_streams(c).items():
            for k, s in enumerate(streams):
                out.append(("%s/%s/%d" % (c.name, form, k), s) + R.inflate_class(s))
    rng = np.random.default_rng(64)
    for i, (s, _) in enumerate(wave64(1)):
        more = [s, s[:-1], s[:len(s) // 2], s + b"\x00"] + [flip(s, int(b)) for b in rng.integers(0, 24 * 8, 8)]
        more += [flip(s, int(b)) for b in rng.integers(24 * 8, len(s) * 8, 4)]
        for k, x in enumerate(more):
            out.append(("wave64/%d/%d" % (i, k), x) + R.inflate_class(x))
    return out
