"""A bit-exact raw DEFLATE writer for the tests, from RFC 1951 alone: the caller
chooses every block type, every code length, every code-length symbol and the
spelling of every match, so that a stream can be shaped as no compressor shapes
it.  Nothing here decodes; what a stream means is asked of zlib (tests/db_ref.py)
and of spell() below, which reads the token lists, not the bits."""
import heapq
from math import gcd

# RFC 1951 3.2.5: length symbols 257..285 and distance symbols 0..29, as the tables stand there
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
            258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)  # 3.2.7
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8  # 3.2.6
FIXED_D = [5] * 32
EOB = "eob"


class BitWriter:
    """Bits into bytes, least significant bit of each byte first.  The pending
    bits are flushed at every call, so the cost is linear in the output."""

    def __init__(self):
        self.out = bytearray()
        self.acc = self.n = 0

    def bits(self, v, k):
        """the k low bits of v, least significant first (everything but a Huffman code)"""
        assert 0 <= v < (1 << k)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, k):
        """a Huffman code of k bits, most significant first"""
        assert k > 0 and 0 <= code < (1 << k)
        self.bits(int(format(code, "0%db" % k)[::-1], 2), k)

    def repeat(self, v, k, count):
        """bits(v, k) count times: whole periods of lcm(k, 8) bits are appended as bytes"""
        while count and self.n:
            self.bits(v, k)
            count -= 1
        per = 8 // gcd(k, 8)  # repeats in one period
        if count >= per:
            p = BitWriter()
            for _ in range(per):
                p.bits(v, k)
            assert p.n == 0
            self.out += bytes(p.out) * (count // per)
            count %= per
        for _ in range(count):
            self.bits(v, k)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def getvalue(self):
        """the bytes so far, the last one padded with zero bits"""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """the code of each symbol (None where the length is 0), RFC 1951 3.2.2"""
    count = [0] * (max(lengths, default=0) + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * len(count), 0
    for l in range(1, len(count)):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = []
    for l in lengths:
        codes.append(nxt[l] if l else None)
        nxt[l] += 1 if l else 0
    return codes


def kraft(lengths, unit=15):
    """the code space used, in units of 2^-unit: 2^unit is complete"""
    return sum(1 << (unit - l) for l in lengths if l)


class Code:
    def __init__(self, lengths):
        self.lens, self.codes = list(lengths), canonical(lengths)

    def put(self, w, sym):
        assert self.lens[sym], "symbol %d has no code" % sym
        w.huff(self.codes[sym], self.lens[sym])


def put_tokens(w, ll, d, tokens):
    """tokens: a literal 0..255, EOB, a match (length symbol, length extra,
    distance symbol, distance extra), or ("raw", value, nbits)"""
    for t in tokens:
        if t == EOB:
            ll.put(w, 256)
        elif isinstance(t, int):
            ll.put(w, t)
        elif t[0] == "raw":
            w.bits(t[1], t[2])
        else:
            ls, le, ds, de = t
            ll.put(w, ls)
            if ls - 257 < 29 and LEN_EXTRA[ls - 257]:
                w.bits(le, LEN_EXTRA[ls - 257])
            d.put(w, ds)
            if ds < 30 and DIST_EXTRA[ds]:
                w.bits(de, DIST_EXTRA[ds])


def spell(tokens, out):
    """what the tokens say, appended to out: the tables above and nothing else"""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t != EOB:
            ls, le, ds, de = t
            length, dist = LEN_BASE[ls - 257] + le, DIST_BASE[ds] + de
            assert le < (1 << LEN_EXTRA[ls - 257]) and de < (1 << DIST_EXTRA[ds]) and dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
    return out


def stored_block(w, final, data):
    assert len(data) <= 0xFFFF
    w.bits(int(final), 1)
    w.bits(0, 2)
    w.align()
    w.raw(len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + bytes(data))


def fixed_block(w, final, tokens):
    w.bits(int(final), 1)
    w.bits(1, 2)
    put_tokens(w, Code(FIXED_LL), Code(FIXED_D), tokens)


def plain_ops(lengths):
    """every length as its own code-length symbol"""
    return [(l, 0) for l in lengths]


def rle_ops(lengths, rep16=True, zeros=True):
    """the lengths with a 16 wherever a run of equal ones allows and, with
    zeros, 17 / 18 for runs of zeros; runs do not stop at the nlen | ndist boundary"""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        l, run = lengths[i], 1
        while i + run < n and lengths[i + run] == l:
            run += 1
        i += run
        if l == 0 and zeros:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r - 11))
                run -= r
            if run >= 3:
                ops.append((17, run - 3))
                run = 0
            ops += [(0, 0)] * run
            continue
        ops.append((l, 0))
        run -= 1
        while rep16 and run >= 3:
            r = min(run, 6)
            ops.append((16, r - 3))
            run -= r
        ops += [(l, 0)] * run
    return ops


def limited_huffman(freq, maxlen):
    """code lengths for the symbols of non-zero frequency, complete, none above
    maxlen: Huffman's, with the frequencies flattened until it fits"""
    freq = dict(freq)
    assert len(freq) >= 2
    while True:
        heap = [(f, s, (s,)) for s, f in sorted(freq.items())]
        heapq.heapify(heap)
        lens = dict.fromkeys(freq, 0)
        while len(heap) > 1:
            fa, sa, a = heapq.heappop(heap)
            fb, sb, b = heapq.heappop(heap)
            for s in a + b:
                lens[s] += 1
            heapq.heappush(heap, (fa + fb, min(sa, sb), a + b))
        if max(lens.values()) <= maxlen:
            return lens
        freq = {s: f // 2 + 1 for s, f in freq.items()}


def dynamic_block(w, final, ll_lens, d_lens, tokens, cl_ops=None, cl_lens=None, hclen=19):
    """ll_lens: the HLIT + 257 literal/length lengths, d_lens: the HDIST + 1
    distance lengths; cl_ops: the (code-length symbol, extra bits' value) sequence
    that spells them (default: one symbol per length); cl_lens: the 19 lengths of
    the code-length code, by symbol (default: a complete code over the symbols
    used); hclen: how many of them are written."""
    assert 257 <= len(ll_lens) and 1 <= len(d_lens) and 4 <= hclen <= 19
    if cl_ops is None:
        cl_ops = plain_ops(list(ll_lens) + list(d_lens))
    if cl_lens is None:
        freq = {}
        for s, _ in cl_ops:
            freq[s] = freq.get(s, 0) + 1
        for s in (0, 18):  # a single one-bit code-length code is incomplete: give it company
            if len(freq) < 2:
                freq.setdefault(s, 0)
        got = limited_huffman(freq, 7)
        cl_lens = [got.get(s, 0) for s in range(19)]
    assert all(cl_lens[s] == 0 for s in CL_ORDER[hclen:]), "hclen cuts off a used symbol"
    w.bits(int(final), 1)
    w.bits(2, 2)
    w.bits(len(ll_lens) - 257, 5)
    w.bits(len(d_lens) - 1, 5)
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lens[s], 3)
    cl = Code(cl_lens)
    for s, extra in cl_ops:
        cl.put(w, s)
        if s >= 16:
            w.bits(extra, CL_EXTRA[s])
    put_tokens(w, Code(ll_lens), Code(d_lens), tokens)


def expand_ops(cl_ops):
    """the lengths that a code-length sequence spells (to check a hand-written one)"""
    out = []
    for s, extra in cl_ops:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + extra)
        else:
            out += [0] * ((3 if s == 17 else 11) + extra)
    return out


def random_complete_lengths(rng, nsym, maxlen=15):
    """nsym lengths of a complete code, in a random order: one leaf, and leaves
    shallower than maxlen split until there are nsym (one symbol: a single
    one-bit code, which is all that inflate accepts of an incomplete code)"""
    if nsym == 1:
        return [1]
    assert nsym <= (1 << maxlen)
    leaves = [0]
    while len(leaves) < nsym:
        open_ = [i for i, l in enumerate(leaves) if l < maxlen]
        i = open_[int(rng.integers(len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return [leaves[int(i)] for i in rng.permutation(nsym)]
