// inflate_core.h -- RFC 1951 (raw DEFLATE) for one stream: the decoder behind
// syzsig_inflate_dev, which reads the values of pkg/db (pkg/db/db.go:257-263:
// flate.NewReader over the record's valLen bytes, read until the final block).
//
// No HIP types here (SYZ_HD only), so that the same code runs on the CPU in
// tests/db_driver.cc under ASan + UBSan, from and into heap blocks of exactly
// the stream's and the output's size.
//
// inflate_stream() decodes in[0 .. n) serially, one byte loaded at a time and
// only when a bit of it is needed, so no byte outside the range is read and the
// bytes consumed are known exactly (the TRAILING class).  With out == nullptr it
// only counts: the lengths come from the symbols alone, and a distance is
// checked against the count.  With out given, every write is bounded by out_cap.
//
// Where RFC 1951 leaves a choice the decoder does what zlib 1.2.11's inflate()
// does, in the same order of "need these bits" and "check", so that a stream cut
// short and a stream that is wrong fall into the same classes as there:
//   - a code-length code with no symbol at all reads every length as one bit of
//     value 0 (inflate_table's empty table), and fails later at "no end-of-block";
//   - an incomplete code is accepted only as one single code of one bit, for the
//     literal/length and the distance code; its unused bit pattern is invalid when
//     it is met; an empty distance code is accepted until a distance is needed;
//   - a dynamic block whose literal/length code has no end-of-block symbol is
//     invalid before any of its symbols is decoded;
//   - a repeat code's extra bits are asked for before its checks.
//
// Tables.  Canonical Huffman decoding (count per length + symbols in code order)
// needs, per code, count[16] and symbol[n], and while the code is built the n
// lengths.  Tab is one array of 16-bit cells reached through get()/set(), so that
// the kernel can lay 64 lanes' tables side by side in LDS:
//   [0, 16)    count of the literal/length code ([0] = its longest length)
//   [16, 32)   count of the distance code      ([16] = its longest length)
//   [32, 48)   next free place per length, while a code is built
//   [48, 368)  per cell: bits 12..15 the length of symbol i (as read from the
//              header), bits 0..8 the symbol at place i of the code order;
//              literal/length at [48, 336), distance at [336, 368)
#pragma once

#include <stdint.h>

#include "common.h"

// SYZ_HD for member functions (the host form of SYZ_HD says `static`)
#ifndef SYZ_HDM
#if defined(__HIPCC__)
#define SYZ_HDM __host__ __device__ __forceinline__
#else
#define SYZ_HDM inline
#endif
#endif

namespace syz {

// the statuses of include/syzsig.h (SYZSIG_INFLATE_*), restated so that this header stands alone
constexpr uint8_t kInfOk = 0, kInfTruncated = 1, kInfInvalid = 2, kInfTrailing = 3, kInfTooLong = 4;

constexpr int kInfTabCells = 368;
constexpr int kInfLenCnt = 0, kInfDistCnt = 16, kInfNext = 32, kInfLenSym = 48, kInfDistSym = 336;
constexpr int kInfMaxLCodes = 286, kInfMaxDCodes = 30, kInfFixLCodes = 288;
// the order of the code-length code's lengths, RFC 1951 3.2.7, five bits each:
// 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
constexpr uint64_t kInfOrderLo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                                 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
constexpr uint64_t kInfOrderHi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;

// the tables of one stream as a plain array (the CPU driver; a kernel passes its own)
struct InflateTabArray {
	uint16_t c[kInfTabCells];
	SYZ_HDM uint32_t get(int i) const { return c[i]; }
	SYZ_HDM void set(int i, uint32_t v) { c[i] = (uint16_t)v; }
};

struct InflateResult {
	uint64_t out_len;    // bytes produced (meaningful when status is kInfOk)
	uint32_t stored, fixed, dynamic;  // block headers decoded
	uint8_t status;
};

// the bit reader: LSB first, a byte is loaded when one of its bits is asked for
struct InflateBits {
	const uint8_t* in;
	uint64_t n, pos;
	uint32_t buf, cnt;  // cnt < 8 between calls
	// the next k <= 16 bits into v; false: the input ended first
	SYZ_HDM bool take(uint32_t k, uint32_t& v)
	{
		while (cnt < k) {
			if (pos >= n)
				return false;
			buf |= (uint32_t)in[pos++] << cnt;
			cnt += 8;
		}
		v = buf & ((1u << k) - 1);
		buf >>= k;
		cnt -= k;
		return true;
	}
};

// Builds the canonical code of the nsym lengths held in the cells' high bits at
// sym0: counts at cnt0.  Returns 0: complete; > 0: incomplete; < 0: over-subscribed.
template <class Tab>
SYZ_HD int inflate_build(Tab& t, int cnt0, int sym0, int nsym)
{
	for (int l = 0; l < 16; l++)
		t.set(cnt0 + l, 0);
	for (int s = 0; s < nsym; s++) {
		const int l = (int)(t.get(sym0 + s) >> 12);
		t.set(cnt0 + l, t.get(cnt0 + l) + 1);
	}
	int left = 1, maxlen = 0;
	uint32_t next = 0;
	for (int l = 1; l < 16; l++) {
		const int c = (int)t.get(cnt0 + l);
		left = (left << 1) - c;
		if (left < 0)
			return -1;
		if (c)
			maxlen = l;
		t.set(kInfNext + l, next);
		next += (uint32_t)c;
	}
	for (int s = 0; s < nsym; s++) {
		const uint32_t cell = t.get(sym0 + s);
		const int l = (int)(cell >> 12);
		if (l) {
			const uint32_t at = t.get(kInfNext + l);
			t.set(kInfNext + l, at + 1);
			t.set(sym0 + (int)at, (t.get(sym0 + (int)at) & 0xF000u) | (uint32_t)s);
		}
	}
	t.set(cnt0, (uint32_t)maxlen);  // (the count of unused symbols is not needed)
	return left;
}

// One symbol of the code at (cnt0, sym0).  kInfOk: sym set; else the status.
template <class Tab>
SYZ_HD uint8_t inflate_symbol(InflateBits& b, const Tab& t, int cnt0, int sym0, uint32_t& sym)
{
	const int maxlen = (int)t.get(cnt0) ? (int)t.get(cnt0) : 1;  // an empty code still takes one bit
	int code = 0, first = 0, index = 0;
	for (int l = 1; l <= maxlen; l++) {
		uint32_t bit;
		if (!b.take(1, bit))
			return kInfTruncated;
		code |= (int)bit;
		const int c = (int)t.get(cnt0 + l);
		if (code - c < first) {
			sym = t.get(sym0 + index + (code - first)) & 0x1FFu;
			return kInfOk;
		}
		index += c;
		first = (first + c) << 1;
		code <<= 1;
	}
	return kInfInvalid;  // the unused pattern of an incomplete code
}

SYZ_HD uint32_t inflate_len_base(uint32_t s)  // s = symbol - 257, 0..28
{
	return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s >> 2) - 1));
}
SYZ_HD uint32_t inflate_len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
SYZ_HD uint32_t inflate_dist_base(uint32_t s)  // 0..29
{
	return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1));
}
SYZ_HD uint32_t inflate_dist_extra(uint32_t s) { return s < 4 ? 0 : (s >> 1) - 1; }

// The dynamic block's header into the tables.  kInfOk or the status.
template <class Tab>
SYZ_HD uint8_t inflate_dynamic_header(InflateBits& b, Tab& t)
{
	uint32_t v;
	if (!b.take(14, v))
		return kInfTruncated;
	const int nlen = (int)(v & 31) + 257, ndist = (int)((v >> 5) & 31) + 1, ncode = (int)(v >> 10) + 4;
	if (nlen > kInfMaxLCodes || ndist > kInfMaxDCodes)
		return kInfInvalid;
	// the code-length code: its 19 lengths sit where the distance code's cells are (built after them)
	for (int i = 0; i < 19; i++)
		t.set(kInfDistSym + i, 0);
	for (int i = 0; i < ncode; i++) {
		if (!b.take(3, v))
			return kInfTruncated;
		const int at = (int)((i < 12 ? kInfOrderLo >> (5 * i) : kInfOrderHi >> (5 * (i - 12))) & 31);
		t.set(kInfDistSym + at, v << 12);
	}
	const int cl = inflate_build(t, kInfDistCnt, kInfDistSym, 19);
	if (cl < 0 || (cl > 0 && t.get(kInfDistCnt) != 0))
		return kInfInvalid;  // over-subscribed, or incomplete (the empty one is met below)
	const bool empty = t.get(kInfDistCnt) == 0;
	// The nlen + ndist lengths go to the high bits of the cells from kInfLenSym on, up to 316 of them:
	// past 288 those are the cells whose low bits hold the code-length code's symbols, which stay.
	int have = 0;
	uint32_t prev = 0;
	while (have < nlen + ndist) {
		uint32_t sym;
		if (empty) {
			if (!b.take(1, v))
				return kInfTruncated;
			sym = 0;
		} else {
			const uint8_t st = inflate_symbol(b, t, kInfDistCnt, kInfDistSym, sym);
			if (st != kInfOk)
				return st;
		}
		if (sym < 16) {
			prev = sym;
			t.set(kInfLenSym + have, (t.get(kInfLenSym + have) & 0x0FFFu) | sym << 12);
			have++;
			continue;
		}
		uint32_t rep, len = 0;
		if (!b.take(sym == 16 ? 2 : sym == 17 ? 3 : 7, v))
			return kInfTruncated;
		if (sym == 16) {
			if (have == 0)
				return kInfInvalid;
			len = prev;
			rep = 3 + v;
		} else {
			rep = (sym == 17 ? 3 : 11) + v;
		}
		if (have + (int)rep > nlen + ndist)
			return kInfInvalid;
		prev = len;
		for (; rep; rep--, have++)
			t.set(kInfLenSym + have, (t.get(kInfLenSym + have) & 0x0FFFu) | len << 12);
	}
	if ((t.get(kInfLenSym + 256) >> 12) == 0)
		return kInfInvalid;  // no end-of-block code
	// The distance lengths to their own cells, now that the code-length code is done with.  The
	// target of i is the source of i + 288 - nlen > i: from the last one down.
	for (int i = ndist - 1; i >= 0; i--)
		t.set(kInfDistSym + i, t.get(kInfLenSym + nlen + i) & 0xF000u);
	const int ll = inflate_build(t, kInfLenCnt, kInfLenSym, nlen);
	if (ll < 0 || (ll > 0 && t.get(kInfLenCnt) != 1))
		return kInfInvalid;
	const int dl = inflate_build(t, kInfDistCnt, kInfDistSym, ndist);
	if (dl < 0 || (dl > 0 && t.get(kInfDistCnt) > 1))
		return kInfInvalid;
	return kInfOk;
}

template <class Tab>
SYZ_HD void inflate_fixed_tables(Tab& t)
{
	for (int s = 0; s < kInfFixLCodes; s++)
		t.set(kInfLenSym + s, (uint32_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8) << 12);
	inflate_build(t, kInfLenCnt, kInfLenSym, kInfFixLCodes);
	for (int s = 0; s < 32; s++)  // (30 and 31 take part in the code and are invalid when met)
		t.set(kInfDistSym + s, 5u << 12);
	inflate_build(t, kInfDistCnt, kInfDistSym, 32);
}

// in[0 .. n) -> out[0 .. out_cap) (out == nullptr: count only).  More than
// max_out bytes of output: kInfTooLong.  With out given, out_cap is the
// extent computed by a counting pass; a write past it ends the decode with
// kInfTooLong as well (it cannot happen for the same input).
template <class Tab>
SYZ_HD InflateResult inflate_stream(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t max_out,
                                    Tab& t)
{
	InflateResult r{0, 0, 0, 0, kInfOk};
	InflateBits b{in, n, 0, 0, 0};
	const uint64_t cap = out && out_cap < max_out ? out_cap : max_out;
	uint64_t pos = 0;
	bool have_fixed = false;
	uint32_t v, last = 0;
	while (!last) {
		if (!b.take(3, v)) {
			r.status = kInfTruncated;
			return r;
		}
		last = v & 1;
		const uint32_t type = v >> 1;
		if (type == 3) {
			r.status = kInfInvalid;
			return r;
		}
		if (type == 0) {
			r.stored++;
			b.buf = 0;  // to the byte boundary
			b.cnt = 0;
			if (n - b.pos < 4) {
				r.status = kInfTruncated;
				return r;
			}
			const uint32_t len = in[b.pos] | (uint32_t)in[b.pos + 1] << 8;
			const uint32_t nlen = in[b.pos + 2] | (uint32_t)in[b.pos + 3] << 8;
			b.pos += 4;
			if (len != (nlen ^ 0xFFFFu)) {
				r.status = kInfInvalid;
				return r;
			}
			// (zlib copies what is there before it asks for more: too long comes before truncated)
			const uint64_t avail = n - b.pos, take = len < avail ? len : avail;
			if (take > cap - pos) {
				r.status = kInfTooLong;
				return r;
			}
			if (out)
				for (uint64_t i = 0; i < take; i++)
					out[pos + i] = in[b.pos + i];
			pos += take;
			b.pos += take;
			if (take < len) {
				r.status = kInfTruncated;
				return r;
			}
			continue;
		}
		if (type == 1) {
			r.fixed++;
			if (!have_fixed)
				inflate_fixed_tables(t);
			have_fixed = true;
		} else {
			r.dynamic++;
			have_fixed = false;
			const uint8_t st = inflate_dynamic_header(b, t);
			if (st != kInfOk) {
				r.status = st;
				return r;
			}
		}
		// Every iteration consumes at least one bit of in[0 .. n) or returns: bounded by 8 n.
		for (;;) {
			uint32_t sym;
			uint8_t st = inflate_symbol(b, t, kInfLenCnt, kInfLenSym, sym);
			if (st != kInfOk) {
				r.status = st;
				return r;
			}
			if (sym < 256) {
				if (pos >= cap) {
					r.status = kInfTooLong;
					return r;
				}
				if (out)
					out[pos] = (uint8_t)sym;
				pos++;
				continue;
			}
			if (sym == 256)
				break;
			sym -= 257;
			if (sym >= 29) {
				r.status = kInfInvalid;
				return r;
			}
			uint32_t len = inflate_len_base(sym), dist, ds;
			if (!b.take(inflate_len_extra(sym), v)) {
				r.status = kInfTruncated;
				return r;
			}
			len += v;
			st = inflate_symbol(b, t, kInfDistCnt, kInfDistSym, ds);
			if (st != kInfOk) {
				r.status = st;
				return r;
			}
			if (ds >= 30) {
				r.status = kInfInvalid;
				return r;
			}
			dist = inflate_dist_base(ds);
			if (!b.take(inflate_dist_extra(ds), v)) {
				r.status = kInfTruncated;
				return r;
			}
			dist += v;
			if (dist > pos) {
				r.status = kInfInvalid;  // before the start of this stream's output
				return r;
			}
			if (len > cap - pos) {
				r.status = kInfTooLong;
				return r;
			}
			if (out)
				for (uint32_t i = 0; i < len; i++)  // (dist < len: the periodic fill, byte by byte)
					out[pos + i] = out[pos + i - dist];
			pos += len;
		}
	}
	r.out_len = pos;
	if (b.pos < n)
		r.status = kInfTrailing;
	return r;
}

}  // namespace syz
