// deflate_core.h -- RFC 1951 (raw DEFLATE) for one value: the compressor behind
// syzsig_deflate_dev and syzsig_deflate_host, which writes the values of pkg/db
// (pkg/db/db.go:147-175 serializeRecord: the stream that deserializeRecord,
// :257-263, reads back to val).
//
// No HIP types here (SYZ_HD only), so that the same code runs on the CPU in
// tests/dbw_driver.cc under ASan + UBSan, from and into heap blocks of exactly
// the value's and the stream's size, and behind syzsig_deflate_host.
//
// What a stream is.  Greedy LZ77 (matches of 3..258 bytes at distances up to
// 32768) coded with the fixed Huffman code in one final block (BTYPE 01); when
// that is not smaller than the stored form, stored blocks of at most 65535
// bytes, the last one final.  So for n > 0 the stream has at most
// n + 5 * ceil(n / 65535) bytes.  No sync-flush block and no empty final block
// (Go's writer emits both; no reader needs them: DESIGN.md).  n = 0 gives no
// stream at all: serializeRecord writes valLen = 0 (db.go:158-159).
//
// Matches.  A head-only hash table of kDefTabCells 16-bit cells, reached through
// get()/set() so that a kernel can lay 64 lanes' tables side by side in LDS.  A
// cell holds the low 16 bits of the last position whose three bytes hashed to
// it, zero at the start.  The candidate of position p is the largest position
// below p with those low bits; it is taken only if it is at most 32768 back and
// its bytes compare equal to p's, one by one, for at least 3: a hash is never
// trusted, so a cell that is stale, wrapped (positions repeat every 65536) or
// still zero can cost a match and never produce a wrong one.  A match of 3 at a
// distance over 4096 is dropped (it codes no shorter than its literals).
//
// Determinism.  The stream depends on in[0 .. n) alone: the table is cleared
// first, and no byte outside the range is ever loaded -- not the two bytes a
// hash would want past the end either.  The counting call (out == nullptr) and
// the writing call run the same search, so their lengths agree.
#pragma once

#include <stdint.h>

#include "common.h"

#ifndef SYZ_HDM
#if defined(__HIPCC__)
#define SYZ_HDM __host__ __device__ __forceinline__
#else
#define SYZ_HDM inline
#endif
#endif

namespace syz {

constexpr int kDefHashBits = 9;
constexpr int kDefTabCells = 1 << kDefHashBits;
constexpr uint32_t kDefMinMatch = 3, kDefMaxMatch = 258, kDefMaxDist = 32768, kDefTooFar = 4096;
constexpr uint64_t kDefStoredChunk = 65535;

// the table of one value as a plain array (the CPU; a kernel passes its own)
struct DeflateTabArray {
	uint16_t c[kDefTabCells];
	SYZ_HDM uint32_t get(int i) const { return c[i]; }
	SYZ_HDM void set(int i, uint32_t v) { c[i] = (uint16_t)v; }
};

struct DeflateResult {
	uint64_t out_len;  // the stream's bytes
	bool stored;       // its form (false for n = 0: no stream)
	bool fits;         // the writing call: every byte was inside out_cap
};

// the stored form's size of n > 0 bytes
SYZ_HD uint64_t deflate_stored_len(uint64_t n) { return n + 5 * ((n + kDefStoredChunk - 1) / kDefStoredChunk); }

// the k <= 16 low bits of v, reversed (Huffman codes go most significant bit first)
SYZ_HD uint32_t deflate_rev(uint32_t v, uint32_t k)
{
	v = (v & 0x5555u) << 1 | (v >> 1 & 0x5555u);
	v = (v & 0x3333u) << 2 | (v >> 2 & 0x3333u);
	v = (v & 0x0F0Fu) << 4 | (v >> 4 & 0x0F0Fu);
	v = (v & 0x00FFu) << 8 | (v >> 8 & 0x00FFu);
	return v >> (16 - k);
}

// the bit writer: LSB first.  out == nullptr: the bits are counted only.
struct DeflateBits {
	uint8_t* out;
	uint64_t cap, pos;  // bytes written (or counted)
	uint64_t buf;
	uint32_t cnt;  // < 8 between calls
	bool fits;
	SYZ_HDM void byte(uint32_t b)
	{
		if (out) {
			if (pos < cap)
				out[pos] = (uint8_t)b;
			else
				fits = false;
		}
		pos++;
	}
	// k <= 32 bits
	SYZ_HDM void put(uint32_t v, uint32_t k)
	{
		buf |= (uint64_t)v << cnt;
		cnt += k;
		while (cnt >= 8) {
			byte((uint32_t)buf & 0xFFu);
			buf >>= 8;
			cnt -= 8;
		}
	}
	SYZ_HDM void finish()
	{
		if (cnt)
			byte((uint32_t)buf & 0xFFu);
		buf = 0;
		cnt = 0;
	}
};

// a literal/length symbol 0..287 in the fixed code (RFC 1951 3.2.6)
SYZ_HD void deflate_fixed_sym(DeflateBits& b, uint32_t s)
{
	if (s < 144)
		b.put(deflate_rev(0x30 + s, 8), 8);
	else if (s < 256)
		b.put(deflate_rev(0x190 + (s - 144), 9), 9);
	else if (s < 280)
		b.put(deflate_rev(s - 256, 7), 7);
	else
		b.put(deflate_rev(0xC0 + (s - 280), 8), 8);
}

// a match of len 3..258 at dist 1..32768: the length symbol and its extra bits,
// the 5-bit distance symbol and its extra bits (the inverses of inflate_core.h's
// inflate_len_base / inflate_dist_base)
SYZ_HD void deflate_fixed_match(DeflateBits& b, uint32_t len, uint32_t dist)
{
	const uint32_t l = len - 3;
	if (l < 8) {
		deflate_fixed_sym(b, 257 + l);
	} else if (len == 258) {
		deflate_fixed_sym(b, 285);
	} else {
		const uint32_t e = (31 - (uint32_t)__builtin_clz(l)) - 2;
		deflate_fixed_sym(b, 257 + 4 * (e + 1) + (l >> e) - 4);
		b.put(l & ((1u << e) - 1), e);
	}
	const uint32_t d = dist - 1;
	if (d < 4) {
		b.put(deflate_rev(d, 5), 5);
	} else {
		const uint32_t e = (31 - (uint32_t)__builtin_clz(d)) - 1;
		b.put(deflate_rev(2 * (e + 1) + (d >> e) - 2, 5), 5);
		b.put(d & ((1u << e) - 1), e);
	}
}

SYZ_HD uint32_t deflate_hash(uint32_t w24) { return (w24 * 0x9E3779B1u) >> (32 - kDefHashBits); }

// The fixed-coded block of in[0 .. n), n > 0, through b (header, symbols,
// end-of-block, the last byte's padding).  Every iteration of the outer loop
// moves pos forward; the inner ones are bounded by 258.
template <class Tab>
SYZ_HD void deflate_fixed_block(const uint8_t* in, uint64_t n, DeflateBits& b, Tab& t)
{
	for (int i = 0; i < kDefTabCells; i++)
		t.set(i, 0);
	b.put(1 | 1 << 1, 3);  // BFINAL, BTYPE 01
	uint64_t pos = 0;
	// w = in[pos] | in[pos + 1] << 8 | in[pos + 2] << 16, of which the bytes inside the value are loaded
	uint32_t w = in[0];
	if (n > 1)
		w |= (uint32_t)in[1] << 8;
	if (n > 2)
		w |= (uint32_t)in[2] << 16;
	while (pos < n) {
		uint32_t len = 0, dist = 0;
		if (n - pos >= kDefMinMatch) {
			const uint32_t h = deflate_hash(w);
			// the largest position below pos with the cell's low 16 bits
			int64_t cand = (int64_t)((pos & ~0xFFFFull) | t.get((int)h));
			if (cand >= (int64_t)pos)
				cand -= 65536;
			t.set((int)h, (uint32_t)(pos & 0xFFFFu));
			if (cand >= 0 && pos - (uint64_t)cand <= kDefMaxDist) {
				const uint64_t left = n - pos;
				const uint32_t max = left < kDefMaxMatch ? (uint32_t)left : kDefMaxMatch;
				while (len < max && in[(uint64_t)cand + len] == in[pos + len])
					len++;
				dist = (uint32_t)(pos - (uint64_t)cand);
				if (len < kDefMinMatch || (len == kDefMinMatch && dist > kDefTooFar))
					len = 0;
			}
		}
		if (len == 0) {
			deflate_fixed_sym(b, w & 0xFFu);
			len = 1;
		} else {
			deflate_fixed_match(b, len, dist);
		}
		// forward by len: the positions passed inside a match go into the table too
		for (uint32_t k = 1; k <= len; k++) {
			pos++;
			w >>= 8;
			if (pos + 2 < n)
				w |= (uint32_t)in[pos + 2] << 16;
			if (k < len && n - pos >= kDefMinMatch)
				t.set((int)deflate_hash(w), (uint32_t)(pos & 0xFFFFu));
		}
	}
	deflate_fixed_sym(b, 256);
	b.finish();
}

// in[0 .. n) -> out[0 .. out_cap) (out == nullptr: count only).  With out
// given, out_len is still the whole stream's size and fits says whether it was
// all inside out_cap (no byte is written outside it either way).
// known_len: the length a counting call returned for the same value, or 0: the
// writing call then skips the match search of a value that goes out stored.
template <class Tab>
SYZ_HD DeflateResult deflate_stream(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t known_len,
                                    Tab& t)
{
	DeflateResult r{0, false, true};
	if (n == 0)
		return r;
	const uint64_t stored = deflate_stored_len(n);
	if (known_len != stored) {
		// count first: the form is decided by the size
		DeflateBits c{nullptr, 0, 0, 0, 0, true};
		uint64_t fixed = known_len;
		if (!known_len) {
			deflate_fixed_block(in, n, c, t);
			fixed = c.pos;
		}
		if (fixed < stored) {
			r.out_len = fixed;
			if (out) {
				DeflateBits b{out, out_cap, 0, 0, 0, true};
				deflate_fixed_block(in, n, b, t);
				r.fits = b.fits;
			}
			return r;
		}
	}
	r.stored = true;
	r.out_len = stored;
	if (out) {
		DeflateBits b{out, out_cap, 0, 0, 0, true};
		for (uint64_t at = 0; at < n; at += kDefStoredChunk) {
			const uint64_t left = n - at;
			const uint32_t k = left < kDefStoredChunk ? (uint32_t)left : (uint32_t)kDefStoredChunk;
			b.byte(at + k == n ? 1 : 0);  // BFINAL on the last, BTYPE 00, padding
			b.byte(k & 0xFFu);
			b.byte(k >> 8);
			b.byte(~k & 0xFFu);
			b.byte(~k >> 8 & 0xFFu);
			for (uint32_t i = 0; i < k; i++)
				b.byte(in[at + i]);
		}
		r.fits = b.fits;
	}
	return r;
}

}  // namespace syz
