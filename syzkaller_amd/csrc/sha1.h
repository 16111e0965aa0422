// sha1.h -- pkg/hash/hash.go:18-26 (Hash = sha1.Sum of the pieces' concatenation)
// for one message per lane: FIPS 180 SHA-1 over a 16-word rolling schedule, and
// the readers that hand it a message's bytes at any byte alignment.
//
// No HIP types here (SYZ_HD / SYZ_HDM only), so that the same code runs on the CPU in
// tests/sigs_driver.cc: there the readers work on exact-size heap blocks under
// ASan, which is the check that no byte outside a message is ever loaded.
//
// A reader sees its message as a stream of ALIGNED 32-bit words: word(k) is the
// aligned word k words past the one that holds the message's first byte, and
// sh = the first byte's position inside that word.  Message word k is then the
// funnel shift of word(k) and word(k + 1) by sh bytes (v_alignbyte on the
// device), byte-swapped to big-endian.  Bytes of an aligned word that lie
// outside the message are never used: a block that is not made of data alone
// masks them away before the padding goes in.
#pragma once

#include <stdint.h>

#include "common.h"

// SYZ_HD for member functions (the host form of SYZ_HD says `static`)
#if defined(__HIPCC__)
#define SYZ_HDM __host__ __device__ __forceinline__
#else
#define SYZ_HDM inline
#endif

namespace syz {

SYZ_HD uint32_t sha1_rotl(uint32_t x, int n)
{
#if defined(__clang__)
	return __builtin_rotateleft32(x, n);
#else
	return (x << n) | (x >> (32 - n));
#endif
}

// ({hi, lo} >> 8 sh) & 0xffffffff, sh < 4
SYZ_HD uint32_t sha1_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
	return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
#endif
}

// One 64-byte block.  The 80 rounds are unrolled, so every index into w is a
// constant and the schedule stays in 16 registers (a runtime index would put
// it into scratch).  Ch, Maj and Parity are written plainly: the compiler picks
// v_bfi / v_xor3 for them and v_alignbit for the rotates.
SYZ_HD void sha1_block(uint32_t (&h)[5], uint32_t (&w)[16])
{
	uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
	for (int t = 0; t < 80; t++) {
		uint32_t x;
		if (t < 16) {
			x = w[t];
		} else {
			x = sha1_rotl(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
			w[t & 15] = x;
		}
		uint32_t f, k;
		if (t < 20) {
			f = (b & c) | (~b & d);
			k = 0x5A827999u;
		} else if (t < 40) {
			f = b ^ c ^ d;
			k = 0x6ED9EBA1u;
		} else if (t < 60) {
			f = (b & c) | (b & d) | (c & d);
			k = 0x8F1BBCDCu;
		} else {
			f = b ^ c ^ d;
			k = 0xCA62C1D6u;
		}
		const uint32_t tmp = sha1_rotl(a, 5) + f + e + k + x;
		e = d;
		d = c;
		c = sha1_rotl(b, 30);
		b = a;
		a = tmp;
	}
	h[0] += a;
	h[1] += b;
	h[2] += c;
	h[3] += d;
	h[4] += e;
}

// The number of 64-byte blocks of a message of len bytes: the data, 0x80, zeros, the 8-byte bit length.
SYZ_HD uint64_t sha1_blocks(uint64_t len) { return (len + 72) >> 6; }

// The SHA-1 of the len bytes (len <= 2^28: the bit length fits the low length
// word) behind reader r.  r.word(k) must be safe for every k <= 16 * blocks;
// r.plain(b) says that block b's 17 aligned words can be loaded by r.load(k)
// without a check.  The loop is bounded by the block count.
template <typename R>
SYZ_HD void sha1_msg(const R& r, uint32_t sh, uint64_t len, uint32_t (&h)[5])
{
	h[0] = 0x67452301u;
	h[1] = 0xEFCDAB89u;
	h[2] = 0x98BADCFEu;
	h[3] = 0x10325476u;
	h[4] = 0xC3D2E1F0u;
	const uint64_t nb = sha1_blocks(len);
	uint32_t w[16];
	uint32_t lo = r.word(0);
	for (uint64_t b = 0; b < nb; b++) {
		const uint64_t p0 = b << 6;
		if (p0 + 64 <= len && r.plain(b)) {
#pragma unroll
			for (int i = 0; i < 16; i++) {
				const uint32_t hi = r.load(b * 16 + i + 1);
				w[i] = __builtin_bswap32(sha1_alignbyte(hi, lo, sh));
				lo = hi;
			}
		} else {
#pragma unroll
			for (int i = 0; i < 16; i++) {
				const uint32_t hi = r.word(b * 16 + i + 1);
				uint32_t x = __builtin_bswap32(sha1_alignbyte(hi, lo, sh));
				lo = hi;
				const uint64_t p = p0 + 4 * i;
				if (p + 4 > len) {  // the message ends inside or before this word
					const uint32_t rem = p < len ? (uint32_t)(len - p) : 0;  // data bytes of it: 0 .. 3
					x = rem ? x & (0xFFFFFFFFu << (8 * (4 - rem))) : 0;
					if (p <= len)
						x |= 0x80u << (8 * (3 - rem));
				}
				w[i] = x;
			}
			if (b == nb - 1) {  // (words 14 and 15 of the last block lie past the 0x80: zero so far)
				w[14] = (uint32_t)(len >> 29);
				w[15] = (uint32_t)(len << 3);
			}
		}
		sha1_block(h, w);
	}
}

// A message in memory, [s, s + len): the aligned words wholly inside it are
// loaded as words, the (at most two) that reach past its ends byte by byte with
// the outside bytes as zero.  Nothing outside [s, s + len) is read.
struct Sha1MemReader {
	uintptr_t s, e;  // the message's first byte, and one past its last
	uintptr_t a0;    // s rounded down to 4
	SYZ_HDM static Sha1MemReader make(const uint8_t* base, uint64_t off, uint64_t len)
	{
		const uintptr_t p = (uintptr_t)base + off;
		return Sha1MemReader{p, p + len, p & ~(uintptr_t)3};
	}
	SYZ_HDM uint32_t shift() const { return (uint32_t)(s & 3); }
	SYZ_HDM bool plain(uint64_t b) const { return a0 + 64 * b >= s && a0 + 64 * b + 68 <= e; }
	SYZ_HDM uint32_t load(uint64_t k) const { return *reinterpret_cast<const uint32_t*>(a0 + 4 * k); }
	SYZ_HDM uint32_t word(uint64_t k) const
	{
		const uintptr_t p = a0 + 4 * k;
		if (p >= s && p + 4 <= e)
			return *reinterpret_cast<const uint32_t*>(p);
		uint32_t v = 0;
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (p + j >= s && p + j < e)
				v |= (uint32_t)*reinterpret_cast<const uint8_t*>(p + j) << (8 * j);
		return v;
	}
};

// A message inside a staged span: st[0 .. nwords) holds the span's bytes from
// an aligned address on, the message starts at byte `pos` of it.  An index past
// the array (only behind the message's last byte) is clamped.
struct Sha1StageReader {
	const uint32_t* st;
	uint32_t q0, last;
	SYZ_HDM static Sha1StageReader make(const uint32_t* st, uint32_t nwords, uint32_t pos)
	{
		return Sha1StageReader{st, pos >> 2, nwords - 1};
	}
	SYZ_HDM bool plain(uint64_t) const { return true; }
	SYZ_HDM uint32_t load(uint64_t k) const { return word(k); }
	SYZ_HDM uint32_t word(uint64_t k) const
	{
		const uint64_t i = q0 + k;
		return st[i < last ? i : last];
	}
};

// A Sig as the sets keep it (hash.go:14 `type Sig [sha1.Size]byte`): three u64
// words whose word order is memcmp's byte order -- bytes 0..7 and 8..15
// big-endian, bytes 16..19 in the high half of the third; its low half is free
// (a batch's sort carries the arrival index there, a set keeps it zero).
SYZ_HD void sig_pack(const uint8_t* p, uint32_t low, uint64_t (&w)[3])
{
	uint64_t a = 0, b = 0, c = 0;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		a = a << 8 | p[i];
		b = b << 8 | p[8 + i];
	}
#pragma unroll
	for (int i = 0; i < 4; i++)
		c = c << 8 | p[16 + i];
	w[0] = a;
	w[1] = b;
	w[2] = c << 32 | low;
}

SYZ_HD void sig_unpack(const uint64_t (&w)[3], uint8_t* p)
{
#pragma unroll
	for (int i = 0; i < 8; i++) {
		p[i] = (uint8_t)(w[0] >> (56 - 8 * i));
		p[8 + i] = (uint8_t)(w[1] >> (56 - 8 * i));
	}
#pragma unroll
	for (int i = 0; i < 4; i++)
		p[16 + i] = (uint8_t)(w[2] >> (56 - 8 * i));
}

}  // namespace syz
