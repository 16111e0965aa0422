// calls_core.h -- the head of a program-text line, once: what a byte is to the
// line that holds it (bufio.ScanLines with its '\r' drop), the two head scanners
// (Deserialize's Ident / Char / Parse walk, prog/encoding.go:159-180 and :740-828;
// CallSet's byte search, :841-860) and the call-name table's hash and probe.
// No HIP here: the kernels of calls.hip read through it from LDS and from global
// memory, tests/progtext_driver.cc from exact-size heap blocks under ASan +
// UBSan.  Whoever includes this has syzsig.h's codes.
//
// A source S gives the bytes of one line's surroundings by absolute position:
//   S.byte(q)         the byte at q (only asked for q < S.lim that are not past the end)
//   S.ends_before(q)  q is at or past the end of the line's program (or of what
//                     the source knows to be the line)
//   S.lim             positions from here on are outside the source's window:
//                     whatever depends on them is undecided (kLnMore)
// The scanners only move forward and stop at the first kLnEol or kLnMore, so a
// source is never asked about a position past the line's end + 1.
#pragma once

#include <cstdint>

#include "common.h"

namespace syz {

constexpr int kLnEol = 256, kLnMore = 257;
constexpr uint64_t kPtMaxLine = SYZSIG_PROGTEXT_MAX_LINE;
constexpr uint32_t kNoCall = 0xffffffffu;

// What position q is to its line: a byte of its content, its end (a '\n', the
// program's end, or the one '\r' that ScanLines drops before either), or unknown.
template <class Src>
SYZ_HD int line_at(const Src& S, uint64_t q)
{
	if (q >= S.lim)
		return kLnMore;
	if (S.ends_before(q))
		return kLnEol;
	const int b = S.byte(q);
	if (b == '\n')
		return kLnEol;
	if (b == '\r') {
		if (q + 1 >= S.lim)
			return kLnMore;
		if (S.ends_before(q + 1) || S.byte(q + 1) == '\n')
			return kLnEol;
	}
	return b;
}

SYZ_HD bool pt_is_ident(int c)
{
	return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_' || c == '$';
}
SYZ_HD bool pt_is_ws(int c) { return c == ' ' || c == '\t'; }

enum HeadKind : uint32_t {
	kHdCall = 0,  // a call line: the name is [lo, hi)
	kHdSkip,      // empty after the '\r' drop, or a comment
	kHdErr,       // status = the SYZSIG_PT_* code
	kHdMore,      // the window ended before the head did
};

struct Head {
	uint32_t kind;
	uint32_t status;  // kHdErr: the code.  kHdCall in Deserialize mode: what Parse('(') says once the
	                  // name is known (SYZSIG_PT_OK or SYZSIG_PT_BAD_HEAD); CallSet mode: SYZSIG_PT_OK
	uint64_t lo, hi;
};

SYZ_HD Head head_of(uint32_t kind, uint32_t status = 0, uint64_t lo = 0, uint64_t hi = 0)
{
	Head h;
	h.kind = kind;
	h.status = status;
	h.lo = lo;
	h.hi = hi;
	return h;
}

// I W* ( '=' W* I W* )? '(' from the line's first byte, in the parser's order.
template <class Src>
SYZ_HD Head head_deserialize(const Src& S, uint64_t p)
{
	int c = line_at(S, p);
	if (c == kLnMore)
		return head_of(kHdMore);
	if (c == kLnEol || c == '#')
		return head_of(kHdSkip);
	uint64_t q = p;
	while (pt_is_ident(c))
		c = line_at(S, ++q);
	if (c == kLnMore)
		return head_of(kHdMore);
	if (q == p)
		return head_of(kHdErr, SYZSIG_PT_BAD_IDENT);
	uint64_t lo = p, hi = q;
	while (pt_is_ws(c))
		c = line_at(S, ++q);
	if (c == kLnMore)
		return head_of(kHdMore);
	if (c == kLnEol)
		return head_of(kHdErr, SYZSIG_PT_BAD_HEAD);  // Char() at EOF
	if (c == '=') {
		c = line_at(S, ++q);
		while (pt_is_ws(c))
			c = line_at(S, ++q);
		if (c == kLnMore)
			return head_of(kHdMore);
		lo = q;
		while (pt_is_ident(c))
			c = line_at(S, ++q);
		if (c == kLnMore)
			return head_of(kHdMore);
		if (q == lo)
			return head_of(kHdErr, SYZSIG_PT_BAD_IDENT);
		hi = q;
		while (pt_is_ws(c))
			c = line_at(S, ++q);
		if (c == kLnMore)
			return head_of(kHdMore);
	}
	return head_of(kHdCall, c == '(' ? SYZSIG_PT_OK : SYZSIG_PT_BAD_HEAD, lo, hi);
}

// ln[:IndexByte(ln, '(')], restarted after its first '=' and the spaces behind it
template <class Src>
SYZ_HD Head head_callset(const Src& S, uint64_t p)
{
	int c = line_at(S, p);
	if (c == kLnMore)
		return head_of(kHdMore);
	if (c == kLnEol || c == '#')
		return head_of(kHdSkip);
	uint64_t q = p, eq = ~0ull;
	while (c != '(') {
		if (c == kLnMore)
			return head_of(kHdMore);
		if (c == kLnEol)
			return head_of(kHdErr, SYZSIG_PT_NO_BRACKET);
		if (c == '=' && eq == ~0ull)
			eq = q;
		c = line_at(S, ++q);
	}
	uint64_t lo = p;
	if (eq != ~0ull) {
		lo = eq + 1;
		while (lo < q && S.byte(lo) == ' ')  // (spaces alone: a tab stays in the name)
			lo++;
	}
	if (lo == q)
		return head_of(kHdErr, SYZSIG_PT_EMPTY_NAME);
	return head_of(kHdCall, SYZSIG_PT_OK, lo, q);
}

template <class Src>
SYZ_HD Head head_scan(const Src& S, uint64_t p, uint32_t mode)
{
	return mode == SYZSIG_PROGTEXT_CALLSET ? head_callset(S, p) : head_deserialize(S, p);
}

// ---- the name table ----

SYZ_HD uint64_t fmix64(uint64_t k)
{
	k ^= k >> 33;
	k *= 0xff51afd7ed558ccdull;
	k ^= k >> 33;
	k *= 0xc4ceb9fe1a85ec53ull;
	k ^= k >> 33;
	return k;
}

// FNV-1a over the bytes, then murmur3's 64-bit finalizer (tests/calltab_keys.py restates it)
template <class Bytes>
SYZ_HD uint64_t name_hash(const Bytes& B, uint64_t lo, uint64_t hi)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (uint64_t q = lo; q < hi; q++)
		h = (h ^ (uint64_t)(uint8_t)B.byte(q)) * 0x100000001b3ull;
	return fmix64(h);
}

struct alignas(16) CallSlot {
	uint64_t hash;
	uint32_t id;  // kNoCall: empty
	uint32_t len;
};

// nslots = mask + 1 is a power of two >= 2 n: an empty slot ends every probe
struct CallTabView {
	const CallSlot* slots;
	uint64_t mask;
	const uint8_t* names;
	const uint64_t* name_off;
	uint32_t n;
};

SYZ_HD uint64_t calltab_home(uint64_t hash, uint64_t mask) { return hash & mask; }

// the id of the name B[lo, hi), or kNoCall: equal hash and length, then equal bytes
template <class Bytes>
SYZ_HD uint32_t calltab_find(const CallTabView& T, const Bytes& B, uint64_t lo, uint64_t hi)
{
	const uint64_t len = hi - lo;
	if (len == 0 || len > 0xffffffffull)
		return kNoCall;
	const uint64_t h = name_hash(B, lo, hi);
	uint64_t s = calltab_home(h, T.mask);
	for (uint64_t k = 0; k <= T.mask; k++, s = (s + 1) & T.mask) {
		const CallSlot e = T.slots[s];
		if (e.id == kNoCall)
			return kNoCall;
		if (e.hash != h || e.len != (uint32_t)len)
			continue;
		const uint8_t* nm = T.names + T.name_off[e.id];
		uint64_t i = 0;
		while (i < len && nm[i] == (uint8_t)B.byte(lo + i))
			i++;
		if (i == len)
			return e.id;
	}
	return kNoCall;
}

// A line record of calls.hip: what one line turned out to be.
constexpr uint32_t kRecCall = 0u << 28, kRecSkip = 1u << 28, kRecErr = 2u << 28, kRecUnknown = 3u << 28,
                   kRecPending = 4u << 28, kRecKindMask = 0xfu << 28, kRecValMask = ~kRecKindMask;

// The record of the line at p: the scan, then the lookup where the mode asks for
// one before it looks at the '('.
template <class Src>
SYZ_HD uint32_t line_record(const Src& S, uint64_t p, uint32_t mode, const CallTabView& T)
{
	const Head h = head_scan(S, p, mode);
	if (h.kind == kHdMore)
		return kRecPending;
	if (h.kind == kHdSkip)
		return kRecSkip;
	if (h.kind == kHdErr)
		return kRecErr | h.status;
	const uint32_t id = calltab_find(T, S, h.lo, h.hi);
	if (mode == SYZSIG_PROGTEXT_CALLSET)
		return id == kNoCall ? kRecUnknown : kRecCall | id;
	if (id == kNoCall)
		return kRecErr | SYZSIG_PT_UNKNOWN_CALL;
	return h.status != SYZSIG_PT_OK ? kRecErr | h.status : kRecCall | id;
}

}  // namespace syz
