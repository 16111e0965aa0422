// shrinkexpand.h -- prog.shrinkExpand's per-candidate rule (prog/hints.go:164-218),
// once: shared by comps.hip (syzsig_shrink_expand_dev: explicit queries) and
// hints.hip (syzsig_hint_mutants_dev: the windows of checkConstArg and
// checkDataArg).  The variants, the mutant, the lookup in a call's sorted
// pairs, the accept test with the special-int search and the replacer are
// device inlines; se_queries is syzsig_shrink_expand_dev's body for queries
// that are already on the device.
#pragma once

#include "segsort.h"

namespace syz {

constexpr uint32_t kCmVariants = 12;          // hints.go:165-191: 7 widths little-endian, 5 big-endian (not at width 1)
constexpr uint32_t kCmMaxSpecial = 4096;
constexpr uint32_t kCmMaxSeg = 0x7fffffffu;   // keys per segment

// Where se_queries leaves query q's distinct replacers, sorted ascending:
// cnt[q] of them from stage[voff[q * kCmVariants]] on; seg_len[q] = its accepted
// candidates before the dedup.  All in the context's sort workspaces
// (kWsSuMeta, kWsSuStage2): valid until the next entry point that sorts.
struct SeOut {
	const uint64_t* stage;
	const uint64_t* voff;
	const uint32_t* cnt;
	const uint32_t* seg_len;
	uint64_t* off;  // nq + 1 words of scratch for the caller's offsets
};

// hints.go:164-218 for nq > 0 device-resident queries against the maps
// (k_se_count, k_se_write, the segsort.h sort-unique, long path included).
// special_ints is the caller's host list (<= kCmMaxSpecial).  timed: the
// entry point's timed span starts at the first kernel.  Enqueues the sort; the
// caller fetches the counters (kCntError: a long segment without workspace).
int se_queries(syzsig_ctx* ctx, const char* what, const uint64_t* d_map_off, const uint64_t* d_pairs, uint64_t ncalls,
               uint64_t npairs, const uint32_t* d_q_call, const uint64_t* d_q_val, uint64_t nq,
               const uint64_t* special_ints, uint32_t nspecial, bool timed, SeOut* out);

#if defined(__HIPCC__)

__device__ __forceinline__ uint64_t cm_swap(uint64_t v, uint32_t width)  // prog/mutation.go:566-579
{
	if (width == 2)
		return __builtin_bswap16((uint16_t)v);
	if (width == 4)
		return __builtin_bswap32((uint32_t)v);
	if (width == 8)
		return __builtin_bswap64(v);
	return v;
}

// variant x of hints.go:165-191: widths 8, 4, 2, 1, -4, -2, -1 little-endian
// (x = 0..6), then 8, 4, 2, -4, -2 big-endian (x = 7..11)
__device__ __forceinline__ void cm_variant(uint32_t x, uint32_t& width, bool& expand, bool& be)
{
	const uint32_t le_w[7] = {8, 4, 2, 1, 4, 2, 1}, be_w[5] = {8, 4, 2, 4, 2};
	be = x >= 7;
	width = be ? be_w[x - 7] : le_w[x];
	expand = be ? x >= 10 : x >= 4;
}

__device__ __forceinline__ uint64_t cm_mask(uint32_t width) { return width == 8 ? ~0ull : (1ull << (8 * width)) - 1; }

__device__ __forceinline__ uint64_t cm_mutant(uint64_t v, uint32_t width, bool expand, bool be)
{
	const uint64_t mask = cm_mask(width);
	const uint64_t m = expand ? v | ~mask : v & mask;  // hints.go:168-176
	return be ? cm_swap(m, width) : m;                 // hints.go:186-191
}

// compMap[m] in the call's sorted pairs [a, b): the first pair with key >= m,
// and from there the number of pairs with key == m (a second search only
// where the key is present)
__device__ __forceinline__ uint32_t cm_values(const uint64_t* __restrict__ pairs, uint64_t a, uint64_t b, uint64_t m,
                                              uint64_t& first)
{
	first = su_search(a, b, [&](uint64_t i) { return pairs[2 * i] < m; });
	if (first >= b || pairs[2 * first] != m)
		return 0;
	const uint64_t past = su_search(first + 1, b, [&](uint64_t i) { return pairs[2 * i] <= m; });
	return (uint32_t)(past - first);
}

__device__ __forceinline__ bool cm_is_special(const uint64_t* __restrict__ sp, uint32_t nsp, uint64_t v)
{
	const uint32_t lo = su_search(0u, nsp, [&](uint32_t i) { return sp[i] < v; });
	return lo < nsp && sp[lo] == v;
}

// hints.go:193-207 for one value nv of compMap[mutant]: false = dropped, else
// rep = the replacer of v
__device__ __forceinline__ bool cm_replacer(uint64_t v, uint64_t nv, uint32_t width, bool be,
                                            const uint64_t* __restrict__ special, uint32_t nspecial, uint64_t& rep)
{
	const uint64_t mask = cm_mask(width), hi = nv & ~mask;
	nv &= mask;
	if (hi != 0 && (hi ^ ~mask) != 0)  // hints.go:194-198
		return false;
	if (be)
		nv = cm_swap(nv, width);  // hints.go:199-201
	if (cm_is_special(special, nspecial, nv))  // hints.go:202-204
		return false;
	rep = (v & ~mask) | nv;  // hints.go:207
	return true;
}

#endif  // __HIPCC__

}  // namespace syz
