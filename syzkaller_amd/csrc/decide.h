// decide.h -- checkNewSignal's decision for one distinct element e from its
// level firsts f4 (the smallest serial among e's records at each level), in the
// pieces that the finalize kernels and k_stair_bucket of agg.hip and the records
// path of recs.hip compose; they differ only in how they reach e's table slots.
#pragma once

#include "internal.h"

namespace syz {

constexpr uint32_t kNoFirst = 0xFFFFFFFFu;  // a level first: no record at this level

// What a finalize kernel counts, and its epilogue.
struct FinCounts {
	uint64_t inserted = 0, changed = 0, ns_ins = 0, ovf = 0;
	// every thread of the block (kOvf = false: the kernel cannot overflow a table)
	template <bool kOvf = true>
	__device__ __forceinline__ void report(unsigned long long* ctr) const
	{
		block_count(&ctr[kCntInserted], inserted);
		block_count(&ctr[kCntChanged], changed);
		block_count(&ctr[kCntAux], ns_ins);
		if (kOvf)
			block_count(&ctr[kCntOverflow], ovf);
	}
};

// the top level present among the run's lm.n, or -1 (none, or !valid)
__device__ __forceinline__ int fin_top(uint4 f4, const LevelMap& lm, bool valid)
{
	const uint32_t f[4] = {f4.x, f4.y, f4.z, f4.w};
	int top = -1;
#pragma unroll
	for (int l = 0; l < 4; l++)
		if (valid && l < (int)lm.n && f[l] != kNoFirst)
			top = l;
	return top;
}

// p0 = M0[e] from the word `old` of e's maxSignal slot (0: inserted or claimed
// just now; an "absent" marker is not live).  True when P raises it, counted.
__device__ __forceinline__ bool fin_raises(uint64_t old, int8_t P, FinCounts& n, int& p0)
{
	const bool present = slot_live(old);
	p0 = present ? (int)slot_prio(old) : kPrioAbsent;
	if ((int)P <= p0)
		return false;
	n.inserted += !present;  // fresh, or an "absent" marker going live
	n.changed++;
	return true;
}

// The staircase of an element's level firsts: from level `top` down, the
// first records of strictly rising level -- each earlier than every record of
// a higher level -- as on(level, first).  cut(level) ends the walk there.
template <typename Cut, typename On>
__device__ __forceinline__ void stair_walk(uint4 f4, int top, Cut cut, On on)
{
	const uint32_t f[4] = {f4.x, f4.y, f4.z, f4.w};
	uint32_t mk = kNoFirst;
#pragma unroll
	for (int l = 3; l >= 0; l--) {
		if (l > top || f[l] == kNoFirst)
			continue;
		if (cut(l))
			break;
		if (f[l] < mk) {
			mk = f[l];
			on(l, f[l]);
		}
	}
}

// whether the record (level, serial) is on the whole staircase (stair_walk
// without a cut: a level whose first equals a higher level's is not on it)
__device__ __forceinline__ bool stair_has(uint4 f4, uint32_t level, uint32_t serial)
{
	bool has = false;
	stair_walk(f4, 3, [](int) { return false; },
	           [&](int l, uint32_t first) { has |= (uint32_t)l == level && first == serial; });
	return has;
}

// the levels of an element's whole staircase (stair_walk without a cut), as a mask
__device__ __forceinline__ uint32_t stair_levels(uint4 f4, uint32_t nlev)
{
	uint32_t m = 0;
	stair_walk(f4, (int)nlev - 1, [](int) { return false; }, [&](int l, uint32_t) { m |= 1u << l; });
	return m;
}

}  // namespace syz
