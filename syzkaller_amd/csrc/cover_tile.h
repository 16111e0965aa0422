// cover_tile.h -- cover.hip's tile type for segsort.h over u32 keys: the 16-B
// loads, the quad sort and the quad-per-thread unique sweep described at the
// top of cover.hip, in a header so that report.hip sorts its per-call covers
// with the same routines.  Device code only: included from .hip files.
#pragma once

#include <algorithm>

#include "segsort.h"

namespace syz {

#ifndef SYZ_COVER_TILE
#define SYZ_COVER_TILE SYZSIG_COVER_TILE
#endif
constexpr uint32_t kCvTile = SYZ_COVER_TILE;
constexpr uint32_t kCvThreads = kSuThreads;
constexpr uint32_t kCvSweep = 4 * kCvThreads;   // keys per unique sweep: one quad per thread
constexpr uint32_t kCvAlign = 4;                // a long segment's key range: whole quads, 16-B aligned
constexpr uint32_t kCvMaxRuns = 8;
constexpr uint32_t kCvMaxSeg = 0x7fffffffu;     // keys per segment (an item's concatenated runs)
static_assert((kCvTile & (kCvTile - 1)) == 0 && kCvTile >= kCvSweep, "tile: a power of two, at least one sweep");
static_assert(kCvTile * 4 <= 64 * 1024, "a workgroup's LDS stays at or below 64 KB");

// survivors: u32 keys (SuSegs::src: u64 PCs, whose low words are the keys, or u32 keys)
using CvOut = SuOutKeys<SuU32>;

// k[0 .. n) = the keys [lo, lo + n) of segment `seg` (workgroup-wide).  A
// source's 16-B aligned body is read 16 B per lane, its ragged ends by a few lanes.
template <bool k64>
__device__ __forceinline__ void cv_load(const SuSegs& S, uint64_t seg, uint32_t lo, uint32_t n, uint32_t* k)
{
	const uint32_t tid = threadIdx.x;
	uint64_t o = 0;
	for (uint32_t r = 0; r < S.R; r++) {
		const uint32_t len = S.src_len[seg * S.R + r];
		const uint64_t a = std::max<uint64_t>(lo, o), b = std::min<uint64_t>((uint64_t)lo + n, o + len);
		if (a < b) {
			const uint64_t g = S.src_start[seg * S.R + r] + (a - o);
			uint32_t* d = k + (a - lo);
			const uint32_t cnt = (uint32_t)(b - a);
			if constexpr (k64) {
				const uint64_t* p = reinterpret_cast<const uint64_t*>(S.src) + g;
				const uint32_t h = (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 3) & 1);  // <= cnt
				const uint32_t np = (cnt - h) >> 1;
				const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p + h);
				for (uint32_t t = tid; t < np; t += kCvThreads) {
					const ulonglong2 v = q[t];
					d[h + 2 * t] = (uint32_t)v.x;
					d[h + 2 * t + 1] = (uint32_t)v.y;
				}
				if (tid == 0) {
					if (h)
						d[0] = (uint32_t)p[0];
					if ((cnt - h) & 1)
						d[cnt - 1] = (uint32_t)p[cnt - 1];
				}
			} else {
				const uint32_t* p = reinterpret_cast<const uint32_t*>(S.src) + g;
				const uint32_t h = std::min<uint32_t>((4 - (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3, cnt);
				const uint32_t nq = (cnt - h) >> 2;
				const uint4* q = reinterpret_cast<const uint4*>(p + h);
				for (uint32_t t = tid; t < nq; t += kCvThreads) {
					const uint4 v = q[t];
					d[h + 4 * t] = v.x;
					d[h + 4 * t + 1] = v.y;
					d[h + 4 * t + 2] = v.z;
					d[h + 4 * t + 3] = v.w;
				}
				if (tid < h)
					d[tid] = p[tid];
				const uint32_t tail = h + 4 * nq;
				if (tid >= 64 && tid - 64 < cnt - tail)
					d[tail + tid - 64] = p[tail + tid - 64];
			}
		}
		o += len;
	}
}

__device__ __forceinline__ void cv_cx(uint32_t& a, uint32_t& b, bool asc)
{
	const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
	a = asc ? lo : hi;
	b = asc ? hi : lo;
}

// strides 2 and 1 of a stage on one aligned quad
__device__ __forceinline__ void cv_quad(uint4& v, bool asc)
{
	cv_cx(v.x, v.z, asc);
	cv_cx(v.y, v.w, asc);
	cv_cx(v.x, v.y, asc);
	cv_cx(v.z, v.w, asc);
}

// Bitonic sort of k[0 .. N) ascending; N a power of two in [4, kCvTile], k
// 16-B aligned.  The caller's barrier follows the fill; ends with a barrier.
__device__ __forceinline__ void cv_sort(uint32_t* k, uint32_t N)
{
	uint4* k4 = reinterpret_cast<uint4*>(k);
	const uint32_t tid = threadIdx.x, NQ = N >> 2;
	for (uint32_t q = tid; q < NQ; q += kCvThreads) {  // stages 2 and 4
		uint4 v = k4[q];
		cv_cx(v.x, v.y, true);
		cv_cx(v.z, v.w, false);
		cv_quad(v, (q & 1) == 0);
		k4[q] = v;
	}
	for (uint32_t size = 8; size <= N; size <<= 1) {
		const uint32_t sq = size >> 2;  // the stage's block in quads
		for (uint32_t st = sq >> 1; st > 0; st >>= 1) {  // quad strides: key strides size/2 .. 4
			__syncthreads();
			for (uint32_t t = tid; t < NQ / 2; t += kCvThreads) {
				const uint32_t i = 2 * t - (t & (st - 1)), j = i + st;
				const bool asc = (i & sq) == 0;
				uint4 a = k4[i], b = k4[j];
				cv_cx(a.x, b.x, asc);
				cv_cx(a.y, b.y, asc);
				cv_cx(a.z, b.z, asc);
				cv_cx(a.w, b.w, asc);
				k4[i] = a;
				k4[j] = b;
			}
		}
		__syncthreads();
		for (uint32_t q = tid; q < NQ; q += kCvThreads) {
			uint4 v = k4[q];
			cv_quad(v, (q & sq) == 0);
			k4[q] = v;
		}
	}
	__syncthreads();
}

// The survivors of the sorted keys 0 .. n) -- key i survives iff i == 0 or it
// differs from key i - 1 -- written densely to out; returns their count
// (workgroup-wide, uniform).  quad(i0) = keys i0 .. i0 + 3 (i0 a multiple of
// 4; keys at n and past it are ignored), prev(i0) = key i0 - 1.
template <typename Quad, typename Prev>
__device__ __forceinline__ uint32_t cv_unique_write(uint32_t n, uint32_t* out, Quad quad, Prev prev)
{
	__shared__ uint32_t s_w[2][kCvThreads / 64];
	const uint32_t tid = threadIdx.x, w = tid >> 6;
	uint32_t run = 0, it = 0;
	for (uint32_t base = 0; base < n; base += kCvSweep, it ^= 1) {
		const uint32_t i0 = base + 4 * tid;
		uint4 v = make_uint4(0, 0, 0, 0);
		uint32_t pv = 0;
		if (i0 < n) {
			v = quad(i0);
			pv = i0 ? prev(i0) : 0;
		}
		const bool f0 = i0 < n && (i0 == 0 || v.x != pv), f1 = i0 + 1 < n && v.y != v.x,
		           f2 = i0 + 2 < n && v.z != v.y, f3 = i0 + 3 < n && v.w != v.z;
		const uint32_t c = (uint32_t)f0 + f1 + f2 + f3;
		const uint32_t incl = wave_incl_scan(c);
		if (lane_id() == 63)
			s_w[it][w] = incl;
		__syncthreads();  // (s_w[it] is rewritten two sweeps on, past the next sweep's barrier)
		uint32_t wb = 0, tot = 0;
#pragma unroll
		for (uint32_t x = 0; x < kCvThreads / 64; x++) {
			wb += x < w ? s_w[it][x] : 0;
			tot += s_w[it][x];
		}
		uint32_t pos = run + wb + incl - c;
		if (f0)
			out[pos++] = v.x;
		if (f1)
			out[pos++] = v.y;
		if (f2)
			out[pos++] = v.z;
		if (f3)
			out[pos++] = v.w;
		run += tot;
	}
	return run;
}

// segsort.h's tile type over the routines above (k64: the source holds u64 PCs)
template <bool k64>
struct CvTile {
	using Key = SuU32;
	static constexpr uint32_t kTile = kCvTile, kAlign = kCvAlign, kMinPad = 4;
	struct Lds {
		__align__(16) uint32_t k[kCvTile];
	};
	static __device__ __forceinline__ void load(const SuSegs& S, uint64_t seg, uint32_t lo, uint32_t n, Lds& t)
	{
		cv_load<k64>(S, seg, lo, n, t.k);
	}
	static __device__ __forceinline__ void sort(Lds& t, uint32_t n, uint32_t N)
	{
		for (uint32_t i = n + threadIdx.x; i < N; i += kCvThreads)
			t.k[i] = SuU32::pad();  // (>= every key: the first n sorted keys are the segment's)
		__syncthreads();
		cv_sort(t.k, N);
	}
	// o 16-B aligned: a key range and a tile's offset in it are multiples of 4 keys
	static __device__ __forceinline__ void store(const Lds& t, uint32_t n, uint32_t* o)
	{
		const uint32_t tid = threadIdx.x;
		for (uint32_t q = tid; q < n >> 2; q += kCvThreads)
			reinterpret_cast<uint4*>(o)[q] = reinterpret_cast<const uint4*>(t.k)[q];
		if (tid < (n & 3))
			o[(n & ~3u) + tid] = t.k[(n & ~3u) + tid];
	}
	// s 16-B aligned and readable in whole quads: a key range of the sort buffers, or the LDS tile
	static __device__ __forceinline__ uint64_t unique_buf(uint32_t n, uint64_t seg, const CvOut& pol, const uint32_t* s)
	{
		return cv_unique_write(
			n, pol.dst(seg), [&](uint32_t i0) { return reinterpret_cast<const uint4*>(s)[i0 >> 2]; },
			[&](uint32_t i0) { return s[i0 - 1]; });
	}
	static __device__ __forceinline__ uint64_t unique_lds(uint32_t n, uint64_t seg, const CvOut& pol, const Lds& t)
	{
		return unique_buf(n, seg, pol, t.k);
	}
};

// Full u64 PCs as keys (cover.hip, the unchecked u64 target: order and equality
// are the u64's, only the survivors are truncated): segsort.h's plain tile of
// one word, with the tile size and key-range alignment of the u32 tile, so that
// k_cover_prep_calls' counts serve both (8 kCvTile bytes of LDS, 32 KB at 4096).
struct CvTile64 : SuWordsTile<1, kCvTile> {
	static constexpr uint32_t kAlign = kCvAlign;
};
static_assert(kCvTile * 8 <= 64 * 1024, "a workgroup's LDS stays at or below 64 KB");

// output policy of CvTile64: executor.h:525-526, each surviving PC's low word
// (CvOut's fields and places)
struct CvOutLow {
	uint32_t* out;
	const uint64_t* out_pos;
	uint64_t pos_stride;
	uint32_t* out_cnt;
	__device__ __forceinline__ uint32_t* dst(uint64_t seg) const { return out + out_pos[seg * pos_stride]; }
	__device__ __forceinline__ uint64_t weight(uint64_t, const SuWords<1>&) const { return 1; }
	__device__ __forceinline__ void put(uint64_t seg, uint64_t pos, const SuWords<1>& k, uint64_t) const
	{
		dst(seg)[pos] = (uint32_t)k.w[0];
	}
	__device__ __forceinline__ void finish(uint64_t seg, uint64_t total) const { out_cnt[seg] = (uint32_t)total; }
};

}  // namespace syz
