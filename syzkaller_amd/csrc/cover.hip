// cover.hip -- the executor's cover output and triageInput's inputCover, on
// device: a segmented sort-unique of u32 keys.
//
// References:
//   executor/executor.h:514-527   write_coverage_signal's second half: with
//       flag_collect_cover the call's PCs go out as u32, after std::sort +
//       std::unique over the u64 PCs with flag_dedup_cover
//       (syzsig_edge_cover_dev);
//   syz-fuzzer/proc.go:139, :173  inputCover.Merge(inf.Cover) over the re-runs
//       and Cover: inputCover.Serialize() (syzsig_triage_cover_dev).
// Both are the same operation per segment (a call's trace; the concatenated
// cover lists of an item's merged runs): sort ascending, drop equal
// neighbours, write the survivors densely and their count.
//
// Exactness of sorting the low words.  Every PC of a completed call passed
// cover_check (executor_linux.cc:196-204), so it lies in [0xffffffff80000000,
// 0xffffffffff000000): its upper word is 0xffffffff.  u64 order and equality
// of such PCs are those of their low words, so sort + unique on the low words,
// which is what leaves here, is the reference's sort + unique on u64 followed
// by the truncation of executor.h:519-526.  A call that did not complete
// (the one holding the PC that failed cover_check, and every later call of its
// program) never reaches this: its segment length is forced to 0 from
// `completed` before any key is read (k_cover_prep_calls), as doexit(0)
// happens inside the signal loop before any cover is written.
//
// The segmented sort-unique is segsort.h's, over u32 keys with this file's
// own tile routines (T = kCvTile keys, SYZSIG_COVER_TILE; 4 T bytes of LDS, 16
// KB at T = 4096: several workgroups share a CU): 16-B global loads on a
// source's aligned body (cv_load), the quad sort below (cv_sort), a quad per
// thread in the unique sweep (cv_unique_write), and key ranges of whole quads
// in the sort buffers, so that the tile stores and the sweep's loads are 16 B.
//   k_cover_prep_calls / _items   validate; per segment its length (and per
//                                 run of an item its merged length); count the
//                                 segments longer than T, their tiles and keys
//
// The LDS sort.  The compare-exchanges of strides 2 and 1 of every stage run
// in registers on the thread's own 16-B quad (no barrier between them, and
// the stages of size 2 and 4 need no LDS step at all); the strides >= 4 pair
// two aligned quads, read and written as 16-B LDS accesses.  At quad strides
// 1..8 the ds_read_b128 lane groups see a 2-way bank conflict (two rows of
// 256 B per 16 lanes), larger strides are conflict-free; the 16-B stores are
// bound by their register transfer, not by the array.
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

// executor.h:514-527 per call: seg_len[c] = call_len[c] for a call with a
// cover record (c - prog_call[p] < completed[p]), else 0.  Validates every
// call of every program as syzsig_edge_derive_dev does.
__global__ __launch_bounds__(64) void k_cover_prep_calls(const uint64_t* __restrict__ call_start,
                                                         const uint32_t* __restrict__ call_len, uint64_t ncalls,
                                                         uint64_t npc, const uint32_t* __restrict__ prog_call,
                                                         uint64_t nprog, const uint32_t* __restrict__ completed,
                                                         uint32_t* seg_len, unsigned long long* cnt)
{
	uint64_t err = 0, nl = 0, nt = 0, nk = 0;
	for (uint64_t p = blockIdx.x; p < nprog; p += gridDim.x) {
		const uint64_t cb = prog_call[p], ce = prog_call[p + 1];
		if (cb > ce || ce > ncalls || completed[p] > ce - cb) {
			err += threadIdx.x == 0;
			continue;
		}
		const uint64_t done = completed[p];
		for (uint64_t c = cb + threadIdx.x; c < ce; c += blockDim.x) {
			const uint64_t start = call_start[c];
			const uint32_t len = call_len[c];
			if (len >= kCoverSize || start > npc || len > npc - start) {
				err++;  // executor_linux.cc:186-187 fail("too much cover") / malformed input
				continue;
			}
			const uint32_t eff = c - cb < done ? len : 0;
			seg_len[c] = eff;
			su_count_large<kCvTile, kCvAlign>(eff, nl, nt, nk, cnt);
		}
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
}

// proc.go:119-139 per item: run r of a kept item is merged (:139) unless the
// loop skipped it (:122-123: not executed, no signal, or failed after a
// successful original); a dropped item took a `return` before :173.
__global__ __launch_bounds__(256) void k_cover_prep_items(
	uint64_t nitems, uint32_t R, const uint8_t* __restrict__ item_flags, const uint8_t* __restrict__ item_keep,
	const uint64_t* __restrict__ run_off, const int32_t* __restrict__ run_errno, const uint8_t* __restrict__ run_exec,
	uint64_t ncover, const uint64_t* __restrict__ run_cover_start, const uint32_t* __restrict__ run_cover_len,
	uint32_t* src_len, uint32_t* seg_len, unsigned long long* cnt)
{
	uint64_t err = 0, ovf = 0, nl = 0, nt = 0, nk = 0, tot = 0;
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < nitems) {
		const bool keep = item_keep[i] != 0, orig_ok = item_flags[i] & SYZSIG_TRIAGE_ORIG_OK;
		uint64_t total = 0;
		for (uint32_t r = 0; r < R; r++) {
			const uint64_t rr = i * R + r, s = run_cover_start[rr];
			const uint32_t l = run_cover_len[rr];
			if (s > ncover || l > ncover - s) {
				err++;
				src_len[rr] = 0;
				continue;
			}
			const bool merged = keep && run_exec[rr] && run_off[rr + 1] > run_off[rr] && !(orig_ok && run_errno[rr] != 0);
			src_len[rr] = merged ? l : 0;
			total += merged ? l : 0;
		}
		if (total > kCvMaxSeg) {
			ovf++;
			total = 0;
		}
		seg_len[i] = (uint32_t)total;
		tot = total;
		su_count_large<kCvTile, kCvAlign>((uint32_t)total, nl, nt, nk, cnt);
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kCntOverflow], ovf);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
	block_count(&cnt[kSuTotal], tot);
}

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

// executor.h:525-527 without flag_dedup_cover: the PCs truncated, in trace order
__global__ __launch_bounds__(kCvThreads) void k_cover_trunc(const uint64_t* __restrict__ pcs, SuSegs S, CvOut pol)
{
	for (uint64_t seg = blockIdx.x; seg < S.nseg; seg += gridDim.x) {
		const uint32_t n = S.seg_len[seg];
		const uint64_t g = S.src_start[seg];
		uint32_t* o = pol.dst(seg);
		for (uint32_t i = threadIdx.x; i < n; i += kCvThreads)
			o[i] = (uint32_t)pcs[g + i];
		if (threadIdx.x == 0)
			pol.finish(seg, n);
	}
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_edge_cover_dev(syzsig_ctx* ctx, const uint64_t* d_pcs, uint64_t npc,
                                     const uint64_t* d_call_start, const uint32_t* d_call_len, uint64_t ncalls,
                                     const uint32_t* d_prog_call, uint64_t nprog, const uint32_t* d_completed,
                                     uint32_t flags, uint32_t* d_cover, uint32_t* d_cover_cnt)
{
	SYZ_LOCK(ctx);
	if (!ctx || (nprog && (!d_prog_call || !d_completed)) || (ncalls && (!d_call_start || !d_call_len || !d_cover_cnt)) ||
	    (npc && (!d_pcs || !d_cover)))
		return fail(SYZSIG_EINVAL, "edge_cover: NULL argument");
	if (flags & ~(uint32_t)SYZSIG_COVER_DEDUP)
		return fail(SYZSIG_EINVAL, "edge_cover: unknown flag");
	if (ncalls == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	void* seg_len;
	SYZ_TRY(ws_get(ctx, kWsSuMeta, ncalls * 4 + 256, &seg_len));
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	// a call outside every program has no record
	SYZ_HIP(hipMemsetAsync(seg_len, 0, ncalls * 4, s));
	if (nprog)
		k_cover_prep_calls<<<grid_cap(nprog), 64, 0, s>>>(d_call_start, d_call_len, ncalls, npc, d_prog_call, nprog,
		                                                  d_completed, (uint32_t*)seg_len, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "edge_cover: malformed program/call ranges, completed past a program's calls, or "
		                           "a call with >= 262144 PCs");
	const SuSegs S{d_pcs, 1, d_call_start, (const uint32_t*)seg_len, 1, (const uint32_t*)seg_len, ncalls};
	const CvOut pol{d_cover, d_call_start, 1, d_cover_cnt};
	if (flags & SYZSIG_COVER_DEDUP) {
		SYZ_TRY((su_sort_unique<CvTile<true>, CvOut>(ctx, S, pol)));
	} else {
		k_cover_trunc<<<grid_cap(ncalls), kCvThreads, 0, s>>>(d_pcs, S, pol);
		SYZ_HIP(hipGetLastError());
	}
	SYZ_TRY(su_time_end(ctx));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "edge_cover: internal: a long segment did not fit its workspace");
	return SYZSIG_OK;
}

extern "C" int syzsig_triage_cover_dev(syzsig_ctx* ctx, uint64_t nitems, uint32_t runs, const uint8_t* d_item_flags,
                                       const uint8_t* d_item_keep, const uint64_t* d_run_off,
                                       const int32_t* d_run_errno, const uint8_t* d_run_exec,
                                       const uint32_t* d_cover, uint64_t ncover, const uint64_t* d_run_cover_start,
                                       const uint32_t* d_run_cover_len, uint64_t* d_item_cover_off,
                                       uint32_t* d_item_cover, uint64_t cap, uint64_t* n_out)
{
	SYZ_LOCK(ctx);
	if (n_out)
		*n_out = 0;
	if (!ctx || !d_item_cover_off || !n_out || (nitems && (!d_item_flags || !d_item_keep)) ||
	    (nitems && runs && (!d_run_off || !d_run_errno || !d_run_exec || !d_run_cover_start || !d_run_cover_len)) ||
	    (ncover && !d_cover) || (cap && !d_item_cover))
		return fail(SYZSIG_EINVAL, "triage_cover: NULL argument");
	if (runs > kCvMaxRuns)
		return fail(SYZSIG_ERANGE, "triage_cover: at most 8 runs per item");
	const hipStream_t s = ctx->stream;
	if (nitems == 0 || runs == 0) {
		SYZ_HIP(hipMemsetAsync(d_item_cover_off, 0, (nitems + 1) * 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	const uint64_t nruns = nitems * runs;
	// src_len[nruns], seg_len[nitems], cnt[nitems], stage_off[nitems + 1], off[nitems + 1]
	char* d;
	const size_t o_seg = align256(nruns * 4), o_cnt = o_seg + align256(nitems * 4), o_soff = o_cnt + align256(nitems * 4),
	             o_off = o_soff + align256((nitems + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsSuMeta, o_off + align256((nitems + 1) * 8), (void**)&d));
	uint32_t *src_len = (uint32_t*)d, *seg_len = (uint32_t*)(d + o_seg), *cnt = (uint32_t*)(d + o_cnt);
	uint64_t *stage_off = (uint64_t*)(d + o_soff), *off = (uint64_t*)(d + o_off);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_cover_prep_items<<<(int)((nitems + 255) / 256), 256, 0, s>>>(nitems, runs, d_item_flags, d_item_keep, d_run_off,
	                                                               d_run_errno, d_run_exec, ncover, d_run_cover_start,
	                                                               d_run_cover_len, src_len, seg_len, ctx->d_cnt);
	k_su_scan<<<1, kCvThreads, 0, s>>>(seg_len, nitems, stage_off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "triage_cover: a run's cover range lies outside the cover buffer");
	if (ctx->h_cnt[kCntOverflow])
		return fail(SYZSIG_ERANGE, "triage_cover: an item's runs hold 2^31 or more PCs");
	void* stage;
	SYZ_TRY(ws_get(ctx, kWsSuStage, ctx->h_cnt[kSuTotal] * 4 + 256, &stage));
	const SuSegs S{d_cover, 1, d_run_cover_start, src_len, runs, seg_len, nitems};
	const CvOut pol{(uint32_t*)stage, stage_off, 1, cnt};
	SYZ_TRY((su_sort_unique<CvTile<false>, CvOut>(ctx, S, pol)));
	k_su_scan<<<1, kCvThreads, 0, s>>>(cnt, nitems, off);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, off + nitems, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "triage_cover: internal: a long segment did not fit its workspace");
	*n_out = total;
	if (total > cap)
		return fail(SYZSIG_ERANGE, "triage_cover: the items' cover needs more than the given capacity");
	k_su_gather<<<grid_cap(nitems), kCvThreads, 0, s>>>((const uint32_t*)stage, stage_off, 1, 1, off, nitems, d_item_cover,
	                                                    d_item_cover_off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}
