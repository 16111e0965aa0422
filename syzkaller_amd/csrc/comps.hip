// comps.hip -- comparison hints on device: the executor's comps output, the
// fuzzer's CompMap and prog.shrinkExpand.
//
// References:
//   executor/executor.h:576-593   handle_completion with flag_collect_comps:
//       std::sort + std::unique over the call's kcov_comparison_t records
//       (operator< / operator== :861-875, on type, arg1, arg2; pc takes no
//       part), ignore() (executor_linux.cc:221-253) and write() (:823-859)
//       (syzsig_exec_comps_dev);
//   pkg/ipc/ipc.go:420-465        the records parsed back into prog.CompMap
//       through CompMap.AddComp (prog/hints.go:43-48) (syzsig_comp_map_dev);
//   prog/hints.go:164-218         shrinkExpand (syzsig_shrink_expand_dev).
// All three reduce to one operation per segment -- sort ascending, drop equal
// neighbours, write the survivors -- over keys of 3, 2 and 1 u64 words: the
// comparison triple; the (key, value) pair of the map; a replacer.
//
// The segmented sort-unique is cover.hip's, templated on the key width W
// (T = kCmTile keys, SYZSIG_COMPS_TILE):
//   k_cm_small        one workgroup per segment of <= T keys: the keys into LDS
//                     as W arrays of T words (a lane's compare reads one word
//                     per array: consecutive lanes, consecutive 8-B words),
//                     padded to a power of two with all-ones keys, bitonic
//                     sort, then neighbour flags, block scan, compacted write.
//                     8 W T bytes of LDS: 48 KB at W = 3.
//   segments longer than T (a call has up to 65535 records, 131070 pairs) go
//   through workspace buffers in HBM:
//   k_cm_register     each gets a slot, a key range and its tiles (three
//                     atomics per SEGMENT; none per key anywhere)
//   k_cm_tile_sort    one workgroup per tile of T keys: sorted in LDS
//   k_cm_merge        ceil(log2(tiles of the longest segment)) passes, known at
//                     launch: runs of w keys merged pairwise by rank (left run:
//                     lower bound in the right one; right run: upper bound in
//                     the left one -- a bijection, duplicates included)
//   k_cm_unique_large one workgroup per segment streams its sorted keys
// What a survivor turns into is the output policy's business: CmOutKeys writes
// the key itself; CmOutComps applies ignore() and write(), so a survivor
// weighs 0, 3 or 5 output words, and the block scan runs over (count << 32 |
// words).  Every loop is bounded by a segment length, a run count, a pass
// count or the 64 steps of a binary search; nothing waits for another wave.
#include <algorithm>
#include <vector>

#include "internal.h"

namespace syz {

#ifndef SYZ_COMPS_TILE
#define SYZ_COMPS_TILE SYZSIG_COMPS_TILE
#endif
constexpr uint32_t kCmTile = SYZ_COMPS_TILE;
constexpr uint32_t kCmThreads = 256;
constexpr uint32_t kCmMaxComps = 65535;       // executor.h:581-582: 8 + 32 n bytes fit kCoverSize * 8
constexpr uint32_t kCmMaxSeg = 0x7fffffffu;   // keys per segment
constexpr uint32_t kCmVariants = 12;          // hints.go:165-191: 7 widths little-endian, 5 big-endian (not at width 1)
constexpr uint32_t kCmMaxSpecial = 4096;
constexpr uint64_t kCmMaxOutput = 16ull << 20;  // executor.h kMaxOutput
constexpr uint32_t kCmpConst = 1, kCmpSizeMask = 6, kCmpSize1 = 0, kCmpSize2 = 2, kCmpSize8 = 6;  // executor.h:147-152
static_assert((kCmTile & (kCmTile - 1)) == 0 && kCmTile >= kCmThreads, "tile: a power of two, at least one sweep");
static_assert(kCmTile * 3 * 8 <= 64 * 1024, "the widest key's tile stays at or below 64 KB of LDS");

// the context's counters as this file uses them (zeroed per call)
constexpr int kCmLarge = kCntAux, kCmTiles = kCntAux2, kCmKeys = kCntCandidates, kCmMaxLen = kCntTouched,
              kCmCurLarge = kCntDefer, kCmCurTiles = kCntDeferNs, kCmCurKeys = kCntDistinct;

template <int W>
struct CmKey {
	uint64_t w[W];
};

template <int W>
__device__ __forceinline__ bool cm_lt(const CmKey<W>& a, const CmKey<W>& b)
{
#pragma unroll
	for (int i = 0; i < W - 1; i++)
		if (a.w[i] != b.w[i])
			return a.w[i] < b.w[i];
	return a.w[W - 1] < b.w[W - 1];
}

template <int W>
__device__ __forceinline__ bool cm_eq(const CmKey<W>& a, const CmKey<W>& b)
{
	bool e = true;
#pragma unroll
	for (int i = 0; i < W; i++)
		e = e && a.w[i] == b.w[i];
	return e;
}

// Segment s is the concatenation of its R sources: the keys at src[(src_start[s
// * R + r] + i) * stride .. + W), i < src_len[s * R + r]; seg_len[s] in all.
struct CmSegs {
	const uint64_t* src;
	uint32_t stride;  // words from one key to the next (>= W)
	const uint64_t* src_start;
	const uint32_t* src_len;
	uint32_t R;
	const uint32_t* seg_len;
	uint64_t nseg;
};

// output policy: the surviving keys themselves, segment s's at out[out_pos[s * pos_stride] * W ..]
template <int W>
struct CmOutKeys {
	uint64_t* out;
	const uint64_t* out_pos;  // in keys; segment s's is out_pos[s * pos_stride]
	uint64_t pos_stride;
	uint32_t* out_cnt;
	__device__ __forceinline__ uint64_t weight(const CmKey<W>&) const { return 1; }
	__device__ __forceinline__ void put(uint64_t seg, uint64_t pos, const CmKey<W>& k) const
	{
		uint64_t* o = out + (out_pos[seg * pos_stride] + pos) * W;
#pragma unroll
		for (int i = 0; i < W; i++)
			o[i] = k.w[i];
	}
	__device__ __forceinline__ void finish(uint64_t seg, uint64_t total) const { out_cnt[seg] = (uint32_t)total; }
};

// output policy: executor.h:586-591 over the unique records -- ignore(), then write()
struct CmOutComps {
	uint32_t* out;
	const uint64_t* call_start;  // in records: call c's words at out[5 * call_start[c] ..]
	uint32_t* out_words;
	uint32_t* comps_cnt;
	uint64_t out_start;
	// executor_linux.cc:221-253 (x86_64)
	__device__ __forceinline__ bool ignore(uint64_t type, uint64_t a1, uint64_t a2) const
	{
		if (a1 == 0 && (a2 == 0 || (type & kCmpConst)))
			return true;
		if ((type & kCmpSizeMask) == kCmpSize8) {
			const uint64_t out_end = out_start + kCmMaxOutput;
			if (a1 >= out_start && a1 <= out_end)
				return true;
			if (a2 >= out_start && a2 <= out_end)
				return true;
			const uint64_t kmem_start = 0xffff880000000000ull, kmem_end = 0xffff890000000000ull;
			const bool kptr1 = a1 >= kmem_start && a1 <= kmem_end, kptr2 = a2 >= kmem_start && a2 <= kmem_end;
			if (kptr1 && kptr2)
				return true;
			if (kptr1 && a2 == 0)
				return true;
			if (kptr2 && a1 == 0)
				return true;
		}
		return false;
	}
	// survivors << 32 | words
	__device__ __forceinline__ uint64_t weight(const CmKey<3>& k) const
	{
		if (ignore(k.w[0], k.w[1], k.w[2]))
			return 0;
		return (1ull << 32) | ((k.w[0] & kCmpSizeMask) == kCmpSize8 ? 5u : 3u);
	}
	// executor.h:823-859.  The low 32 bits of a sign extension from 1, 2 or 4
	// bytes are what leaves for those sizes.
	__device__ __forceinline__ void put(uint64_t seg, uint64_t pos, const CmKey<3>& k) const
	{
		uint32_t* o = out + 5 * call_start[seg] + (uint32_t)pos;
		const uint32_t sz = (uint32_t)k.w[0] & kCmpSizeMask;
		uint64_t a1 = k.w[1], a2 = k.w[2];
		o[0] = (uint32_t)k.w[0];
		if (sz == kCmpSize8) {
			o[1] = (uint32_t)a1;
			o[2] = (uint32_t)(a1 >> 32);
			o[3] = (uint32_t)a2;
			o[4] = (uint32_t)(a2 >> 32);
			return;
		}
		if (sz == kCmpSize1) {
			a1 = (uint64_t)(int64_t)(int8_t)a1;
			a2 = (uint64_t)(int64_t)(int8_t)a2;
		} else if (sz == kCmpSize2) {
			a1 = (uint64_t)(int64_t)(int16_t)a1;
			a2 = (uint64_t)(int64_t)(int16_t)a2;
		} else {
			a1 = (uint64_t)(int64_t)(int32_t)a1;
			a2 = (uint64_t)(int64_t)(int32_t)a2;
		}
		o[1] = (uint32_t)a1;
		o[2] = (uint32_t)a2;
	}
	__device__ __forceinline__ void finish(uint64_t seg, uint64_t total) const
	{
		out_words[seg] = (uint32_t)total;
		comps_cnt[seg] = (uint32_t)(total >> 32);
	}
};

// the segments longer than a tile, their key ranges in the sort buffers and
// the tiles of all of them
struct CmLarge {
	const uint64_t* lg_seg;
	const uint64_t* lg_base;  // in keys
	const uint32_t* tile_lg;
	const uint32_t* tile_idx;
};

__device__ __forceinline__ void cm_count_large(uint32_t len, uint64_t& nl, uint64_t& nt, uint64_t& nk,
                                               unsigned long long* cnt)
{
	if (len > kCmTile) {
		nl++;
		nt += (len + kCmTile - 1) / kCmTile;
		nk += len;
		atomicMax(&cnt[kCmMaxLen], (unsigned long long)len);
	}
}

// executor.h:578-582 per call: its records lie inside the buffer and are at
// most 65535 (fail("too many comparisons")).  seg_len[c] = call_len[c].
__global__ __launch_bounds__(256) void k_cm_prep_calls(const uint64_t* __restrict__ call_start,
                                                       const uint32_t* __restrict__ call_len, uint64_t ncalls,
                                                       uint64_t ncmp, uint32_t* seg_len, unsigned long long* cnt)
{
	uint64_t err = 0, nl = 0, nt = 0, nk = 0;
	const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (c < ncalls) {
		const uint64_t start = call_start[c];
		const uint32_t len = call_len[c];
		if (len > kCmMaxComps || start > ncmp || len > ncmp - start) {
			err++;
			seg_len[c] = 0;
		} else {
			seg_len[c] = len;
			cm_count_large(len, nl, nt, nk, cnt);
		}
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kCmLarge], nl);
	block_count(&cnt[kCmTiles], nt);
	block_count(&cnt[kCmKeys], nk);
}

// seg_len[s] = the sum of its R source lengths (as a kernel left them)
__global__ __launch_bounds__(256) void k_cm_prep_sources(const uint32_t* __restrict__ src_len, uint32_t R,
                                                         uint64_t nseg, uint32_t* seg_len, unsigned long long* cnt)
{
	uint64_t ovf = 0, nl = 0, nt = 0, nk = 0;
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s < nseg) {
		uint64_t total = 0;
		for (uint32_t r = 0; r < R; r++)
			total += src_len[s * R + r];
		if (total > kCmMaxSeg) {
			ovf++;
			total = 0;
		}
		seg_len[s] = (uint32_t)total;
		cm_count_large((uint32_t)total, nl, nt, nk, cnt);
	}
	block_count(&cnt[kCntOverflow], ovf);
	block_count(&cnt[kCmLarge], nl);
	block_count(&cnt[kCmTiles], nt);
	block_count(&cnt[kCmKeys], nk);
}

__device__ __forceinline__ uint64_t cm_wave_incl_scan(uint64_t v)
{
	const uint32_t lane = lane_id();
#pragma unroll
	for (uint32_t o = 1; o < 64; o <<= 1) {
		const uint64_t x = __shfl_up(v, o, 64);
		if (lane >= o)
			v += x;
	}
	return v;
}

// off[0..n] = the exclusive prefix sums of v[0..n) (one workgroup)
__global__ __launch_bounds__(kCmThreads) void k_cm_scan(const uint32_t* __restrict__ v, uint64_t n, uint64_t* off)
{
	__shared__ uint64_t s_w[kCmThreads / 64];
	const uint32_t w = threadIdx.x >> 6;
	uint64_t run = 0;
	for (uint64_t base = 0; base < n; base += kCmThreads) {
		const uint64_t i = base + threadIdx.x;
		const uint64_t x = i < n ? v[i] : 0;
		const uint64_t incl = cm_wave_incl_scan(x);
		if (lane_id() == 63)
			s_w[w] = incl;
		__syncthreads();
		uint64_t wb = 0, tot = 0;
#pragma unroll
		for (uint32_t k = 0; k < kCmThreads / 64; k++) {
			wb += k < w ? s_w[k] : 0;
			tot += s_w[k];
		}
		if (i < n)
			off[i] = run + wb + incl - x;
		run += tot;
		__syncthreads();
	}
	if (threadIdx.x == 0)
		off[n] = run;
}

// the tile in LDS: W arrays of kCmTile words
template <int W>
struct CmTileLds {
	uint64_t k[W][kCmTile];
	__device__ __forceinline__ CmKey<W> get(uint32_t i) const
	{
		CmKey<W> x;
#pragma unroll
		for (int w = 0; w < W; w++)
			x.w[w] = k[w][i];
		return x;
	}
	__device__ __forceinline__ void set(uint32_t i, const CmKey<W>& x)
	{
#pragma unroll
		for (int w = 0; w < W; w++)
			k[w][i] = x.w[w];
	}
};

// t[0 .. n) = the keys [lo, lo + n) of segment `seg` (workgroup-wide)
template <int W>
__device__ __forceinline__ void cm_load(const CmSegs& S, uint64_t seg, uint32_t lo, uint32_t n, CmTileLds<W>& t)
{
	uint64_t o = 0;
	for (uint32_t r = 0; r < S.R; r++) {
		const uint32_t len = S.src_len[seg * S.R + r];
		const uint64_t a = std::max<uint64_t>(lo, o), b = std::min<uint64_t>((uint64_t)lo + n, o + len);
		if (a < b) {
			const uint64_t* p = S.src + (S.src_start[seg * S.R + r] + (a - o)) * S.stride;
			const uint32_t d = (uint32_t)(a - lo), cnt = (uint32_t)(b - a);
			for (uint32_t i = threadIdx.x; i < cnt; i += kCmThreads) {
#pragma unroll
				for (int w = 0; w < W; w++)
					t.k[w][d + i] = p[(uint64_t)i * S.stride + w];
			}
		}
		o += len;
	}
}

// Bitonic sort of t[0 .. N) ascending; N a power of two <= kCmTile.  Starts and
// ends with a barrier.
template <int W>
__device__ __forceinline__ void cm_sort(CmTileLds<W>& t, uint32_t N)
{
	for (uint32_t size = 2; size <= N; size <<= 1) {
		for (uint32_t st = size >> 1; st > 0; st >>= 1) {
			__syncthreads();
			for (uint32_t x = threadIdx.x; x < N / 2; x += kCmThreads) {
				const uint32_t i = 2 * x - (x & (st - 1)), j = i + st;
				const bool asc = (i & size) == 0;
				const CmKey<W> a = t.get(i), b = t.get(j);
				if (asc ? cm_lt(b, a) : cm_lt(a, b)) {
					t.set(i, b);
					t.set(j, a);
				}
			}
		}
	}
	__syncthreads();
}

// The survivors of the sorted keys 0 .. n) -- key i survives iff i == 0 or it
// differs from key i - 1 -- handed to the policy at the exclusive sums of their
// weights; returns the total (workgroup-wide, uniform).
template <int W, typename Pol, typename Get>
__device__ __forceinline__ uint64_t cm_unique_write(uint32_t n, uint64_t seg, const Pol& pol, Get get)
{
	__shared__ uint64_t s_w[2][kCmThreads / 64];
	const uint32_t tid = threadIdx.x, w = tid >> 6;
	uint64_t run = 0;
	uint32_t it = 0;
	for (uint32_t base = 0; base < n; base += kCmThreads, it ^= 1) {
		const uint32_t i = base + tid;
		CmKey<W> k = {};
		uint64_t wt = 0;
		if (i < n) {
			k = get(i);
			if (i == 0 || !cm_eq(k, get(i - 1)))
				wt = pol.weight(k);
		}
		const uint64_t incl = cm_wave_incl_scan(wt);
		if (lane_id() == 63)
			s_w[it][w] = incl;
		__syncthreads();  // (s_w[it] is rewritten two sweeps on, past the next sweep's barrier)
		uint64_t wb = 0, tot = 0;
#pragma unroll
		for (uint32_t x = 0; x < kCmThreads / 64; x++) {
			wb += x < w ? s_w[it][x] : 0;
			tot += s_w[it][x];
		}
		if (wt)
			pol.put(seg, run + wb + incl - wt, k);
		run += tot;
	}
	return run;
}

__device__ __forceinline__ uint32_t cm_pow2(uint32_t n)
{
	uint32_t N = 1;
	while (N < n)
		N <<= 1;
	return N;
}

template <int W>
__device__ __forceinline__ void cm_pad(CmTileLds<W>& t, uint32_t n, uint32_t N)
{
	CmKey<W> pad;
#pragma unroll
	for (int w = 0; w < W; w++)
		pad.w[w] = ~0ull;
	for (uint32_t i = n + threadIdx.x; i < N; i += kCmThreads)
		t.set(i, pad);  // (>= every key: the first n sorted keys are the segment's)
}

template <int W, typename Pol>
__global__ __launch_bounds__(kCmThreads) void k_cm_small(CmSegs S, Pol pol)
{
	__shared__ CmTileLds<W> t;
	for (uint64_t seg = blockIdx.x; seg < S.nseg; seg += gridDim.x) {
		const uint32_t n = S.seg_len[seg];
		if (n > kCmTile)
			continue;  // k_cm_unique_large finishes it
		if (n == 0) {
			if (threadIdx.x == 0)
				pol.finish(seg, 0);
			continue;
		}
		const uint32_t N = cm_pow2(n);  // <= kCmTile
		cm_load<W>(S, seg, 0, n, t);
		cm_pad<W>(t, n, N);
		cm_sort<W>(t, N);
		const uint64_t c = cm_unique_write<W>(n, seg, pol, [&](uint32_t i) { return t.get(i); });
		if (threadIdx.x == 0)
			pol.finish(seg, c);
		__syncthreads();  // t is refilled for the next segment
	}
}

// Every segment longer than a tile takes a slot, a key range and its tiles.
// The capacities are the counts the prep kernel took over the same lengths, so
// the checks cannot fail; they keep a write inside its array whatever happens.
__global__ __launch_bounds__(256) void k_cm_register(const uint32_t* __restrict__ seg_len, uint64_t nseg,
                                                     uint64_t cap_large, uint64_t cap_tiles, uint64_t cap_keys,
                                                     uint64_t* lg_seg, uint64_t* lg_base, uint32_t* tile_lg,
                                                     uint32_t* tile_idx, unsigned long long* cnt)
{
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg)
		return;
	const uint32_t len = seg_len[s];
	if (len <= kCmTile)
		return;
	const uint32_t nt = (len + kCmTile - 1) / kCmTile;
	const uint64_t L = atomicAdd(&cnt[kCmCurLarge], 1ull), tb = atomicAdd(&cnt[kCmCurTiles], (unsigned long long)nt),
	               kb = atomicAdd(&cnt[kCmCurKeys], (unsigned long long)len);
	if (L >= cap_large || tb + nt > cap_tiles || kb + len > cap_keys) {
		atomicAdd(&cnt[kCntError], 1ull);
		return;
	}
	lg_seg[L] = s;
	lg_base[L] = kb;
	for (uint32_t t = 0; t < nt; t++) {
		tile_lg[tb + t] = (uint32_t)L;
		tile_idx[tb + t] = t;
	}
}

// the sort buffers hold a key's W words side by side
template <int W>
__device__ __forceinline__ CmKey<W> cm_buf_get(const uint64_t* __restrict__ p, uint64_t i)
{
	CmKey<W> x;
#pragma unroll
	for (int w = 0; w < W; w++)
		x.w[w] = p[i * W + w];
	return x;
}

template <int W>
__global__ __launch_bounds__(kCmThreads) void k_cm_tile_sort(CmSegs S, CmLarge G, uint64_t ntiles, uint64_t* buf,
                                                              const unsigned long long* cnt)
{
	__shared__ CmTileLds<W> t;
	if (cnt[kCntError])
		return;  // k_cm_register left a table unwritten: the call fails, nothing reads it
	for (uint64_t b = blockIdx.x; b < ntiles; b += gridDim.x) {
		const uint32_t L = G.tile_lg[b];
		const uint64_t seg = G.lg_seg[L];
		const uint32_t len = S.seg_len[seg], lo = G.tile_idx[b] * kCmTile;
		const uint32_t n = len - lo < kCmTile ? len - lo : kCmTile, N = cm_pow2(n);
		cm_load<W>(S, seg, lo, n, t);
		cm_pad<W>(t, n, N);
		cm_sort<W>(t, N);
		uint64_t* o = buf + (G.lg_base[L] + lo) * W;
		for (uint32_t i = threadIdx.x; i < n; i += kCmThreads) {
			const CmKey<W> x = t.get(i);
#pragma unroll
			for (int w = 0; w < W; w++)
				o[(uint64_t)i * W + w] = x.w[w];
		}
		__syncthreads();
	}
}

// the first index in [lo, hi) of the sorted keys p whose key is >= x (kUpper: > x)
template <int W, bool kUpper>
__device__ __forceinline__ uint64_t cm_bound(const uint64_t* __restrict__ p, uint64_t lo, uint64_t hi,
                                             const CmKey<W>& x)
{
	for (uint32_t it = 0; it < 32 && lo < hi; it++) {  // hi - lo < 2^31 halves every step
		const uint64_t mid = lo + ((hi - lo) >> 1);
		const CmKey<W> v = cm_buf_get<W>(p, mid);
		if (kUpper ? !cm_lt(x, v) : cm_lt(v, x))
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// one merge pass: sorted runs of w keys -> sorted runs of 2 w keys
template <int W>
__global__ __launch_bounds__(kCmThreads) void k_cm_merge(const uint32_t* __restrict__ seg_len, CmLarge G,
                                                          uint64_t ntiles, uint64_t w,
                                                          const uint64_t* __restrict__ src, uint64_t* dst,
                                                          const unsigned long long* cnt)
{
	if (cnt[kCntError])
		return;
	for (uint64_t b = blockIdx.x; b < ntiles; b += gridDim.x) {
		const uint32_t L = G.tile_lg[b];
		const uint64_t len = seg_len[G.lg_seg[L]], lo = (uint64_t)G.tile_idx[b] * kCmTile;
		const uint64_t n = len - lo < kCmTile ? len - lo : kCmTile;
		const uint64_t* s = src + G.lg_base[L] * W;
		uint64_t* d = dst + G.lg_base[L] * W;
		// a tile lies inside one run (w is a multiple of the tile): uniform per workgroup
		const uint64_t pb = lo / (2 * w) * (2 * w), a1 = std::min(pb + w, len), b1 = std::min(pb + 2 * w, len);
		const bool left = lo < a1;
		for (uint64_t li = lo + threadIdx.x; li < lo + n; li += kCmThreads) {
			const CmKey<W> x = cm_buf_get<W>(s, li);
			const uint64_t pos = left ? li + (cm_bound<W, false>(s, a1, b1, x) - a1)
			                          : pb + (li - a1) + (cm_bound<W, true>(s, pb, a1, x) - pb);
#pragma unroll
			for (int q = 0; q < W; q++)
				d[pos * W + q] = x.w[q];
		}
	}
}

template <int W, typename Pol>
__global__ __launch_bounds__(kCmThreads) void k_cm_unique_large(CmSegs S, CmLarge G, uint64_t nlarge,
                                                                 const uint64_t* __restrict__ buf, Pol pol,
                                                                 const unsigned long long* cnt)
{
	if (cnt[kCntError])
		return;
	for (uint64_t L = blockIdx.x; L < nlarge; L += gridDim.x) {
		const uint64_t seg = G.lg_seg[L];
		const uint32_t n = S.seg_len[seg];
		const uint64_t* s = buf + G.lg_base[L] * W;
		const uint64_t c = cm_unique_write<W>(n, seg, pol, [&](uint32_t i) { return cm_buf_get<W>(s, i); });
		if (threadIdx.x == 0)
			pol.finish(seg, c);
		__syncthreads();
	}
}

// segment i's sorted keys from the staging buffer to their place in the output
template <int W>
__global__ __launch_bounds__(kCmThreads) void k_cm_gather(const uint64_t* __restrict__ stage,
                                                           const uint64_t* __restrict__ stage_pos,
                                                           uint64_t pos_stride, const uint64_t* __restrict__ off,
                                                           uint64_t nseg, uint64_t* out, uint64_t* out_off)
{
	for (uint64_t i = blockIdx.x; i < nseg; i += gridDim.x) {
		const uint64_t a = off[i], n = (off[i + 1] - a) * W;
		const uint64_t* s = stage + stage_pos[i * pos_stride] * W;
		for (uint64_t x = threadIdx.x; x < n; x += kCmThreads)
			out[a * W + x] = s[x];
		if (threadIdx.x == 0)
			out_off[i] = a;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
		out_off[nseg] = off[nseg];
}

// ---- syzsig_comp_map_dev ----

// the ranges are inside the buffer, a call has at most 65535 records
__global__ __launch_bounds__(256) void k_cm_check_regions(const uint64_t* __restrict__ comps_start,
                                                          const uint32_t* __restrict__ comps_cnt,
                                                          const uint64_t* __restrict__ comps_end, uint64_t ncalls,
                                                          uint64_t nwords, unsigned long long* cnt)
{
	uint64_t err = 0;
	const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (c < ncalls) {
		const uint64_t end = comps_end ? comps_end[c] : nwords;
		if (comps_cnt[c] > kCmMaxComps || end > nwords || comps_start[c] > end)
			err++;
	}
	block_count(&cnt[kCntError], err);
}

// ipc.go:420-465 per call, one lane each: a record's length depends on its
// type, so the walk is a dependent chain.  The raw pairs go to the call's
// staging range of 2 * comps_cnt pairs at 2 * rec_base[c].
__global__ __launch_bounds__(64) void k_cm_walk(const uint32_t* __restrict__ words,
                                                const uint64_t* __restrict__ comps_start,
                                                const uint32_t* __restrict__ comps_cnt,
                                                const uint64_t* __restrict__ comps_end, uint64_t ncalls,
                                                uint64_t nwords, const uint64_t* __restrict__ rec_base,
                                                uint64_t* stage, uint64_t* pair_start, uint32_t* pair_len,
                                                int32_t* status)
{
	const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= ncalls)
		return;
	const uint64_t hi = comps_end ? comps_end[c] : nwords;
	const uint32_t n = comps_cnt[c];
	uint64_t pos = comps_start[c];
	uint64_t* o = stage + 4 * rec_base[c];
	uint32_t np = 0;
	int32_t st = SYZSIG_INGEST_OK;
	for (uint32_t j = 0; j < n; j++) {
		if (pos >= hi) {  // ipc.go:424-428
			st = SYZSIG_INGEST_ECOMPS;
			break;
		}
		const uint32_t typ = words[pos++];
		if (typ > (kCmpConst | kCmpSizeMask)) {  // ipc.go:429-433
			st = SYZSIG_INGEST_ECOMPTYPE;
			break;
		}
		uint64_t op1, op2;
		if ((typ & kCmpSizeMask) == kCmpSize8) {  // ipc.go:438-442
			if (hi - pos < 4) {
				st = SYZSIG_INGEST_ECOMPS;
				break;
			}
			op1 = words[pos] | (uint64_t)words[pos + 1] << 32;
			op2 = words[pos + 2] | (uint64_t)words[pos + 3] << 32;
			pos += 4;
		} else {  // ipc.go:443-451: zero-extended
			if (hi - pos < 2) {
				st = SYZSIG_INGEST_ECOMPS;
				break;
			}
			op1 = words[pos];
			op2 = words[pos + 1];
			pos += 2;
		}
		if (op1 == op2)  // ipc.go:452-454
			continue;
		o[2 * np] = op2;  // AddComp(op2, op1), ipc.go:455
		o[2 * np + 1] = op1;
		np++;
		if (typ & kCmpConst)  // ipc.go:456-462
			continue;
		o[2 * np] = op1;  // AddComp(op1, op2), ipc.go:463
		o[2 * np + 1] = op2;
		np++;
	}
	pair_start[c] = 2 * rec_base[c];
	pair_len[c] = st == SYZSIG_INGEST_OK ? np : 0;  // the Go returns before :465: no map
	status[c] = st;
}

// ---- syzsig_shrink_expand_dev ----

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

// per (query, variant): the range of the call's pairs whose key is the mutant
__global__ __launch_bounds__(256) void k_se_count(const uint64_t* __restrict__ map_off,
                                                  const uint64_t* __restrict__ pairs, uint64_t ncalls,
                                                  uint64_t npairs, const uint32_t* __restrict__ q_call,
                                                  const uint64_t* __restrict__ q_val, uint64_t nq, uint64_t* vlo,
                                                  uint32_t* vcnt, unsigned long long* cnt)
{
	uint64_t err = 0;
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g < nq * kCmVariants) {
		const uint64_t q = g / kCmVariants;
		const uint32_t x = (uint32_t)(g % kCmVariants), call = q_call[q];
		uint64_t a = 0, b = 0;
		bool ok = call < ncalls;
		if (ok) {
			a = map_off[call];
			b = map_off[call + 1];
			ok = a <= b && b <= npairs && b - a <= kCmMaxSeg;
		}
		if (!ok) {
			err += x == 0;
			vlo[g] = 0;
			vcnt[g] = 0;
		} else {
			uint32_t width;
			bool expand, be;
			cm_variant(x, width, expand, be);
			const uint64_t m = cm_mutant(q_val[q], width, expand, be);
			uint64_t lo = a, hi = b;  // the first pair with key >= m
			for (uint32_t it = 0; it < 32 && lo < hi; it++) {
				const uint64_t mid = lo + ((hi - lo) >> 1);
				if (pairs[2 * mid] < m)
					lo = mid + 1;
				else
					hi = mid;
			}
			const uint64_t first = lo;
			hi = b;  // the first pair with key > m
			for (uint32_t it = 0; it < 32 && lo < hi; it++) {
				const uint64_t mid = lo + ((hi - lo) >> 1);
				if (pairs[2 * mid] <= m)
					lo = mid + 1;
				else
					hi = mid;
			}
			vlo[g] = first;
			vcnt[g] = (uint32_t)(lo - first);
		}
	}
	block_count(&cnt[kCntError], err);
}

__device__ __forceinline__ bool cm_is_special(const uint64_t* __restrict__ sp, uint32_t nsp, uint64_t v)
{
	uint32_t lo = 0, hi = nsp;
	for (uint32_t it = 0; it < 32 && lo < hi; it++) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (sp[mid] < v)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < nsp && sp[lo] == v;
}

// hints.go:192-213, one wave per query: the accepted replacers of variant x
// packed at the head of its candidate range cand[voff[q * 12 + x] ..], their
// count in src_len
__global__ __launch_bounds__(256) void k_se_write(const uint64_t* __restrict__ pairs,
                                                  const uint64_t* __restrict__ q_val, uint64_t nq,
                                                  const uint64_t* __restrict__ vlo, const uint32_t* __restrict__ vcnt,
                                                  const uint64_t* __restrict__ voff,
                                                  const uint64_t* __restrict__ special, uint32_t nspecial,
                                                  uint64_t* cand, uint32_t* src_len)
{
	const uint32_t lane = lane_id();
	const uint64_t q = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
	if (q >= nq)
		return;  // (whole waves: no barrier below)
	const uint64_t v = q_val[q];
	for (uint32_t x = 0; x < kCmVariants; x++) {
		const uint64_t g = q * kCmVariants + x, lo = vlo[g];
		const uint32_t n = vcnt[g];
		uint64_t* o = cand + voff[g];
		uint32_t width;
		bool expand, be;
		cm_variant(x, width, expand, be);
		const uint64_t mask = cm_mask(width);
		uint32_t run = 0;
		for (uint32_t base = 0; base < n; base += 64) {
			const uint32_t i = base + lane;
			bool acc = false;
			uint64_t rep = 0;
			if (i < n) {
				uint64_t nv = pairs[2 * (lo + i) + 1];
				const uint64_t hi = nv & ~mask;
				nv &= mask;
				acc = hi == 0 || (hi ^ ~mask) == 0;  // hints.go:194-198
				if (be)
					nv = cm_swap(nv, width);  // hints.go:199-201
				acc = acc && !cm_is_special(special, nspecial, nv);  // hints.go:202-204
				rep = (v & ~mask) | nv;  // hints.go:207
			}
			const uint64_t m = __ballot(acc);
			if (acc)
				o[run + lane_rank(m)] = rep;
			run += (uint32_t)__popcll(m);
		}
		if (lane == 0)
			src_len[g] = run;
	}
}

static size_t cm_align(size_t b) { return (b + 255) & ~(size_t)255; }

static int cm_grid(uint64_t n) { return (int)std::min<uint64_t>(std::max<uint64_t>(n, 1), 1u << 20); }

// The sort-unique of every segment of S (lengths and counts as the prep
// kernel left them in ctx->h_cnt).  Enqueues only.
template <int W, typename Pol>
static int cm_sort_unique(syzsig_ctx* ctx, const CmSegs& S, const Pol& pol)
{
	const hipStream_t s = ctx->stream;
	const uint64_t nlarge = ctx->h_cnt[kCmLarge], ntiles = ctx->h_cnt[kCmTiles], nkeys = ctx->h_cnt[kCmKeys],
	               maxlen = ctx->h_cnt[kCmMaxLen];
	k_cm_small<W, Pol><<<cm_grid(S.nseg), kCmThreads, 0, s>>>(S, pol);
	if (nlarge) {
		char* tab;
		void *ba, *bb;
		const size_t o_base = cm_align(nlarge * 8), o_tlg = o_base + cm_align(nlarge * 8),
		             o_tix = o_tlg + cm_align(ntiles * 4);
		SYZ_TRY(ws_get(ctx, kWsSuTab, o_tix + cm_align(ntiles * 4), (void**)&tab));
		SYZ_TRY(ws_get(ctx, kWsSuBufA, nkeys * 8 * W + 256, &ba));
		SYZ_TRY(ws_get(ctx, kWsSuBufB, nkeys * 8 * W + 256, &bb));
		uint64_t* lg_seg = (uint64_t*)tab;
		uint64_t* lg_base = (uint64_t*)(tab + o_base);
		uint32_t* tile_lg = (uint32_t*)(tab + o_tlg);
		uint32_t* tile_idx = (uint32_t*)(tab + o_tix);
		k_cm_register<<<(int)((S.nseg + 255) / 256), 256, 0, s>>>(S.seg_len, S.nseg, nlarge, ntiles, nkeys, lg_seg,
		                                                          lg_base, tile_lg, tile_idx, ctx->d_cnt);
		const CmLarge G{lg_seg, lg_base, tile_lg, tile_idx};
		uint64_t *src = (uint64_t*)ba, *dst = (uint64_t*)bb;
		k_cm_tile_sort<W><<<cm_grid(ntiles), kCmThreads, 0, s>>>(S, G, ntiles, src, ctx->d_cnt);
		for (uint64_t w = kCmTile; w < maxlen; w <<= 1) {
			k_cm_merge<W><<<cm_grid(ntiles), kCmThreads, 0, s>>>(S.seg_len, G, ntiles, w, src, dst, ctx->d_cnt);
			std::swap(src, dst);
		}
		k_cm_unique_large<W, Pol><<<cm_grid(nlarge), kCmThreads, 0, s>>>(S, G, nlarge, src, pol, ctx->d_cnt);
	}
	SYZ_HIP(hipGetLastError());
	return SYZSIG_OK;
}

static int cm_finish_timing(syzsig_ctx* ctx)
{
	if (ctx->timing) {
		float t = 0;
		SYZ_HIP(hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]));
		ctx->last_ms = t;
	}
	return SYZSIG_OK;
}

// The tail the two CSR entry points share: the segments' survivors lie in
// `stage` (segment i's at stage_pos[i * pos_stride], cnt[i] of them); their
// offsets, the capacity check and the gather.
template <int W>
static int cm_emit_csr(syzsig_ctx* ctx, const char* what, const uint64_t* stage, const uint64_t* stage_pos,
                       uint64_t pos_stride, const uint32_t* cnt, uint64_t* off, uint64_t nseg, uint64_t* d_off,
                       uint64_t* d_out, uint64_t cap, uint64_t* n_out, int32_t* d_status = nullptr,
                       const int32_t* status = nullptr)
{
	const hipStream_t s = ctx->stream;
	k_cm_scan<<<1, kCmThreads, 0, s>>>(cnt, nseg, off);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, off + nseg, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, std::string(what) + ": internal: a long segment did not fit its workspace");
	*n_out = total;
	if (total > cap)
		return fail(SYZSIG_ERANGE, std::string(what) + ": the result needs more than the given capacity");
	k_cm_gather<W><<<cm_grid(nseg), kCmThreads, 0, s>>>(stage, stage_pos, pos_stride, off, nseg, d_out, d_off);
	SYZ_HIP(hipGetLastError());
	if (d_status)
		SYZ_HIP(hipMemcpyAsync(d_status, status, nseg * 4, hipMemcpyDeviceToDevice, s));
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[1], s));
	SYZ_HIP(hipStreamSynchronize(s));
	return cm_finish_timing(ctx);
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_exec_comps_dev(syzsig_ctx* ctx, const uint64_t* d_comps, uint64_t ncmp,
                                     const uint64_t* d_call_start, const uint32_t* d_call_len, uint64_t ncalls,
                                     uint64_t out_start, uint32_t* d_out, uint32_t* d_out_words,
                                     uint32_t* d_comps_cnt)
{
	SYZ_LOCK(ctx);
	if (!ctx || (ncalls && (!d_call_start || !d_call_len || !d_out_words || !d_comps_cnt)) ||
	    (ncmp && (!d_comps || !d_out)))
		return fail(SYZSIG_EINVAL, "exec_comps: NULL argument");
	if (ncmp > (1ull << 58))
		return fail(SYZSIG_EINVAL, "exec_comps: record count out of range");
	if (ncalls == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	void* seg_len;
	SYZ_TRY(ws_get(ctx, kWsSuMeta, ncalls * 4 + 256, &seg_len));
	SYZ_TRY(counters_reset(ctx));
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[0], s));
	k_cm_prep_calls<<<(int)((ncalls + 255) / 256), 256, 0, s>>>(d_call_start, d_call_len, ncalls, ncmp,
	                                                            (uint32_t*)seg_len, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "exec_comps: a call's records lie outside the buffer, or a call has more than "
		                           "65535 comparisons");
	const CmSegs S{d_comps, 4, d_call_start, (const uint32_t*)seg_len, 1, (const uint32_t*)seg_len, ncalls};
	const CmOutComps pol{d_out, d_call_start, d_out_words, d_comps_cnt, out_start};
	SYZ_TRY((cm_sort_unique<3, CmOutComps>(ctx, S, pol)));
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[1], s));
	SYZ_TRY(counters_fetch(ctx));
	SYZ_TRY(cm_finish_timing(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "exec_comps: internal: a long segment did not fit its workspace");
	return SYZSIG_OK;
}

extern "C" int syzsig_comp_map_dev(syzsig_ctx* ctx, const uint32_t* d_words, uint64_t nwords,
                                   const uint64_t* d_comps_start, const uint32_t* d_comps_cnt,
                                   const uint64_t* d_comps_end, uint64_t ncalls, int32_t* d_status,
                                   uint64_t* d_map_off, uint64_t* d_pairs, uint64_t cap, uint64_t* n_out)
{
	SYZ_LOCK(ctx);
	if (n_out)
		*n_out = 0;
	if (!ctx || !d_map_off || !n_out || (ncalls && (!d_comps_start || !d_comps_cnt || !d_status)) ||
	    (nwords && !d_words) || (cap && !d_pairs))
		return fail(SYZSIG_EINVAL, "comp_map: NULL argument");
	const hipStream_t s = ctx->stream;
	if (ncalls == 0) {
		SYZ_HIP(hipMemsetAsync(d_map_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	// rec_base[ncalls + 1], pair_start[ncalls], pair_len[ncalls], seg_len[ncalls], cnt[ncalls], off[ncalls + 1],
	// status[ncalls] (nothing of the caller's is written before the capacity check)
	char* d;
	const size_t o_ps = cm_align((ncalls + 1) * 8), o_pl = o_ps + cm_align(ncalls * 8), o_sl = o_pl + cm_align(ncalls * 4),
	             o_cnt = o_sl + cm_align(ncalls * 4), o_off = o_cnt + cm_align(ncalls * 4), o_st = o_off + cm_align((ncalls + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsSuMeta, o_st + cm_align(ncalls * 4), (void**)&d));
	uint64_t *rec_base = (uint64_t*)d, *pair_start = (uint64_t*)(d + o_ps), *off = (uint64_t*)(d + o_off);
	uint32_t *pair_len = (uint32_t*)(d + o_pl), *seg_len = (uint32_t*)(d + o_sl), *cnt = (uint32_t*)(d + o_cnt);
	int32_t* status = (int32_t*)(d + o_st);
	SYZ_TRY(counters_reset(ctx));
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[0], s));
	const int cb = (int)((ncalls + 255) / 256);
	k_cm_check_regions<<<cb, 256, 0, s>>>(d_comps_start, d_comps_cnt, d_comps_end, ncalls, nwords, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "comp_map: a call's comparisons start outside its region, a region ends outside "
		                           "the buffer, or a call has more than 65535 comparisons");
	k_cm_scan<<<1, kCmThreads, 0, s>>>(d_comps_cnt, ncalls, rec_base);
	SYZ_HIP(hipGetLastError());
	uint64_t nrec = 0;
	SYZ_HIP(hipMemcpyAsync(&nrec, rec_base + ncalls, 8, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipStreamSynchronize(s));
	void *stage, *stage2;  // two pairs of two words per record
	SYZ_TRY(ws_get(ctx, kWsSuStage, nrec * 32 + 256, &stage));
	SYZ_TRY(ws_get(ctx, kWsSuStage2, nrec * 32 + 256, &stage2));
	k_cm_walk<<<(int)((ncalls + 63) / 64), 64, 0, s>>>(d_words, d_comps_start, d_comps_cnt, d_comps_end, ncalls,
	                                                   nwords, rec_base, (uint64_t*)stage, pair_start, pair_len,
	                                                   status);
	k_cm_prep_sources<<<cb, 256, 0, s>>>(pair_len, 1, ncalls, seg_len, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	const CmSegs S{(const uint64_t*)stage, 2, pair_start, pair_len, 1, seg_len, ncalls};
	const CmOutKeys<2> pol{(uint64_t*)stage2, pair_start, 1, cnt};
	SYZ_TRY((cm_sort_unique<2, CmOutKeys<2>>(ctx, S, pol)));
	return cm_emit_csr<2>(ctx, "comp_map", (const uint64_t*)stage2, pair_start, 1, cnt, off, ncalls, d_map_off,
	                      d_pairs, cap, n_out, d_status, status);
}

extern "C" int syzsig_shrink_expand_dev(syzsig_ctx* ctx, const uint64_t* d_map_off, const uint64_t* d_pairs,
                                        uint64_t ncalls, uint64_t npairs, const uint32_t* d_q_call,
                                        const uint64_t* d_q_val, uint64_t nq, const uint64_t* special_ints,
                                        uint32_t nspecial, uint64_t* d_rep_off, uint64_t* d_rep, uint64_t cap,
                                        uint64_t* n_out)
{
	SYZ_LOCK(ctx);
	if (n_out)
		*n_out = 0;
	if (!ctx || !d_rep_off || !n_out || !d_map_off || (npairs && !d_pairs) || (nq && (!d_q_call || !d_q_val)) ||
	    (nspecial && !special_ints) || (cap && !d_rep))
		return fail(SYZSIG_EINVAL, "shrink_expand: NULL argument");
	if (nspecial > kCmMaxSpecial)
		return fail(SYZSIG_ERANGE, "shrink_expand: at most 4096 special ints");
	if (nq > (1ull << 32))
		return fail(SYZSIG_EINVAL, "shrink_expand: query count out of range");
	const hipStream_t s = ctx->stream;
	if (nq == 0) {
		SYZ_HIP(hipMemsetAsync(d_rep_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	const uint64_t nv = nq * kCmVariants;
	// vlo[nv], voff[nv + 1], vcnt[nv], src_len[nv], seg_len[nq], cnt[nq], off[nq + 1], special[nspecial]
	char* d;
	const size_t o_voff = cm_align(nv * 8), o_vcnt = o_voff + cm_align((nv + 1) * 8), o_sl = o_vcnt + cm_align(nv * 4),
	             o_seg = o_sl + cm_align(nv * 4), o_cnt = o_seg + cm_align(nq * 4), o_off = o_cnt + cm_align(nq * 4),
	             o_sp = o_off + cm_align((nq + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsSuMeta, o_sp + cm_align((size_t)nspecial * 8 + 8), (void**)&d));
	uint64_t *vlo = (uint64_t*)d, *voff = (uint64_t*)(d + o_voff), *off = (uint64_t*)(d + o_off),
	         *special = (uint64_t*)(d + o_sp);
	uint32_t *vcnt = (uint32_t*)(d + o_vcnt), *src_len = (uint32_t*)(d + o_sl), *seg_len = (uint32_t*)(d + o_seg),
	         *cnt = (uint32_t*)(d + o_cnt);
	std::vector<uint64_t> sp(special_ints, special_ints + nspecial);
	std::sort(sp.begin(), sp.end());
	SYZ_TRY(counters_reset(ctx));
	if (nspecial) {  // (pageable: the copy has left sp when the call returns)
		SYZ_HIP(hipMemcpyAsync(special, sp.data(), (size_t)nspecial * 8, hipMemcpyHostToDevice, s));
		SYZ_HIP(hipStreamSynchronize(s));
	}
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[0], s));
	k_se_count<<<(int)((nv + 255) / 256), 256, 0, s>>>(d_map_off, d_pairs, ncalls, npairs, d_q_call, d_q_val, nq, vlo,
	                                                   vcnt, ctx->d_cnt);
	k_cm_scan<<<1, kCmThreads, 0, s>>>(vcnt, nv, voff);
	SYZ_HIP(hipGetLastError());
	uint64_t ncand = 0;
	SYZ_HIP(hipMemcpyAsync(&ncand, voff + nv, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "shrink_expand: a query's call is outside the map, or the map's offsets are not "
		                           "ascending inside its pairs");
	void *cand, *stage2;
	SYZ_TRY(ws_get(ctx, kWsSuStage, ncand * 8 + 256, &cand));
	SYZ_TRY(ws_get(ctx, kWsSuStage2, ncand * 8 + 256, &stage2));
	k_se_write<<<(int)((nq + 3) / 4), 256, 0, s>>>(d_pairs, d_q_val, nq, vlo, vcnt, voff, special, nspecial,
	                                               (uint64_t*)cand, src_len);
	k_cm_prep_sources<<<(int)((nq + 255) / 256), 256, 0, s>>>(src_len, kCmVariants, nq, seg_len, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntOverflow])
		return fail(SYZSIG_ERANGE, "shrink_expand: a query has 2^31 or more candidates");
	const CmSegs S{(const uint64_t*)cand, 1, voff, src_len, kCmVariants, seg_len, nq};
	// a query's survivors go to the head of its own candidate range in stage2
	const CmOutKeys<1> pol{(uint64_t*)stage2, voff, kCmVariants, cnt};
	SYZ_TRY((cm_sort_unique<1, CmOutKeys<1>>(ctx, S, pol)));
	return cm_emit_csr<1>(ctx, "shrink_expand", (const uint64_t*)stage2, voff, kCmVariants, cnt, off, nq,
	                      d_rep_off, d_rep, cap, n_out);
}
