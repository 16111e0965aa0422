// segsort.h -- the segmented sort-unique and the sort-and-walk, once: shared by
// cover.hip and items.hip (u32 keys), comps.hip (keys of 1-3 u64 words),
// corpus.hip and poll.hip (u64 keys = keys of one word).  Everything here is a template or
// inline: each translation unit instantiates what it launches.
//
// Per segment: sort ascending, drop equal neighbours, hand the survivors to an
// output policy.  With T = Tile::kTile keys:
//   k_su_small        one workgroup per segment of <= T keys: the keys into
//                     LDS, padded to a power of two with all-ones keys, bitonic
//                     sort, then neighbour flags, block scan, compacted write.
//   segments longer than T go through two workspace buffers in HBM, described
//   by one tile table (SuTiles):
//   k_su_register     each long segment takes a slot, a key range and its
//                     tiles (three atomics per SEGMENT; none per key anywhere);
//                     corpus.hip fills the table on the host instead
//   k_su_tile_sort    one workgroup per tile of T keys: sorted in LDS
//   k_su_merge        ceil(log2(tiles of the longest segment)) passes, known
//                     at launch: runs of w keys merged pairwise into runs of
//                     2 w by rank -- a key of the left run goes to its index
//                     plus the keys of the right run below it (lower bound),
//                     a key of the right run to its index plus the keys of the
//                     left run not above it (upper bound): a bijection onto
//                     the pair's range, duplicates included, no waiting.  A
//                     segment of at most w keys is copied through, so every
//                     segment is in the same buffer after every pass.
//   k_su_unique_large one workgroup per segment streams its sorted keys:
//                     flags, block scan with a running count, compacted write
//   k_su_scan, k_su_gather   survivors' counts -> offsets -> CSR output
//   su_sort_unique    the host driver of all of the above (enqueues only)
// Every loop is bounded by a segment length, a run count, the pass count or
// the kSuSearchSteps of a binary search; nothing waits for another wave.
//
// A key type (SuU32, SuU64<W>) gives the value type T, lt / eq, the pad key
// and the key's layout in the HBM sort buffers (get / put over Word).  A tile
// type gives the key, the tile size and the tile's LDS routines: SuWordsTile
// is the plain one (struct-of-arrays tile, su_bitonic) and SuU32Tile the same
// for u32 keys; cover.hip brings its tuned u32 routines as a tile type of its
// own.
//
// su_sort_walk is the other user of the plain sort: Poll's and NewInput's
// workgroup-per-partition event walk (k_poll_part_walk, k_ni_walk).
#pragma once

#include <algorithm>

#include "internal.h"

namespace syz {

constexpr uint32_t kSuThreads = 256;

// the context's counters as the sort uses them (zeroed per call): what the prep
// kernels count over the segment lengths, and k_su_register's cursors
constexpr int kSuLarge = kCntAux, kSuTiles = kCntAux2, kSuKeys = kCntCandidates, kSuMaxLen = kCntTouched,
              kSuTotal = kCntChanged, kSuCurLarge = kCntDefer, kSuCurTiles = kCntDeferNs, kSuCurKeys = kCntDistinct;

// A binary search runs over at most one segment, whose length is a u32, and a
// step takes a range of r keys to at most r / 2.
constexpr uint32_t kSuSearchSteps = 32;

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline int grid_cap(uint64_t n, uint64_t cap = 1u << 20) { return (int)std::min<uint64_t>(std::max<uint64_t>(n, 1), cap); }

// the timed span of an entry point: ev[0] at its first kernel, ev[1] after its
// last, ctx->last_ms once ev[1] has passed
inline int su_time_begin(syzsig_ctx* ctx)
{
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
	return SYZSIG_OK;
}

inline int su_time_end(syzsig_ctx* ctx)
{
	if (ctx->timing) {
		float t = 0;
		SYZ_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
		SYZ_HIP(hipEventSynchronize(ctx->ev[1]));
		SYZ_HIP(hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]));
		ctx->last_ms = t;
	}
	return SYZSIG_OK;
}

// the least power of two >= n and >= min (min a power of two)
template <typename U>
SYZ_HD U pow2_at_least(U n, U min)
{
	U N = min;
	while (N < n)
		N <<= 1;
	return N;
}

#if defined(__HIPCC__)

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v)
{
	const uint32_t lane = lane_id();
#pragma unroll
	for (uint32_t o = 1; o < 64; o <<= 1) {
		const T x = __shfl_up(v, o, 64);
		if (lane >= o)
			v += x;
	}
	return v;
}

// ---- keys ----

struct SuU32 {
	using T = uint32_t;
	using Word = uint32_t;
	static constexpr int kWords = 1;
	static __device__ __forceinline__ bool lt(T a, T b) { return a < b; }
	static __device__ __forceinline__ bool eq(T a, T b) { return a == b; }
	static __device__ __forceinline__ T pad() { return 0xffffffffu; }
	static __device__ __forceinline__ T get(const Word* __restrict__ p, uint64_t i) { return p[i]; }
	static __device__ __forceinline__ void put(Word* p, uint64_t i, T x) { p[i] = x; }
};

template <int W>
struct SuWords {
	uint64_t w[W];
};

// W u64 words, compared word by word; a buffer holds a key's words side by side
template <int W>
struct SuU64 {
	using T = SuWords<W>;
	using Word = uint64_t;
	static constexpr int kWords = W;
	static __device__ __forceinline__ bool lt(const T& a, const T& b)
	{
#pragma unroll
		for (int i = 0; i < W - 1; i++)
			if (a.w[i] != b.w[i])
				return a.w[i] < b.w[i];
		return a.w[W - 1] < b.w[W - 1];
	}
	static __device__ __forceinline__ bool eq(const T& a, const T& b)
	{
		bool e = true;
#pragma unroll
		for (int i = 0; i < W; i++)
			e = e && a.w[i] == b.w[i];
		return e;
	}
	static __device__ __forceinline__ T pad()
	{
		T x;
#pragma unroll
		for (int i = 0; i < W; i++)
			x.w[i] = ~0ull;
		return x;
	}
	static __device__ __forceinline__ T get(const Word* __restrict__ p, uint64_t i)
	{
		T x;
#pragma unroll
		for (int w = 0; w < W; w++)
			x.w[w] = p[i * W + w];
		return x;
	}
	static __device__ __forceinline__ void put(Word* p, uint64_t i, const T& x)
	{
#pragma unroll
		for (int w = 0; w < W; w++)
			p[i * W + w] = x.w[w];
	}
};

// ---- segments, output, tile table ----

// Segment s is the concatenation of its R sources: the keys at src[(src_start[s
// * R + r] + i) * stride ..], i < src_len[s * R + r]; seg_len[s] in all.
struct SuSegs {
	const void* src;
	uint32_t stride;  // words from one key to the next (cover.hip: the source's own width)
	const uint64_t* src_start;
	const uint32_t* src_len;
	uint32_t R;
	const uint32_t* seg_len;
	uint64_t nseg;
};

// output policy: the surviving keys themselves, segment s's from key
// out_pos[s * pos_stride] of out on, their count to out_cnt[s]
template <typename Key>
struct SuOutKeys {
	typename Key::Word* out;
	const uint64_t* out_pos;
	uint64_t pos_stride;
	uint32_t* out_cnt;
	__device__ __forceinline__ typename Key::Word* dst(uint64_t seg) const
	{
		return out + out_pos[seg * pos_stride] * Key::kWords;
	}
	__device__ __forceinline__ uint64_t weight(uint64_t, const typename Key::T&) const { return 1; }
	__device__ __forceinline__ void put(uint64_t seg, uint64_t pos, const typename Key::T& k, uint64_t) const
	{
		Key::put(dst(seg), pos, k);
	}
	__device__ __forceinline__ void finish(uint64_t seg, uint64_t total) const { out_cnt[seg] = (uint32_t)total; }
};

// The segments that go through the HBM buffers -- long segment L is segment
// seg[L] (nullptr: segment L; the host-built table of corpus.hip lists every
// group), len[L] keys from key base[L] of either buffer on -- and the tiles of
// all of them: tile b = keys [tile_idx[b] * T, + T) of long segment tile_owner[b].
struct SuTiles {
	uint64_t* seg;
	uint64_t* base;
	uint32_t* len;
	uint32_t* tile_owner;
	uint32_t* tile_idx;
	uint64_t nlarge, ntiles;
};

// what a prep kernel counts per segment: kAlign = the key-range alignment
template <uint32_t kTile, uint32_t kAlign>
__device__ __forceinline__ void su_count_large(uint32_t len, uint64_t& nl, uint64_t& nt, uint64_t& nk,
                                               unsigned long long* cnt)
{
	if (len > kTile) {
		nl++;
		nt += (len + kTile - 1) / kTile;
		nk += ((uint64_t)len + (kAlign - 1)) & ~(uint64_t)(kAlign - 1);
		atomicMax(&cnt[kSuMaxLen], (unsigned long long)len);
	}
}

// Every segment longer than a tile takes a slot, a key range (a multiple of
// kAlign keys) and its tiles.  The capacities are the counts the prep kernel
// took over the same lengths, so the checks cannot fail; they keep a write
// inside its array whatever happens.
template <uint32_t kTile, uint32_t kAlign>
__global__ __launch_bounds__(256) void k_su_register(const uint32_t* __restrict__ seg_len, uint64_t nseg,
                                                     uint64_t cap_keys, SuTiles T, unsigned long long* cnt)
{
	const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg)
		return;
	const uint32_t len = seg_len[s];
	if (len <= kTile)
		return;
	const uint32_t nt = (len + kTile - 1) / kTile;
	const uint64_t L = atomicAdd(&cnt[kSuCurLarge], 1ull), tb = atomicAdd(&cnt[kSuCurTiles], (unsigned long long)nt),
	               kb = atomicAdd(&cnt[kSuCurKeys],
	                              (unsigned long long)(((uint64_t)len + (kAlign - 1)) & ~(uint64_t)(kAlign - 1)));
	if (L >= T.nlarge || tb + nt > T.ntiles || kb + len > cap_keys) {
		atomicAdd(&cnt[kCntError], 1ull);
		return;
	}
	T.seg[L] = s;
	T.base[L] = kb;
	T.len[L] = len;
	for (uint32_t t = 0; t < nt; t++) {
		T.tile_owner[tb + t] = (uint32_t)L;
		T.tile_idx[tb + t] = t;
	}
}

// ---- the plain tile ----

// Bitonic sort of t[0 .. N) ascending over a tile's get / set; N a power of
// two.  The fill needs no barrier of its own; ends with a barrier.
template <typename Key, typename Lds>
__device__ __forceinline__ void su_bitonic(Lds& t, uint32_t N)
{
	for (uint32_t size = 2; size <= N; size <<= 1) {
		for (uint32_t st = size >> 1; st > 0; st >>= 1) {
			__syncthreads();
			for (uint32_t x = threadIdx.x; x < N / 2; x += kSuThreads) {
				const uint32_t i = 2 * x - (x & (st - 1)), j = i + st;
				const bool asc = (i & size) == 0;
				const typename Key::T a = t.get(i), b = t.get(j);
				if (asc ? Key::lt(b, a) : Key::lt(a, b)) {
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
// weights, each with its own weight (nonzero: what weight() found out about the
// key need not be found out again); returns the total (workgroup-wide, uniform).
template <typename Key, typename Pol, typename Get>
__device__ __forceinline__ uint64_t su_unique_write(uint32_t n, uint64_t seg, const Pol& pol, Get get)
{
	__shared__ uint64_t s_w[2][kSuThreads / 64];
	const uint32_t tid = threadIdx.x, w = tid >> 6;
	uint64_t run = 0;
	uint32_t it = 0;
	for (uint32_t base = 0; base < n; base += kSuThreads, it ^= 1) {
		const uint32_t i = base + tid;
		typename Key::T k = {};
		uint64_t wt = 0;
		if (i < n) {
			k = get(i);
			if (i == 0 || !Key::eq(k, get(i - 1)))
				wt = pol.weight(seg, k);
		}
		const uint64_t incl = wave_incl_scan(wt);
		if (lane_id() == 63)
			s_w[it][w] = incl;
		__syncthreads();  // (s_w[it] is rewritten two sweeps on, past the next sweep's barrier)
		uint64_t wb = 0, tot = 0;
#pragma unroll
		for (uint32_t x = 0; x < kSuThreads / 64; x++) {
			wb += x < w ? s_w[it][x] : 0;
			tot += s_w[it][x];
		}
		if (wt)
			pol.put(seg, run + wb + incl - wt, k, wt);
		run += tot;
	}
	return run;
}

// The plain tile of kTileKeys keys of W words: W arrays of kTileKeys words in
// LDS (a lane's compare reads one word per array: consecutive lanes,
// consecutive 8-B words), 8 W kTileKeys bytes.
template <int W, uint32_t kTileKeys>
struct SuWordsTile {
	using Key = SuU64<W>;
	static constexpr uint32_t kTile = kTileKeys, kAlign = 1, kMinPad = 1;
	struct Lds {
		uint64_t k[W][kTileKeys];
		__device__ __forceinline__ SuWords<W> get(uint32_t i) const
		{
			SuWords<W> x;
#pragma unroll
			for (int w = 0; w < W; w++)
				x.w[w] = k[w][i];
			return x;
		}
		__device__ __forceinline__ void set(uint32_t i, const SuWords<W>& x)
		{
#pragma unroll
			for (int w = 0; w < W; w++)
				k[w][i] = x.w[w];
		}
	};
	// t[0 .. n) = the keys [lo, lo + n) of segment `seg` (workgroup-wide)
	static __device__ __forceinline__ void load(const SuSegs& S, uint64_t seg, uint32_t lo, uint32_t n, Lds& t)
	{
		uint64_t o = 0;
		for (uint32_t r = 0; r < S.R; r++) {
			const uint32_t len = S.src_len[seg * S.R + r];
			const uint64_t a = std::max<uint64_t>(lo, o), b = std::min<uint64_t>((uint64_t)lo + n, o + len);
			if (a < b) {
				const uint64_t* p =
					reinterpret_cast<const uint64_t*>(S.src) + (S.src_start[seg * S.R + r] + (a - o)) * S.stride;
				const uint32_t d = (uint32_t)(a - lo), cnt = (uint32_t)(b - a);
				for (uint32_t i = threadIdx.x; i < cnt; i += kSuThreads) {
#pragma unroll
					for (int w = 0; w < W; w++)
						t.k[w][d + i] = p[(uint64_t)i * S.stride + w];
				}
			}
			o += len;
		}
	}
	// t[n .. N) padded (>= every key: the first n sorted keys are the segment's), t[0 .. N) sorted
	static __device__ __forceinline__ void sort(Lds& t, uint32_t n, uint32_t N)
	{
		for (uint32_t i = n + threadIdx.x; i < N; i += kSuThreads)
			t.set(i, Key::pad());
		su_bitonic<Key>(t, N);
	}
	static __device__ __forceinline__ void store(const Lds& t, uint32_t n, uint64_t* o)
	{
		for (uint32_t i = threadIdx.x; i < n; i += kSuThreads)
			Key::put(o, i, t.get(i));
	}
	template <typename Pol>
	static __device__ __forceinline__ uint64_t unique_lds(uint32_t n, uint64_t seg, const Pol& pol, const Lds& t)
	{
		return su_unique_write<Key>(n, seg, pol, [&](uint32_t i) { return t.get(i); });
	}
	template <typename Pol>
	static __device__ __forceinline__ uint64_t unique_buf(uint32_t n, uint64_t seg, const Pol& pol, const uint64_t* s)
	{
		return su_unique_write<Key>(n, seg, pol, [&](uint32_t i) { return Key::get(s, i); });
	}
};

// The plain tile of kTileKeys u32 keys (sources of u32 words): one array in
// LDS, 4 kTileKeys bytes.
template <uint32_t kTileKeys>
struct SuU32Tile {
	using Key = SuU32;
	static constexpr uint32_t kTile = kTileKeys, kAlign = 1, kMinPad = 1;
	struct Lds {
		uint32_t k[kTileKeys];
		__device__ __forceinline__ uint32_t get(uint32_t i) const { return k[i]; }
		__device__ __forceinline__ void set(uint32_t i, uint32_t x) { k[i] = x; }
	};
	static __device__ __forceinline__ void load(const SuSegs& S, uint64_t seg, uint32_t lo, uint32_t n, Lds& t)
	{
		uint64_t o = 0;
		for (uint32_t r = 0; r < S.R; r++) {
			const uint32_t len = S.src_len[seg * S.R + r];
			const uint64_t a = std::max<uint64_t>(lo, o), b = std::min<uint64_t>((uint64_t)lo + n, o + len);
			if (a < b) {
				const uint32_t* p =
					reinterpret_cast<const uint32_t*>(S.src) + (S.src_start[seg * S.R + r] + (a - o)) * S.stride;
				const uint32_t d = (uint32_t)(a - lo), cnt = (uint32_t)(b - a);
				for (uint32_t i = threadIdx.x; i < cnt; i += kSuThreads)
					t.k[d + i] = p[(uint64_t)i * S.stride];
			}
			o += len;
		}
	}
	static __device__ __forceinline__ void sort(Lds& t, uint32_t n, uint32_t N)
	{
		for (uint32_t i = n + threadIdx.x; i < N; i += kSuThreads)
			t.k[i] = Key::pad();
		su_bitonic<Key>(t, N);
	}
	static __device__ __forceinline__ void store(const Lds& t, uint32_t n, uint32_t* o)
	{
		for (uint32_t i = threadIdx.x; i < n; i += kSuThreads)
			o[i] = t.k[i];
	}
	template <typename Pol>
	static __device__ __forceinline__ uint64_t unique_lds(uint32_t n, uint64_t seg, const Pol& pol, const Lds& t)
	{
		return su_unique_write<Key>(n, seg, pol, [&](uint32_t i) { return t.k[i]; });
	}
	template <typename Pol>
	static __device__ __forceinline__ uint64_t unique_buf(uint32_t n, uint64_t seg, const Pol& pol, const uint32_t* s)
	{
		return su_unique_write<Key>(n, seg, pol, [&](uint32_t i) { return s[i]; });
	}
};

// ---- kernels ----

template <typename Tile, typename Pol>
__global__ __launch_bounds__(kSuThreads) void k_su_small(SuSegs S, Pol pol)
{
	__shared__ typename Tile::Lds t;
	for (uint64_t seg = blockIdx.x; seg < S.nseg; seg += gridDim.x) {
		const uint32_t n = S.seg_len[seg];
		if (n > Tile::kTile)
			continue;  // k_su_unique_large finishes it
		if (n == 0) {
			if (threadIdx.x == 0)
				pol.finish(seg, 0);
			continue;
		}
		Tile::load(S, seg, 0, n, t);
		Tile::sort(t, n, pow2_at_least(n, Tile::kMinPad));  // <= kTile
		const uint64_t c = Tile::unique_lds(n, seg, pol, t);
		if (threadIdx.x == 0)
			pol.finish(seg, c);
		__syncthreads();  // t is refilled for the next segment
	}
}

// cnt: the counters of a call whose table k_su_register built (an error there
// left a table unwritten: the call fails, nothing reads it); nullptr for a
// host-built table
template <typename Tile>
__global__ __launch_bounds__(kSuThreads) void k_su_tile_sort(SuSegs S, SuTiles T, typename Tile::Key::Word* buf,
                                                             const unsigned long long* cnt)
{
	__shared__ typename Tile::Lds t;
	if (cnt && cnt[kCntError])
		return;
	for (uint64_t b = blockIdx.x; b < T.ntiles; b += gridDim.x) {
		const uint32_t L = T.tile_owner[b];
		const uint32_t len = T.len[L], lo = T.tile_idx[b] * Tile::kTile;
		const uint32_t n = len - lo < Tile::kTile ? len - lo : Tile::kTile;
		Tile::load(S, T.seg ? T.seg[L] : L, lo, n, t);
		Tile::sort(t, n, pow2_at_least(n, Tile::kMinPad));
		Tile::store(t, n, buf + (T.base[L] + lo) * Tile::Key::kWords);
		__syncthreads();  // t is refilled for the next tile
	}
}

// The binary search: the first index in [lo, hi) at which `before` is false
// (true on a prefix of the range, false from there on).
template <typename Index, typename Before>
__device__ __forceinline__ Index su_search(Index lo, Index hi, Before before)
{
	for (uint32_t it = 0; it < kSuSearchSteps && lo < hi; it++) {
		const Index mid = lo + ((hi - lo) >> 1);
		if (before(mid))
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// the first index in [lo, hi) of the sorted keys p whose key is >= x (kUpper: > x)
template <typename Key, bool kUpper>
__device__ __forceinline__ uint64_t su_bound(const typename Key::Word* __restrict__ p, uint64_t lo, uint64_t hi,
                                             const typename Key::T& x)
{
	return su_search(lo, hi, [&](uint64_t mid) {
		const typename Key::T v = Key::get(p, mid);
		return kUpper ? !Key::lt(x, v) : Key::lt(v, x);
	});
}

// one merge pass: sorted runs of w keys -> sorted runs of 2 w keys
template <typename Key, uint32_t kTile>
__global__ __launch_bounds__(kSuThreads) void k_su_merge(SuTiles T, uint64_t w,
                                                         const typename Key::Word* __restrict__ src,
                                                         typename Key::Word* dst, const unsigned long long* cnt)
{
	if (cnt && cnt[kCntError])
		return;
	for (uint64_t b = blockIdx.x; b < T.ntiles; b += gridDim.x) {
		const uint32_t L = T.tile_owner[b];
		const uint64_t len = T.len[L], lo = (uint64_t)T.tile_idx[b] * kTile;
		const uint64_t n = len - lo < kTile ? len - lo : kTile;
		const typename Key::Word* s = src + T.base[L] * Key::kWords;
		typename Key::Word* d = dst + T.base[L] * Key::kWords;
		// a tile lies inside one run (w is a multiple of the tile): uniform per workgroup
		const uint64_t pb = lo / (2 * w) * (2 * w), a1 = std::min(pb + w, len), b1 = std::min(pb + 2 * w, len);
		const bool left = lo < a1;
		for (uint64_t li = lo + threadIdx.x; li < lo + n; li += kSuThreads) {
			const typename Key::T x = Key::get(s, li);
			const uint64_t pos = left ? li + (su_bound<Key, false>(s, a1, b1, x) - a1)
			                          : pb + (li - a1) + (su_bound<Key, true>(s, pb, a1, x) - pb);
			Key::put(d, pos, x);
		}
	}
}

template <typename Tile, typename Pol>
__global__ __launch_bounds__(kSuThreads) void k_su_unique_large(SuTiles T, const typename Tile::Key::Word* __restrict__ buf,
                                                                Pol pol, const unsigned long long* cnt)
{
	if (cnt[kCntError])
		return;
	for (uint64_t L = blockIdx.x; L < T.nlarge; L += gridDim.x) {
		const uint64_t seg = T.seg[L];
		const uint64_t c = Tile::unique_buf(T.len[L], seg, pol, buf + T.base[L] * Tile::Key::kWords);
		if (threadIdx.x == 0)
			pol.finish(seg, c);
		__syncthreads();
	}
}

// off[0..n] = the exclusive prefix sums of v[0..n) (one workgroup)
template <typename V>
__global__ __launch_bounds__(kSuThreads) void k_su_scan(const V* __restrict__ v, uint64_t n, uint64_t* off)
{
	__shared__ uint64_t s_w[kSuThreads / 64];
	const uint32_t w = threadIdx.x >> 6;
	uint64_t run = 0;
	for (uint64_t base = 0; base < n; base += kSuThreads) {
		const uint64_t i = base + threadIdx.x;
		const uint64_t x = i < n ? v[i] : 0;  // (64-bit sums: 256 lengths below 2^31 may pass 2^32)
		const uint64_t incl = wave_incl_scan(x);
		if (lane_id() == 63)
			s_w[w] = incl;
		__syncthreads();
		uint64_t wb = 0, tot = 0;
#pragma unroll
		for (uint32_t k = 0; k < kSuThreads / 64; k++) {
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

// Segment i's off[i + 1] - off[i] results of W elements each, from result
// stage_pos[i * pos_stride] of the staging buffer to result off[i] of the
// output; out_off (if given) = off.
template <typename Elem>
__global__ __launch_bounds__(kSuThreads) void k_su_gather(const Elem* __restrict__ stage,
                                                          const uint64_t* __restrict__ stage_pos, uint64_t pos_stride,
                                                          uint32_t W, const uint64_t* __restrict__ off, uint64_t nseg,
                                                          Elem* out, uint64_t* out_off)
{
	for (uint64_t i = blockIdx.x; i < nseg; i += gridDim.x) {
		const uint64_t a = off[i], n = (off[i + 1] - a) * W;
		const Elem* s = stage + stage_pos[i * pos_stride] * W;
		for (uint64_t x = threadIdx.x; x < n; x += kSuThreads)
			out[a * W + x] = s[x];
		if (out_off && threadIdx.x == 0)
			out_off[i] = a;
	}
	if (out_off && blockIdx.x == 0 && threadIdx.x == 0)
		out_off[nseg] = off[nseg];
}

// The sort-unique of every segment of S (lengths and counts as the prep
// kernel left them in ctx->h_cnt).  Enqueues only.
template <typename Tile, typename Pol>
int su_sort_unique(syzsig_ctx* ctx, const SuSegs& S, const Pol& pol)
{
	using Word = typename Tile::Key::Word;
	const hipStream_t s = ctx->stream;
	const uint64_t nlarge = ctx->h_cnt[kSuLarge], ntiles = ctx->h_cnt[kSuTiles], nkeys = ctx->h_cnt[kSuKeys],
	               maxlen = ctx->h_cnt[kSuMaxLen];
	const size_t key_bytes = sizeof(Word) * Tile::Key::kWords;
	k_su_small<Tile, Pol><<<grid_cap(S.nseg), kSuThreads, 0, s>>>(S, pol);
	if (nlarge) {
		char* tab;
		void *ba, *bb;
		const size_t o_base = align256(nlarge * 8), o_len = o_base + align256(nlarge * 8),
		             o_own = o_len + align256(nlarge * 4), o_idx = o_own + align256(ntiles * 4);
		SYZ_TRY(ws_get(ctx, kWsSuTab, o_idx + align256(ntiles * 4), (void**)&tab));
		SYZ_TRY(ws_get(ctx, kWsSuBufA, nkeys * key_bytes + 256, &ba));
		SYZ_TRY(ws_get(ctx, kWsSuBufB, nkeys * key_bytes + 256, &bb));
		const SuTiles T{(uint64_t*)tab,           (uint64_t*)(tab + o_base), (uint32_t*)(tab + o_len),
		                (uint32_t*)(tab + o_own), (uint32_t*)(tab + o_idx),  nlarge,
		                ntiles};
		k_su_register<Tile::kTile, Tile::kAlign><<<(int)((S.nseg + 255) / 256), 256, 0, s>>>(S.seg_len, S.nseg, nkeys, T,
		                                                                                     ctx->d_cnt);
		Word *src = (Word*)ba, *dst = (Word*)bb;
		k_su_tile_sort<Tile><<<grid_cap(ntiles), kSuThreads, 0, s>>>(S, T, src, ctx->d_cnt);
		for (uint64_t w = Tile::kTile; w < maxlen; w <<= 1) {
			k_su_merge<typename Tile::Key, Tile::kTile><<<grid_cap(ntiles), kSuThreads, 0, s>>>(T, w, src, dst, ctx->d_cnt);
			std::swap(src, dst);
		}
		k_su_unique_large<Tile, Pol><<<grid_cap(nlarge), kSuThreads, 0, s>>>(T, src, pol, ctx->d_cnt);
	}
	SYZ_HIP(hipGetLastError());
	return SYZSIG_OK;
}

// ---- sort-and-walk ----

// One workgroup per element partition p (<= kRpCap entries, keys
// h_residual << 32 | entry index from rp_group).  The keys are sorted in LDS,
// so each element's entries are one run in entry order -- arrival order of
// their owners (polls, inputs), and inside an owner the Serial's order -- and
// one thread per run walks it: tbl[e] (absent, or tbl == nullptr for a nil
// set: below every prio), then each owner's last entry of e (Deserialize: a
// later duplicate wins); wherever the prio exceeds the running maximum,
// event(e, owner, prio) gives the event word.  Read-only on the table.  The
// workgroup's events are gathered in LDS and written to ev (room for ev_cap)
// with one device atomic on *nev.
template <typename Event>
__device__ __forceinline__ void su_sort_walk(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ base,
                                             uint32_t pbits, const uint32_t* __restrict__ rec_owner,
                                             const int8_t* __restrict__ rec_prio, const uint64_t* tbl,
                                             uint64_t tbl_bmask, uint64_t* ev, uint64_t ev_cap,
                                             unsigned long long* nev, const unsigned long long* ctr, Event event)
{
	using Tile = SuWordsTile<1, kRpCap>;
	__shared__ typename Tile::Lds t;
	__shared__ uint64_t out[kRpCap];
	__shared__ uint32_t s_n;
	__shared__ unsigned long long s_base;
	if (ctr[kCntSpill])
		return;  // a partition past kRpCap: the batch takes the sequential path
	const uint32_t p = blockIdx.x, tid = threadIdx.x, b0 = base[p], n = base[p + 1] - b0;
	if (n == 0 || n > kRpCap)
		return;
	const uint64_t* k = t.k[0];
	for (uint32_t i = tid; i < n; i += kSuThreads)
		t.k[0][i] = keys[b0 + i];
	if (tid == 0)
		s_n = 0;
	Tile::sort(t, n, pow2_at_least(n, 1u));
	const uint32_t hp = pbits ? p << (32 - pbits) : 0;
	for (uint32_t i = tid; i < n; i += kSuThreads) {
		const uint32_t hr = (uint32_t)(k[i] >> 32);
		if (i > 0 && (uint32_t)(k[i - 1] >> 32) == hr)
			continue;  // not the head of e's run
		const uint32_t e = fmix32_inv(hp | hr);
		uint64_t v = 0;
		int m = kPrioAbsent;  // (signal.go:79-81)
		if (tbl && tbl_lookup(tbl, tbl_bmask, e, v) >= 0 && slot_live(v))
			m = slot_prio(v);
		uint32_t owner_next = 0;
		for (uint32_t q = i; q < n && (uint32_t)(k[q] >> 32) == hr; q++) {
			const uint32_t r = (uint32_t)k[q], owner = q == i ? rec_owner[r] : owner_next;
			const bool more = q + 1 < n && (uint32_t)(k[q + 1] >> 32) == hr;
			owner_next = more ? rec_owner[(uint32_t)k[q + 1]] : 0;
			if (more && owner_next == owner)
				continue;  // an earlier duplicate inside one Serial
			const int pr = rec_prio[r];
			if (pr > m) {
				out[atomicAdd(&s_n, 1u)] = event(e, owner, pr);
				m = pr;
			}
		}
	}
	__syncthreads();
	const uint32_t ne = s_n;
	if (tid == 0)
		s_base = ne ? atomicAdd(nev, (unsigned long long)ne) : 0;
	__syncthreads();
	for (uint32_t i = tid; i < ne; i += kSuThreads)
		if (s_base + i < ev_cap)  // (at most one event per entry: cannot fail)
			ev[s_base + i] = out[i];
}

#endif  // __HIPCC__

}  // namespace syz
