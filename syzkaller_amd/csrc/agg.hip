// agg.hip -- K3 for large batches: checkNewSignal over a whole batch by
// aggregating the batch's records per element in LDS.
//
// Reference: syz-fuzzer/fuzzer.go:494-511 checkNewSignal, pkg/signal/signal.go
// :90-102 DiffRaw and :117-131 Merge.  With the batch in serial order
// (program-major, call-minor; call k has raw signal sig_k and prio p_k) and
// M0 = maxSignal before the batch:
//
//   e in new_k  <=>  e in sig_k  and  p_k > M0[e]  and  no j < k has e in sig_j with p_j >= p_k
//   M_final[e]  =  max(M0[e], max_k p_k)
//   newSignal  +=  { e : M_final[e] != M0[e] } with prio M_final[e]
//
// Everything about an element e is a function of
//   first[e][l] = min serial k over the records of e at prio level l   (<= 4 levels per run)
// and M0[e]: walking the levels from the top down, a level l with
// val[l] > M0[e] holds a new record iff first[e][l] < min_{l' > l} first[e][l'],
// and that record is (first[e][l], e) -- the call's DiffRaw result.  So the
// batch needs ONE maxSignal probe per distinct element, not one per record.
//
// Record format.  h = fmix32(e) is a bijection of u32.  A run is cut into
// P = 2^pbits partitions by the top pbits of h, and into chunks of 2^cbits
// consecutive calls (cbits = pbits - 2).  Partition p stores its records chunk
// after chunk (one "cell" per (chunk, p)), so a record only needs
//   h's low 32 - pbits bits | level (2 bits) | serial inside its chunk (cbits bits)
// = exactly 32 bits: the partition and the chunk are implied by where the
// record is stored.
//
// Pipeline (one run of <= 4 prio levels):
//   k_agg_count / k_agg_scan_chunks / k_agg_scan_totals / k_agg_scatter
//       records -> 4-B packed records grouped by partition, cells in chunk order
//       (counted cells: sized by a count pass and a scan).
//   k_fast_prep or k_chunk_sizes / k_cell_plan / k_scat3 + k_agg_scatter_blk
//       the same records into capped cells, sized from the chunks' record
//       counts alone (the default; a cell that overflows voids the run, which
//       is redone with counted cells).  Both kernels write whole 64/128-B
//       blocks through ScatBlocks and split the run's work items by how well
//       k_scat3's one-call tiles would be filled (launch_capped_scatter).
//   k_agg       one 1024-thread workgroup per partition: an LDS hash table
//       (residual key + 4 level firsts, 20 B/slot, kAggSlots slots = 145 KiB)
//       absorbs the partition's records -- one ds_read_b128 of the home bucket,
//       a ds_cmpst on first sight, one ds_min per record; then the distinct
//       elements are written out compactly.  A partition with more distinct
//       elements than kAggLimit is flagged and redone by k_agg_global (the same
//       aggregation in an HBM table).
//   k_agg_finalize_x  one workgroup per partition's distinct list: probe/insert
//       maxSignal, emit the new (call, elem) pairs and call flags, write
//       M_final, merge newSignal.  maxSignal's home bucket is the top bits of
//       the same h (internal.h home_bucket), so one partition's probes stay in
//       one contiguous slice of the table, which the workgroup owns for the
//       launch: plain stores, no global atomics.  What leaves its slice goes
//       to k_fin_deferred; k_agg_finalize is the same decision with global
//       atomics, for the HBM fallback's lists and for tables with fewer
//       buckets than partitions.  Capacity is reserved before any of them,
//       so nothing is ever retried.
//   k_pairs_mark (optional) per-record new bits from the pairs.
#include <algorithm>
#include <vector>

#include "decide.h"
#include "internal.h"

namespace syz {

constexpr uint32_t kAggThreads = 1024;
constexpr uint32_t kAggSlots = 7424;               // LDS slots per workgroup (+ 8 KB of first-sight queues)
constexpr uint32_t kAggBW = 4;                     // keys per LDS bucket: one ds_read_b128 per probe
using KBucket = uint4;
constexpr uint32_t kAggBuckets = kAggSlots / kAggBW;
constexpr uint32_t kAggNoSlot = 0xFFFFFFFFu;
static_assert(kAggRegion == kAggSlots, "distinct-list region per partition (internal.h)");
constexpr uint32_t kAggLimit = kAggSlots * 4 / 5;  // distinct elements before a partition overflows
constexpr double kAggTargetLoad = 0.4;             // partitions are sized for this LDS load
constexpr double kAggTargetLoadEntry = 0.6;        // ... and for Minimize
constexpr uint64_t kMinItems = 2048;               // Minimize: at least this many partitioning work items
constexpr uint32_t kAggEmpty = 0xFFFFFFFFu;        // empty key (LDS keys are residuals < 2^29)
constexpr uint32_t kAggOverflow = 0xFFFFFFFFu;     // partition count marker
constexpr uint32_t kAggMinBits = 3, kAggMaxBits = 11;
constexpr uint32_t kAggMaxParts = 1u << kAggMaxBits;
constexpr uint32_t kAggTile = 18432;  // records per scatter tile (18 per lane; 6 B of LDS each)
constexpr uint32_t kAggGroup = 8;  // cells per wave work item of k_agg (<= 64)
// k_agg's record pipeline: U records per lane per batch, D batches in flight ahead
constexpr uint32_t kAggU = 4, kAggD = 2;

// Partition geometry of one run (see the header).
struct AggGeom {
	uint32_t pbits;  // P = 2^pbits partitions
	uint32_t ibits;  // partitioning work items of 2^ibits calls (<= cbits): a chunk is 2^(cbits-ibits) items
	__host__ __device__ uint32_t rbits() const { return 32 - pbits; }
	__host__ __device__ uint32_t cbits() const { return pbits - 2; }
	__host__ __device__ uint32_t items_per_chunk_log2() const { return cbits() - ibits; }
	__host__ __device__ uint32_t part(uint32_t h) const { return h >> (32 - pbits); }
	__host__ __device__ uint32_t meta(uint32_t level, uint64_t serial) const
	{
		return (level << cbits()) | ((uint32_t)serial & ((1u << cbits()) - 1));
	}
	__host__ __device__ uint32_t rec(uint32_t h, uint32_t meta) const { return (h << pbits) | meta; }
	__host__ __device__ uint32_t resid(uint32_t r) const { return r >> pbits; }
	__host__ __device__ uint32_t level(uint32_t r) const { return (r >> cbits()) & 3; }
	__host__ __device__ uint32_t local(uint32_t r) const { return r & ((1u << cbits()) - 1); }
};

// LDS home bucket of a residual: its top bits (h is already mixed)
__device__ __forceinline__ uint32_t agg_home_bucket(uint32_t key, const AggGeom& g)
{
	return __umulhi(key << g.pbits, kAggBuckets);
}

// Workgroup flag in LDS, read and set without `volatile`: a volatile access
// through a generic pointer compiles to a flat access whose vmcnt(0) wait
// drains every global load in flight (the record prefetch).
__device__ __forceinline__ uint32_t lds_flag(uint32_t* f)
{
	return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_flag_set(uint32_t* f)
{
	__hip_atomic_store(f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// position of e in a 4-key bucket, 4 if absent
__device__ __forceinline__ uint32_t bucket_find(uint4 B, uint32_t e)
{
	return B.x == e ? 0 : B.y == e ? 1 : B.z == e ? 2 : B.w == e ? 3 : 4;
}

// position of the first empty key in a 4-key bucket, 4 if full
__device__ __forceinline__ uint32_t bucket_first_empty(uint4 B)
{
	return B.x == kAggEmpty ? 0 : B.y == kAggEmpty ? 1 : B.z == kAggEmpty ? 2 : B.w == kAggEmpty ? 3 : 4;
}

// Find-or-insert e in the LDS key buckets, bucket-linear from its home bucket
// b, whose snapshot B the caller already read.  Keys only go empty -> key, so
// a key is always at or before the first empty slot of its probe sequence:
// an insert is one ds_cmpst at the snapshot's first empty slot, re-reading the
// bucket only when another lane took that slot first.  Returns the slot
// (ins incremented if this call inserted e), or kAggNoSlot if the probe sequence ran
// through the whole table (the partition is then redone in HBM).
__device__ uint32_t agg_find_insert(KBucket* kb, uint32_t e, uint32_t b, KBucket B, uint32_t* s_ovf, uint32_t& ins)
{
	uint32_t* keys = reinterpret_cast<uint32_t*>(kb);
	for (uint32_t step = 0; step < kAggBuckets;) {
		const uint32_t f = bucket_find(B, e);
		if (f < kAggBW)
			return b * kAggBW + f;
		const uint32_t j = bucket_first_empty(B);
		if (j == kAggBW) {
			b = b + 1 == kAggBuckets ? 0 : b + 1;
			B = kb[b];
			step++;
			continue;
		}
		const uint32_t i = b * kAggBW + j;
		const uint32_t key = atomicCAS(&keys[i], kAggEmpty, e);
		if (key == kAggEmpty) {
			ins++;
			return i;
		}
		if (key == e)
			return i;
		B = kb[b];  // another lane filled the slot first
	}
	lds_flag_set(s_ovf);
	return kAggNoSlot;
}

// Cell boundaries of one group of kAggGroup chunks of a partition (uniform
// over the wave: scalar loads), and the serial of a record inside the group.
struct CellGroup {
	uint64_t ch0;
	uint32_t bnd[kAggGroup + 1];
	__device__ void load(const uint32_t* __restrict__ ot, uint64_t nchunks, uint64_t gi)
	{
		ch0 = gi * kAggGroup;
#pragma unroll
		for (uint32_t i = 0; i <= kAggGroup; i++)
			bnd[i] = ot[min<uint64_t>(ch0 + i, nchunks)];
	}
	__device__ uint32_t serial(uint32_t j, uint32_t r, const AggGeom& g) const
	{
		uint32_t chunk = (uint32_t)ch0;
#pragma unroll
		for (uint32_t i = 1; i < kAggGroup; i++)
			chunk += j >= bnd[i];
		return (chunk << g.cbits()) | g.local(r);
	}
};

// ---------------------------------------------------------------- partitioning
// Calls of the run [c0, c1) in work items of 2^ibits; counts[item][p].  kShard:
// only the records whose element shard x.shard of x.nshards owns (owner_of).
template <bool kShard>
__global__ __launch_bounds__(kAggThreads) void k_agg_count(const uint32_t* __restrict__ sigs,
                                                           const uint64_t* __restrict__ call_start,
                                                           const uint32_t* __restrict__ call_len, uint64_t c0,
                                                           uint64_t c1, AggGeom g, AggSrc x, uint32_t* counts)
{
	__shared__ uint32_t h[kAggMaxParts];
	auto add = [&](uint32_t e) {
		if (!kShard || owner_of(e, x.nshards) == x.shard)
			atomicAdd(&h[g.part(fmix32(e))], 1u);
	};
	const uint32_t P = 1u << g.pbits, cb = g.ibits;  // per work item of 2^ibits calls
	const uint32_t w = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = lane_id();
	const uint64_t ncalls = c1 - c0, nchunks = (ncalls + (1ull << cb) - 1) >> cb;
	for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
		for (uint32_t i = threadIdx.x; i < P; i += blockDim.x)
			h[i] = 0;
		__syncthreads();
		const uint64_t ce = min<uint64_t>(ncalls, (ch + 1) << cb);
		for (uint64_t s = (ch << cb) + w; s < ce; s += nw) {
			const uint64_t c = c0 + s, start = call_start[c];
			const uint32_t len = call_len[c];
			uint32_t j = lane;
			for (; j + 192 < len; j += 256) {
				const uint32_t a = sigs[start + j], b = sigs[start + j + 64], d = sigs[start + j + 128],
				               f = sigs[start + j + 192];
				add(a);
				add(b);
				add(d);
				add(f);
			}
			for (; j < len; j += 64)
				add(sigs[start + j]);
		}
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < P; i += blockDim.x)
			counts[ch * P + i] = h[i];
		__syncthreads();
	}
}

// exclusive scan over a 1024-thread block; returns the total
__device__ __forceinline__ uint32_t block_excl_scan_1k(uint32_t v, uint32_t* out)
{
	__shared__ uint32_t wsum[16];
	const uint32_t lane = lane_id(), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
	uint32_t x = v;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t y = __shfl_up(x, o, 64);
		if (lane >= (uint32_t)o)
			x += y;
	}
	if (lane == 63)
		wsum[w] = x;
	__syncthreads();
	uint32_t pre = 0, tot = 0;
	for (uint32_t i = 0; i < nw; i++) {
		pre += i < w ? wsum[i] : 0;
		tot += wsum[i];
	}
	__syncthreads();
	*out = pre + x - v;
	return tot;
}

// block p: exclusive scan over work items of counts[.][p] -> offs[.][p]
// (item-major, for the scatter) and, at every chunk's first item, offsT[p][.]
// (partition-major by chunk, the partition's total at [nchunks], for k_agg);
// totals[p].  An item is 2^ilog items of a chunk (ilog = 0: items are chunks).
__global__ __launch_bounds__(1024) void k_agg_scan_chunks(const uint32_t* counts, uint64_t nitems, uint32_t ilog,
                                                          uint32_t P, uint32_t* offs, uint32_t* offsT, uint64_t* totals)
{
	const uint32_t p = blockIdx.x;
	const uint64_t nchunks = (nitems + (1ull << ilog) - 1) >> ilog;
	uint32_t* ot = offsT + (uint64_t)p * (nchunks + 1);
	uint64_t run = 0;
	for (uint64_t b0 = 0; b0 < nitems; b0 += blockDim.x) {
		const uint64_t b = b0 + threadIdx.x;
		const uint32_t v = b < nitems ? counts[b * P + p] : 0;
		uint32_t ex;
		const uint32_t tot = block_excl_scan_1k(v, &ex);
		if (b < nitems) {
			offs[b * P + p] = (uint32_t)(run + ex);
			if ((b & ((1ull << ilog) - 1)) == 0)
				ot[b >> ilog] = (uint32_t)(run + ex);
		}
		run += tot;
	}
	if (threadIdx.x == 0) {
		totals[p] = run;
		ot[nchunks] = (uint32_t)run;
	}
}

// totals -> rec_base[P + 1] (one block of 1024 threads, P <= 2048: two
// partitions per thread, a wave scan, then the 16 wave sums)
__global__ __launch_bounds__(1024) void k_agg_scan_totals(const uint64_t* totals, uint32_t P, uint64_t* rec_base)
{
	__shared__ uint64_t wsum[16];
	const uint32_t lane = lane_id(), w = threadIdx.x >> 6, i0 = threadIdx.x * 2;
	const uint64_t a = i0 < P ? totals[i0] : 0, b = i0 + 1 < P ? totals[i0 + 1] : 0;
	uint64_t x = a + b;  // inclusive wave scan of the pair sums
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint64_t y = __shfl_up(x, o, 64);
		if (lane >= (uint32_t)o)
			x += y;
	}
	if (lane == 63)
		wsum[w] = x;
	__syncthreads();
	uint64_t pre = 0, tot = 0;
	for (uint32_t k = 0; k < 16; k++) {
		pre += k < w ? wsum[k] : 0;
		tot += wsum[k];
	}
	const uint64_t ex = pre + x - (a + b);
	if (i0 < P)
		rec_base[i0] = ex;
	if (i0 + 1 < P)
		rec_base[i0 + 1] = ex + a;
	if (threadIdx.x == 0)
		rec_base[P] = tot;
}

// ---------------------------------------------------------------- scatter
// Three kernels move a run's records into their cells, every one with
// workgroups of kAggThreads threads that take work items of 2^ibits calls:
//   k_agg_scatter      counted cells (offsets from the scan), a sorted tile
//   k_agg_scatter_blk  capped cells, a wave's tile spans calls
//   k_scat3            capped cells, a wave's tile is a piece of one call
// The two capped scatters write through ScatBlocks and share a run's work
// items between them (CapCells::split).
constexpr uint32_t kScatChunkMax = 1u << (kAggMaxBits - 2);  // calls per chunk (cbits <= 9)
constexpr uint32_t kScatWaves = kAggThreads / 64;

// The capped scatters' tuning (measured alternatives: DESIGN.md section 8).
constexpr uint32_t kScat3K = 16;        // k_scat3: records per lane per tile
constexpr uint32_t kScat3KEntry = 10;   // ... with per-record levels (Minimize: the prios take registers)
constexpr uint32_t kScat3Fill = 85;     // % of its tiles' lanes an item must fill for k_scat3 to take it
constexpr uint32_t kScatPer = 12;       // k_agg_scatter_blk: records per lane per tile
constexpr uint32_t kScatPerEntry = 10;  // ... for Minimize (the prios take registers too)
constexpr uint32_t kBlk = 16;           // records per 64-B block
constexpr uint32_t kDummyLines = 2048;  // CapCells::dummy lines (of 64 B)
typedef uint32_t scat_v4u __attribute__((ext_vector_type(4)));  // a flush lane: 16 B

// Capped cells (the count-free layout of a run):
// chunk c's cells are consecutive regions of cap[c] records (a multiple of 64)
// from base[c], partition after partition; the scatter writes cnt[p][c] and
// raises *ovf when a cell receives more than its capacity (the run is then
// redone with counted cells).
struct CapCells {
	const uint64_t* base;  // [nchunks] first record of chunk c's cells
	const uint32_t* cap;   // [nchunks] records per cell of chunk c
	uint32_t* cnt;         // [P][nchunks] records in cell (c, p)
	uint32_t* ovf;         // set to 1 by a cell overflow
	uint64_t nchunks;
	uint32_t* dummy;       // one 64-B line per block: the target of stores that are not made
	// With split set, k_scat3 takes the work items its one-call tiles would
	// fill (scat3_takes: sizes[] = records, tiles[] = k_scat3 tiles per item)
	// and k_agg_scatter_blk the rest, each skipping the other's items
	const uint64_t* sizes = nullptr;
	const uint32_t* tiles = nullptr;
	bool split = false;
	uint32_t tile = 1024;  // records per k_scat3 tile the tiles[] were counted in (set with tiles)
};

// k_scat3's tiles of one work item (every call in ceil(len / tile) tiles), and
// the split between the two capped scatters: k_scat3 takes an item whose tiles
// would be at least kScat3Fill % full, k_agg_scatter_blk the others.
constexpr uint32_t kScat3Tile = kScat3K * 64, kScat3TileEntry = kScat3KEntry * 64;
__host__ __device__ inline uint64_t scat3_tiles(uint32_t len, uint32_t tile)
{
	return (len + tile - 1) / tile;
}
__device__ inline bool scat3_takes(uint64_t recs, uint32_t tiles, uint32_t tile)
{
	return recs * 100 >= (uint64_t)tiles * tile * kScat3Fill;
}

// Minimize's per-record levels (kEntry): a record's level comes from its own
// prio byte (AggSrc::elem_prio, parallel to sigs) through the run's prio ->
// level table in LDS (an LDS read waits on lgkmcnt, not vmcnt).  kOn = false:
// no table.
template <bool kOn>
struct PrioLevels {
	uint8_t lvl[kOn ? 256 : 1];
	__device__ __forceinline__ void load(const LevelMap& lm, uint32_t nthreads)
	{
		if (kOn) {
			for (uint32_t i = threadIdx.x; i < 256; i += nthreads)
				lvl[i] = lm.lvl[i];
		}
	}
	// the level bits of a record with prio byte pv; bad |= a kept record's prio has no level
	__device__ __forceinline__ uint32_t level(uint32_t pv, bool kept, bool& bad) const
	{
		const uint32_t lv = lvl[kOn ? pv : 0];
		bad |= kept && lv == 0xff;
		return lv & 3;
	}
	// at the kernel's end: report a prio without a level to AggSrc::bad_level
	static __device__ __forceinline__ void report(bool bad, const AggSrc& x)
	{
		if (kOn && x.bad_level && __ballot(bad) && lane_id() == 0)
			atomicOr(x.bad_level, 1u);
	}
};

// The calls of one work item in LDS, and a wave's walk over them in quotas of
// kPer records per lane: wave w takes local calls w, w + kScatWaves, ...
// (k_agg_scatter and k_agg_scatter_blk; k_scat3 walks its calls as scalars).
struct CallTable {
	uint64_t start[kScatChunkMax];
	uint32_t len[kScatChunkMax];
	uint16_t meta[kScatChunkMax];  // AggGeom::meta of the call (level 0 where the records have their own)
	template <bool kEntry>
	__device__ __forceinline__ void load(const uint64_t* __restrict__ call_start, const uint32_t* __restrict__ call_len,
	                                     const uint8_t* __restrict__ call_prio, const LevelMap& lm, const AggGeom& g,
	                                     uint64_t c0, uint64_t cbeg, uint32_t nc)
	{
		for (uint32_t i = threadIdx.x; i < nc; i += blockDim.x) {
			const uint64_t c = c0 + cbeg + i;
			start[i] = call_start[c];
			len[i] = call_len[c];
			meta[i] = (uint16_t)g.meta(kEntry ? 0 : lm.lvl[call_prio[c]], cbeg + i);
		}
	}
	// A record slot's loc = (wave call number j << 24) | offset in the call
	// (calls hold < 2^24 records, batch validation); the wave's j-th call is
	// local call w + j * kScatWaves (j < 2^cbits / kScatWaves <= 32).
	__device__ __forceinline__ uint32_t call_of(uint32_t w, uint32_t loc) const { return w + (loc >> 24) * kScatWaves; }
	// Issue the loads of wave w's next quota from its position (local call wc,
	// offset wo inside it; both advanced): ev[] = elements, loc[] as above,
	// kEntry: pv[] = prio bytes.  Returns how many records the quota has; the
	// slots past them hold a clamped, valid address.
	template <bool kEntry, uint32_t kPer>
	__device__ __forceinline__ uint32_t fetch(uint32_t w, uint32_t lane, uint32_t nc, uint32_t& wc, uint32_t& wo,
	                                          const uint32_t* __restrict__ sigs, const AggSrc& x, uint32_t (&ev)[kPer],
	                                          uint32_t (&loc)[kPer], uint32_t (&pv)[kEntry ? kPer : 1]) const
	{
		constexpr uint32_t kQuota = kPer * 64;
		uint32_t q = 0;
		while (q < kQuota && wc < nc) {
			const uint32_t ln = len[wc], m = min(kQuota - q, ln - wo);
			const uint32_t tag = ((wc - w) / kScatWaves) << 24;
			if (q == 0) {
#pragma unroll
				for (uint32_t u = 0; u < kPer; u++)
					loc[u] = tag | wo;  // clamped default: a valid address
			}
#pragma unroll
			for (uint32_t u = 0; u < kPer; u++) {
				const uint32_t i = u * 64 + lane;
				loc[u] = i >= q && i < q + m ? tag | (wo + i - q) : loc[u];
			}
			q += m;
			wo += m;
			if (wo == ln) {
				wc += kScatWaves;
				wo = 0;
			}
		}
		if (q) {
#pragma unroll
			for (uint32_t u = 0; u < kPer; u++) {
				const uint64_t a = start[call_of(w, loc[u])] + (loc[u] & 0xFFFFFFu);
				ev[u] = __builtin_nontemporal_load(&sigs[a]);
				if (kEntry)
					pv[kEntry ? u : 0] = (uint8_t)__builtin_nontemporal_load(&x.elem_prio[a]);
			}
		}
		return q;
	}
};

// Records of each chunk -> their counted cells (fixed by the scan, so no
// global atomics).  A tile of kAggTile records lives in registers (kPer per
// lane), is counting-sorted by partition into LDS and written out as one run
// per partition; the runs of one chunk's consecutive tiles continue each other.
// The next tile's loads are issued before the write-out of the current one,
// so HBM reads overlap the stores instead of following them.
// kEntry (Minimize): per-record levels (PrioLevels), and only the records
// whose element shard x.shard owns are kept.
template <bool kEntry>
__global__ __launch_bounds__(kAggThreads) void k_agg_scatter(const uint32_t* __restrict__ sigs,
                                                             const uint64_t* __restrict__ call_start,
                                                             const uint32_t* __restrict__ call_len,
                                                             const uint8_t* __restrict__ call_prio, LevelMap lm,
                                                             uint64_t c0, uint64_t c1, AggGeom g, AggSrc x,
                                                             const uint32_t* __restrict__ offs,
                                                             const uint64_t* __restrict__ rec_base, uint32_t* recs)
{
	constexpr uint32_t kQuota = kAggTile / kScatWaves, kPer = kQuota / 64;
	static_assert(kQuota % 64 == 0, "tile quota per wave");
	__shared__ uint32_t t_rec[kAggTile];   // sorted by partition: packed records
	__shared__ uint16_t t_part[kAggTile];  // ... and their partitions
	__shared__ uint64_t cur[kAggMaxParts];
	__shared__ uint32_t hist[kAggMaxParts], pos[kAggMaxParts];
	__shared__ CallTable calls;
	__shared__ PrioLevels<kEntry> levels;
	const uint32_t P = 1u << g.pbits, cb = g.cbits(), ib = g.ibits;
	levels.load(lm, blockDim.x);
	const uint32_t w = threadIdx.x >> 6, lane = lane_id();
	const uint64_t ncalls = c1 - c0, nitems = (ncalls + (1ull << ib) - 1) >> ib;
	const uint32_t per_t = (P + blockDim.x - 1) / blockDim.x;
	bool badlv = false;
	for (uint64_t ch = blockIdx.x; ch < nitems; ch += gridDim.x) {  // ch: work item (of 2^ibits calls)
		const uint64_t cbeg = ch << ib;
		const uint32_t nc = (uint32_t)min<uint64_t>(ncalls - cbeg, 1ull << ib);
		for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) {
			cur[i] = rec_base[i] + offs[ch * P + i];
			hist[i] = 0;
		}
		calls.load<kEntry>(call_start, call_len, call_prio, lm, g, c0, cbeg, nc);
		__syncthreads();
		uint32_t wc = w, wo = 0;  // this wave's walk
		uint32_t ev[kPer], loc[kPer], pv[kEntry ? kPer : 1];
		// (through a lambda: called directly at both sites the kernel takes 11 more VGPRs)
		auto fetch = [&]() { return calls.fetch<kEntry>(w, lane, nc, wc, wo, sigs, x, ev, loc, pv); };
		uint32_t n = fetch();
		for (;;) {
			// stage: partition and rank of every record of the tile (loc = ~0: not kept)
#pragma unroll
			for (uint32_t u = 0; u < kPer; u++) {
				const uint32_t i = u * 64 + lane;
				const bool keep = i < n && (!kEntry || x.nshards == 1 || owner_of(ev[u], x.nshards) == x.shard);
				if (keep) {
					const uint32_t h = fmix32(ev[u]), p = g.part(h);
					const uint32_t r = atomicAdd(&hist[p], 1u);
					uint32_t meta = calls.meta[calls.call_of(w, loc[u])];
					if (kEntry)
						meta |= levels.level(pv[kEntry ? u : 0], true, badlv) << cb;
					ev[u] = g.rec(h, meta);
					loc[u] = p | (r << 16);
				} else {
					loc[u] = ~0u;
				}
			}
			__syncthreads();
			// exclusive scan of hist; pos[p] = the partition's first sorted position
			uint32_t hsum = 0;
			for (uint32_t q = 0; q < per_t; q++) {
				const uint32_t i = threadIdx.x * per_t + q;
				hsum += i < P ? hist[i] : 0;
			}
			uint32_t ex;
			const uint32_t nt = block_excl_scan_1k(hsum, &ex);  // records kept in the tile
			for (uint32_t q = 0; q < per_t; q++) {
				const uint32_t i = threadIdx.x * per_t + q;
				if (i < P) {
					pos[i] = ex;
					cur[i] -= ex;  // cur[p] + d = output index of sorted position d (u64 wrap intended)
					ex += hist[i];
				}
			}
			__syncthreads();
#pragma unroll
			for (uint32_t u = 0; u < kPer; u++) {
				if (loc[u] != ~0u) {
					const uint32_t p = loc[u] & 0xFFFFu, d = pos[p] + (loc[u] >> 16);
					t_rec[d] = ev[u];
					t_part[d] = (uint16_t)p;
				}
			}
			// next tile's loads fly during the write-out
			n = fetch();
			__syncthreads();
			// consecutive threads write consecutive records of one partition's run
			for (uint32_t d = threadIdx.x; d < nt; d += blockDim.x)
				recs[cur[t_part[d]] + d] = t_rec[d];
			__syncthreads();
			for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) {
				cur[i] += pos[i] + hist[i];  // advance by the run
				hist[i] = 0;
			}
			if (!__syncthreads_or(n != 0))
				break;
		}
	}
	PrioLevels<kEntry>::report(badlv, x);
}

// The write-combining blocks of a capped scatter's workgroup.
// A store costs one memory request per 64-B segment it touches, whatever the
// bytes: a ~9-record piece of a cell at an arbitrary offset touches ~1.6
// segments, a whole aligned block one (scripts/mb_scatter.hip: 2.0-2.3 vs
// 3.4-3.8 TB/s read+write).  So every partition has a buffer of one block of
// kB records in LDS: 2048 partitions x 16 records (64 B), or 1024 partitions
// x 32 records (128 B, a whole line) -- 128 KB either way.  A work item is
// scattered in sub-rounds:
//   place   every pending record claims a slot in its partition's block (one
//           ds_add_rtn, all claims of a tile in flight together) and is
//           written there (one ds_write), or, its block being full, stays
//           pending for the next sub-round;
//   wg_or   one barrier, which also tells whether any record is still pending;
//   flush   no list of full blocks is built while placing: each wave scans
//           the counts of its own share of the partitions (partition
//           i * kAggThreads + w * 64 + lane) and writes the full blocks of
//           its share to their cells, 16 B per lane (ds_read_b128,
//           global_store_dwordx4).  A lane group without a block, or whose
//           block no longer fits its cell, stores to the workgroup's dummy
//           line instead (the same instruction count on every path).
// No tile sort, no scan of the tile.  finish() writes each cell's last
// partial block and the cell counts when the work item ends.
struct ScatLane {  // one thread's registers for ScatBlocks
	uint32_t w, lane;      // its wave in the workgroup (uniform) and lane
	uint32_t seq = 0;      // wg_or's row in turn
	bool spilled = false;  // a block or a tail did not fit its cell: the run is redone with counted cells
};
struct ScatItem {  // the cells of the work item being scattered
	uint32_t* recs;
	uint64_t base;  // CapCells::base and cap of the item
	uint32_t cap;
};
template <uint32_t kB>
struct ScatBlocks {
	static_assert(kB == 16 || kB == 32, "block of 64 or 128 B");
	static constexpr uint32_t kMaxP = kB == 16 ? 2048 : 1024;  // partitions
	static_assert(kMaxP * kB * 4 == 128 * 1024 && kMaxP <= kAggMaxParts, "128 KB of blocks");
	static constexpr uint32_t kG = 64 / kB;                   // finish: cells per wave and pass (kB lanes each)
	static constexpr uint32_t kLB = kB / 4, kGF = 64 / kLB;  // flush: 16-B lanes per block, blocks per wave store
	static constexpr uint32_t kShare = (kMaxP + kAggThreads - 1) / kAggThreads;  // partitions per lane in the scan
	alignas(16) uint32_t buf[kMaxP * kB];    // per partition: the block being filled
	uint32_t fillc[kMaxP + 1];               // slots handed out in it (may overshoot kB)
	uint32_t written[kMaxP + 1];             // records of the cell written so far (+ a spare)
	uint16_t flist[kShare * kAggThreads];    // per wave: partitions of its share whose block filled this sub-round
	uint32_t s_or[2][kScatWaves];

	// a new work item (a barrier must follow)
	__device__ __forceinline__ void reset(uint32_t P)
	{
		for (uint32_t i = threadIdx.x; i < P; i += kAggThreads) {
			fillc[i] = 0;
			written[i] = 0;
		}
	}
	// Workgroup OR in one barrier (__syncthreads_or takes three): every wave
	// writes its flag to a row, all read the row (lane i reads wave i's flag);
	// two rows alternate, so a row is rewritten only after every wave passed
	// the barrier of the call between.
	__device__ __forceinline__ bool wg_or(ScatLane& t, bool pred)
	{
		uint32_t* r = s_or[t.seq++ & 1];
		const bool any = __ballot(pred) != 0;
		if (t.lane == 0)
			r[t.w] = any;
		__syncthreads();
		return __ballot(r[t.lane & (kScatWaves - 1)] != 0) != 0;
	}
	// one placement pass over a tile's records rec[] of partitions pt[]: pend
	// = the mask of those to place; returns what is left
	template <uint32_t M>
	__device__ __forceinline__ uint32_t place(const uint32_t (&rec)[M], const uint32_t (&pt)[M], uint32_t pend)
	{
		uint32_t sl[M];
#pragma unroll
		for (uint32_t u = 0; u < M; u++)
			sl[u] = (pend >> u) & 1 ? atomicAdd(&fillc[pt[u]], 1u) : kB;
#pragma unroll
		for (uint32_t u = 0; u < M; u++) {
			if (sl[u] < kB) {
				buf[pt[u] * kB + sl[u]] = rec[u];
				pend &= ~(1u << u);
			}
		}
		return pend;
	}
	// write out the blocks of this wave's share that filled in this sub-round
	__device__ __forceinline__ void flush(ScatLane& t, uint32_t P, const ScatItem& it, uint32_t* dummy)
	{
		const uint32_t fgrp = t.lane / kLB, fq = t.lane % kLB;
		uint16_t* wl = flist + t.w * kShare * 64;  // this wave's list
		uint32_t nw = 0;
#pragma unroll
		for (uint32_t i = 0; i < kShare; i++) {
			const uint32_t p = i * kAggThreads + t.w * 64 + t.lane;
			const bool f = p < P && fillc[p] >= kB;
			const uint64_t m = __ballot(f);
			if (f)
				wl[nw + lane_rank(m)] = (uint16_t)p;
			nw += (uint32_t)__popcll(m);
		}
		// (the wave's LDS operations run in order: the list is read below as written)
		for (uint32_t jb = 0; jb < nw; jb += kGF) {
			const bool ok = jb + fgrp < nw;
			const uint32_t pp = wl[min(jb + fgrp, nw - 1)];
			const uint32_t wr = written[pp];
			const scat_v4u v = *reinterpret_cast<const scat_v4u*>(&buf[pp * kB + fq * 4]);
			const bool fits = wr + kB <= it.cap;
			t.spilled |= ok && !fits;
			uint32_t* d = ok && fits ? it.recs + it.base + (uint64_t)pp * it.cap + wr
			                         : dummy + (blockIdx.x % (kDummyLines * kBlk / kB)) * kB;
			*reinterpret_cast<scat_v4u*>(d + fq * 4) = v;
			__builtin_amdgcn_wave_barrier();
			if (fq == 0 && ok) {
				written[pp] = wr + kB;
				fillc[pp] = 0;
			}
		}
	}
	// one tile: place in sub-rounds until every record is in a block
	template <uint32_t M>
	__device__ __forceinline__ void scatter_tile(ScatLane& t, uint32_t P, const ScatItem& it, uint32_t* dummy,
	                                             const uint32_t (&rec)[M], const uint32_t (&pt)[M], uint32_t pend)
	{
		for (;;) {
			pend = place(rec, pt, pend);
			const bool more = wg_or(t, pend != 0);
			flush(t, P, it, dummy);
			if (!more)
				break;
			__syncthreads();
		}
	}
	// The end of work item ch: every cell's last partial block and its count,
	// and the run's spill flag; ends with the barrier before the next reset.
	// The flag is raised here, at the end of the item that spilled, not once at
	// the kernel's end, on purpose: it keeps the flag's address out of what a
	// later store after the item loop would hold live (measured: fewer SGPR
	// spills).  The run is void either way; a workgroup
	// of the same launch that starts late may see the flag and return at once.
	__device__ __forceinline__ void finish(ScatLane& t, uint32_t P, const ScatItem& it, const CapCells& cc, uint64_t ch)
	{
		const uint32_t grp = t.lane / kB, slot = t.lane & (kB - 1);
		for (uint32_t p = t.w * kG + grp; p < P; p += kScatWaves * kG) {
			const uint32_t c = fillc[p], wr = written[p];
			if (wr + c > it.cap)
				t.spilled = true;
			else if (slot < c)
				it.recs[it.base + (uint64_t)p * it.cap + wr + slot] = buf[p * kB + slot];
			if (slot == 0)
				cc.cnt[(uint64_t)p * cc.nchunks + ch] = min(wr + c, it.cap);
		}
		if (t.spilled)
			*cc.ovf = 1u;
		__syncthreads();
	}
};

// Capped cells, a wave's tile of kPer records per lane walks the item's calls
// through the CallTable: it is full whatever the calls' lengths, at the price
// of per-record call bookkeeping (loc, an LDS lookup of the call's start and
// meta).  Takes the work items k_scat3 leaves (cc.split), or all of them.
// kEntry (Minimize): per-record levels (PrioLevels), and only the records
// whose element shard x.shard owns are kept.
template <bool kEntry, uint32_t kB>
__global__ __launch_bounds__(kAggThreads, 4) void k_agg_scatter_blk(const uint32_t* __restrict__ sigs,
                                                                    const uint64_t* __restrict__ call_start,
                                                                    const uint32_t* __restrict__ call_len,
                                                                    const uint8_t* __restrict__ call_prio, LevelMap lm,
                                                                    uint64_t c0, uint64_t c1, AggGeom g, AggSrc x,
                                                                    CapCells cc, uint32_t* recs)
{
	constexpr uint32_t kPer = kEntry ? kScatPerEntry : kScatPer;
	__shared__ ScatBlocks<kB> blocks;
	__shared__ CallTable calls;
	__shared__ PrioLevels<kEntry> levels;
	const uint32_t P = 1u << g.pbits, cb = g.cbits(), ib = g.ibits;
	ScatLane t{threadIdx.x >> 6, lane_id()};
	const uint32_t w = t.w, lane = t.lane;
	const uint64_t ncalls = c1 - c0, nchunks = (ncalls + (1ull << ib) - 1) >> ib;  // work items
	if (*cc.ovf)
		return;  // the run is already void (an optimistic run's assumptions failed, or a cell spilled)
	bool badlv = false;
	levels.load(lm, blockDim.x);
	for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
		const uint64_t cbeg = ch << ib;
		const uint32_t nc = (uint32_t)min<uint64_t>(ncalls - cbeg, 1ull << ib);
		if (cc.split && scat3_takes(cc.sizes[ch], cc.tiles[ch], cc.tile))
			continue;  // long calls: k_scat3's item
		const ScatItem it{recs, cc.base[ch], cc.cap[ch]};
		blocks.reset(P);
		calls.load<kEntry>(call_start, call_len, call_prio, lm, g, c0, cbeg, nc);
		__syncthreads();
		uint32_t wc = w, wo = 0;  // this wave's walk
		uint32_t ev[kPer], loc[kPer], pv[kEntry ? kPer : 1];
		uint32_t n = calls.fetch<kEntry>(w, lane, nc, wc, wo, sigs, x, ev, loc, pv);
		for (;;) {
			// the tile's packed records and partitions, and the mask of those to place
			uint32_t rec[kPer], pt[kPer], pend = 0;
#pragma unroll
			for (uint32_t u = 0; u < kPer; u++) {
				const uint32_t h = fmix32(ev[u]);
				pt[u] = g.part(h);
				uint32_t meta = calls.meta[calls.call_of(w, loc[u])];
				const bool keep = !kEntry || x.nshards == 1 || owner_of(ev[u], x.nshards) == x.shard;
				if (kEntry)
					meta |= levels.level(pv[kEntry ? u : 0], u * 64 + lane < n && keep, badlv) << cb;
				rec[u] = g.rec(h, meta);
				pend |= (uint32_t)(u * 64 + lane < n && keep) << u;
			}
			n = calls.fetch<kEntry>(w, lane, nc, wc, wo, sigs, x, ev, loc, pv);  // the next tile's loads fly while this one is placed
			blocks.scatter_tile(t, P, it, cc.dummy, rec, pt, pend);
			if (!blocks.wg_or(t, n != 0))  // (its barrier also ends the last flush)
				break;
		}
		blocks.finish(t, P, it, cc, ch);
	}
	PrioLevels<kEntry>::report(badlv, x);
}

// Capped cells, the lean scatter: the per-record bookkeeping of the loads is
// taken out.  A wave walks whole calls (calls w, w + kScatWaves, .. of its
// work item) in tiles of up to kK * 64 records of ONE call: the tile's start,
// level and serial are wave-uniform scalars (s_load of the call, no LDS call
// table), and the pending mask comes from the record count, so a record costs
// its load, fmix32, one ds_add_rtn and one ds_write.  A call a little longer
// than a tile leaves lanes idle: with cc.split the kernel takes only the work
// items whose tiles it would fill (scat3_takes).
// kEntry (Minimize, one shard): per-record levels (PrioLevels).
template <uint32_t kK, bool kEntry, uint32_t kB>
__global__ __launch_bounds__(kAggThreads, 4) void k_scat3(const uint32_t* __restrict__ sigs,
                                                          const uint64_t* __restrict__ call_start,
                                                          const uint32_t* __restrict__ call_len,
                                                          const uint8_t* __restrict__ call_prio, LevelMap lm,
                                                          uint64_t c0, uint64_t c1, AggGeom g, CapCells cc,
                                                          uint32_t* recs, AggSrc x)
{
	constexpr uint32_t kTile = kK * 64;
	static_assert(kK <= 31, "pending masks are 32-bit");
	__shared__ ScatBlocks<kB> blocks;
	__shared__ PrioLevels<true> levels;  // (also the calls' levels: an LDS read)
	const uint32_t P = 1u << g.pbits;
	// (w through readfirstlane: the compiler then knows the call walk is
	// wave-uniform and reads the calls with scalar loads, which wait on
	// lgkmcnt -- a vector load there would need vmcnt(0), draining the
	// prefetch and the block stores)
	ScatLane t{(uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane_id()};
	const uint32_t w = t.w, lane = t.lane;
	const uint64_t ncalls = c1 - c0, nchunks = (ncalls + (1ull << g.ibits) - 1) >> g.ibits;
	if (*cc.ovf)
		return;  // the run is already void
	bool badlv = false;
	levels.load(lm, kAggThreads);
	for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {  // work items
		const uint64_t cbeg = ch << g.ibits;
		const uint32_t nc = (uint32_t)min<uint64_t>(ncalls - cbeg, 1ull << g.ibits);
		if (cc.split && !scat3_takes(cc.sizes[ch], cc.tiles[ch], cc.tile))
			continue;  // short calls: k_agg_scatter_blk's item
		const ScatItem it{recs, cc.base[ch], cc.cap[ch]};
		blocks.reset(P);
		__syncthreads();
		// this wave's call walk (wave-uniform): call j of the chunk, offset wo
		uint32_t j = w, wo = 0, clen = 0, cmeta = 0;
		uint64_t cstart = 0;
		auto open_call = [&]() {
			while (j < nc) {
				const uint64_t c = c0 + cbeg + j;
				clen = call_len[c];
				if (clen) {
					cstart = call_start[c];
					// the prio byte through a scalar dword load of its aligned word
					// (a byte load would be a vector load, waited for with vmcnt(0))
					const uintptr_t pa = (uintptr_t)(call_prio + c);
					const uint32_t word =
					    *(const __attribute__((address_space(4))) uint32_t*)(pa & ~(uintptr_t)3);  // (constant: s_load)
					cmeta = g.meta(kEntry ? 0 : levels.lvl[(word >> (8 * (pa & 3))) & 0xFF], cbeg + j);
					return;
				}
				j += kScatWaves;
			}
		};
		open_call();
		// the next tile's loads: v[] and its scalars (records n, meta); n = 0: none
		auto fetch = [&](uint32_t (&v)[kK], uint32_t (&pv)[kEntry ? kK : 1], uint32_t& n, uint32_t& meta) {
			n = j < nc ? min(kTile, clen - wo) : 0u;
			meta = cmeta;
			const uint32_t* src = sigs + cstart + wo;
			const uint32_t last = n ? n - 1 : 0;
#pragma unroll
			for (uint32_t u = 0; u < kK; u++)
				v[u] = __builtin_nontemporal_load(&src[min(u * 64 + lane, last)]);
			if constexpr (kEntry) {
				const int8_t* psrc = x.elem_prio + cstart + wo;
#pragma unroll
				for (uint32_t u = 0; u < kK; u++)
					pv[u] = (uint8_t)__builtin_nontemporal_load(&psrc[min(u * 64 + lane, last)]);
			}
			if (n) {
				wo += n;
				if (wo == clen) {
					wo = 0;
					j += kScatWaves;
					open_call();
				}
			}
		};
		// one tile: pack its records, then place them
		auto tile = [&](const uint32_t (&v)[kK], const uint32_t (&pv)[kEntry ? kK : 1], uint32_t n, uint32_t meta) {
			uint32_t rec[kK], pt[kK];
#pragma unroll
			for (uint32_t u = 0; u < kK; u++) {
				const uint32_t h = fmix32(v[u]);
				pt[u] = g.part(h);
				uint32_t m = meta;
				if constexpr (kEntry)
					m |= levels.level(pv[kEntry ? u : 0], u * 64 + lane < n, badlv) << g.cbits();
				rec[u] = g.rec(h, m);
			}
			// records u * 64 + lane < n: the lane's first nu (a mask, not a compare per record)
			const uint32_t nu = n > lane ? (n - lane + 63) >> 6 : 0u;  // (<= kK <= 31)
			blocks.scatter_tile(t, P, it, cc.dummy, rec, pt, (1u << nu) - 1);
		};
		// two register buffers in turn (static indices: the prefetch lands
		// where it is consumed, no moves that would wait for it)
		uint32_t va[kK], vb[kK], pa[kEntry ? kK : 1], pb[kEntry ? kK : 1], na, nb, ma, mb;
		fetch(va, pa, na, ma);
		for (;;) {
			fetch(vb, pb, nb, mb);
			tile(va, pa, na, ma);
			if (!blocks.wg_or(t, nb != 0))  // (its barrier also ends the last flush)
				break;
			fetch(va, pa, na, ma);
			tile(vb, pb, nb, mb);
			if (!blocks.wg_or(t, na != 0))
				break;
		}
		blocks.finish(t, P, it, cc, ch);
	}
	PrioLevels<kEntry>::report(badlv, x);
}

static uint64_t nchunks_of(uint64_t ncalls, uint32_t ibits)
{
	return (ncalls + (1ull << ibits) - 1) >> ibits;
}

// The capped-cell scatter of one run: which kernels, and the block width.
// xp: Minimize's per-record extras (nullptr: a triage run).
//   k_scat3 plus split: a triage run, or a Minimize run of one shard (its
//       contexts come in rank order, Len desc, so the heavy first work items
//       fill k_scat3's one-call tiles).  k_scat3's tiles hold one call's
//       records, so the items whose tiles would be less than kScat3Fill % full
//       go to k_agg_scatter_blk, decided per item on the device: both kernels
//       are launched, each skips the other's items.
//   k_agg_scatter_blk alone: a sharded Minimize part (the owner filter).
// Blocks are 128 B at <= 1024 partitions (the same 128 KB of LDS), else 64 B;
// a triage run's k_scat3 keeps 64-B blocks.
static void launch_capped_scatter(hipStream_t s, const syzsig_batch* b, uint64_t c0, uint64_t c1, const LevelMap& lm,
                                  const AggGeom& g, CapCells cc, uint32_t* recs, const AggSrc* xp)
{
	const uint32_t grid = (uint32_t)std::min<uint64_t>(cc.nchunks, 2048);
	const bool wide = g.pbits < kAggMaxBits;
	const AggSrc x = xp ? *xp : AggSrc{nullptr, 1, 0, 0};
	auto launch = [&](auto kernel, auto... tail) {
		kernel<<<grid, kAggThreads, 0, s>>>(b->sigs, b->call_start, b->call_len, b->call_prio, lm, c0, c1, g, tail...);
	};
	if (!xp || xp->nshards == 1) {
		cc.split = xp || (cc.sizes && cc.tiles);
		if (!xp)
			launch(k_scat3<kScat3K, false, 16>, cc, recs, x);
		else if (wide)
			launch(k_scat3<kScat3KEntry, true, 32>, cc, recs, x);
		else
			launch(k_scat3<kScat3KEntry, true, 16>, cc, recs, x);
		if (!cc.split)
			return;
	}
	if (xp)
		launch(wide ? k_agg_scatter_blk<true, 32> : k_agg_scatter_blk<true, 16>, x, cc, recs);
	else
		launch(wide ? k_agg_scatter_blk<false, 32> : k_agg_scatter_blk<false, 16>, x, cc, recs);
}

// Capped cells of a run: records per chunk -> cell capacity and chunk base.
// cap = m + sd * sqrt(m) + 64 rounded up to 64, m = the chunk's records / P
// (the cells of a uniformly hashed chunk hold m +- sqrt(m)); the host reserves
// 1.25 * records + nchunks * P * (sd^2 + 128), an upper bound of the sum
// (sd * sqrt(m) <= m / 4 + sd^2).
__global__ __launch_bounds__(256) void k_chunk_sizes(const uint32_t* __restrict__ call_len, uint64_t c0, uint64_t c1,
                                                     uint32_t cbits, uint64_t* sizes, uint32_t* tiles, uint32_t tile)
{
	const uint64_t ch = blockIdx.x, cbeg = c0 + (ch << cbits), cend = min<uint64_t>(c1, cbeg + (1ull << cbits));
	uint64_t s = 0, t = 0;
	for (uint64_t c = cbeg + threadIdx.x; c < cend; c += blockDim.x) {
		s += call_len[c];
		t += scat3_tiles(call_len[c], tile);
	}
	s = wave_sum_u64(s);
	t = wave_sum_u64(t);
	__shared__ uint64_t ws[4][2];
	if (lane_id() == 0) {
		ws[threadIdx.x >> 6][0] = s;
		ws[threadIdx.x >> 6][1] = t;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		sizes[ch] = ws[0][0] + ws[1][0] + ws[2][0] + ws[3][0];
		if (tiles)
			tiles[ch] = (uint32_t)min<uint64_t>(ws[0][1] + ws[1][1] + ws[2][1] + ws[3][1], 0xFFFFFFFFu);
	}
}

__device__ __forceinline__ void cell_plan(const uint64_t* __restrict__ sizes, uint64_t nchunks, uint32_t P, float sd,
                                          uint64_t* base, uint32_t* cap)
{
	__shared__ uint64_t wsum[16];
	uint64_t run = 0;
	for (uint64_t b0 = 0; b0 < nchunks; b0 += blockDim.x) {
		const uint64_t c = b0 + threadIdx.x;
		uint64_t v = 0;
		if (c < nchunks) {
			const float m = (float)sizes[c] / (float)P;
			const uint32_t k = sd < 0 ? 64u : ((uint32_t)(m + sd * sqrtf(m)) + 64 + 63) & ~63u;  // sd < 0: tests
			cap[c] = k;
			v = (uint64_t)k * P;
		}
		// exclusive block scan of v
		uint64_t xs = v;
		const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const uint64_t y = __shfl_up(xs, o, 64);
			if (lane >= (uint32_t)o)
				xs += y;
		}
		if (lane == 63)
			wsum[w] = xs;
		__syncthreads();
		uint64_t pre = 0, tot = 0;
		for (uint32_t i = 0; i < 16; i++) {
			pre += i < w ? wsum[i] : 0;
			tot += wsum[i];
		}
		if (c < nchunks)
			base[c] = run + pre + xs - v;
		run += tot;
		__syncthreads();
	}
}

__global__ __launch_bounds__(1024) void k_cell_plan(const uint64_t* __restrict__ sizes, uint64_t nchunks, uint32_t P,
                                                    float sd, uint64_t* base, uint32_t* cap)
{
	cell_plan(sizes, nchunks, P, sd, base, cap);
}

// The one-sync triage run's first pass, one block per chunk of calls: the
// chunk's records (for k_cell_plan_fast), call ranges checked, whether a
// prio outside the run's levels (0..3 for a triage run) occurs, and call_new
// zeroed.  part[2 ch] = records,
// part[2 ch + 1] = bad ranges | other prio << 63.
__global__ __launch_bounds__(256) void k_fast_prep(const uint64_t* __restrict__ call_start,
                                                   const uint32_t* __restrict__ call_len,
                                                   const uint8_t* __restrict__ call_prio, uint64_t c0, uint64_t c1,
                                                   uint32_t ibits, uint64_t nrec_space, uint64_t* sizes,
                                                   uint64_t* part, uint8_t* call_new, LevelMap lm, uint32_t* tiles)
{
	const uint64_t ch = blockIdx.x, cbeg = c0 + (ch << ibits), cend = min<uint64_t>(c1, cbeg + (1ull << ibits));
	uint64_t tot = 0, bad = 0, other = 0, nt = 0;
	for (uint64_t c = cbeg + threadIdx.x; c < cend; c += blockDim.x) {
		const uint64_t st = call_start[c];
		const uint32_t ln = call_len[c];
		tot += ln;
		nt += scat3_tiles(ln, kScat3Tile);
		bad += st > nrec_space || ln > nrec_space - st || ln > kSerialMask;
		other |= lm.lvl[call_prio[c]] == 0xff;
		call_new[c] = 0;
	}
	tot = wave_sum_u64(tot);
	bad = wave_sum_u64(bad);
	other = wave_sum_u64(other);
	nt = wave_sum_u64(nt);
	__shared__ uint64_t ws[4][4];
	if (lane_id() == 0) {
		ws[threadIdx.x >> 6][0] = tot;
		ws[threadIdx.x >> 6][1] = bad;
		ws[threadIdx.x >> 6][2] = other;
		ws[threadIdx.x >> 6][3] = nt;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t t = 0, b = 0, o = 0, tl = 0;
		for (int w = 0; w < 4; w++) {
			t += ws[w][0];
			b += ws[w][1];
			o += ws[w][2];
			tl += ws[w][3];
		}
		sizes[ch] = t;
		if (tiles)
			tiles[ch] = (uint32_t)min<uint64_t>(tl, 0xFFFFFFFFu);
		part[2 * ch] = t;
		part[2 * ch + 1] = b | (o ? 1ull << 63 : 0);
	}
}

// k_cell_plan for the one-sync run: the counters are zeroed here (npairs
// preset), the assumptions checked from k_fast_prep's partials -- prios in
// 0..3 (else flag 2), valid ranges and at most `guess` records (else flag 4)
// -- and the run's void flag (ctr[kCntSpill]) set before anything reads it.
__global__ __launch_bounds__(1024) void k_cell_plan_fast(const uint64_t* __restrict__ sizes, uint64_t nchunks,
                                                         uint32_t P, float sd, uint64_t* base, uint32_t* cap,
                                                         const uint64_t* __restrict__ part, uint64_t guess,
                                                         uint64_t npairs0, unsigned long long* ctr)
{
	__shared__ unsigned long long s_tot, s_flag;
	if (threadIdx.x == 0) {
		s_tot = 0;
		s_flag = 0;
	}
	if (threadIdx.x < kNumCounters)
		ctr[threadIdx.x] = threadIdx.x == kCntAux2 ? npairs0 : 0;
	__syncthreads();
	uint64_t t = 0, f = 0;
	for (uint64_t c = threadIdx.x; c < nchunks; c += blockDim.x) {
		t += part[2 * c];
		f |= part[2 * c + 1];
	}
	t = wave_sum_u64(t);
	for (int o = 32; o > 0; o >>= 1)
		f |= __shfl_xor(f, o, 64);
	if (lane_id() == 0) {
		atomicAdd(&s_tot, (unsigned long long)t);
		atomicOr(&s_flag, (unsigned long long)f);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		ctr[kCntRecords] = s_tot;
		// 2: a prio outside the levels; 4: a bad call range or more records than
		// `guess` (the caller's exact path validates and sizes those)
		ctr[kCntSpill] = (s_flag >> 63 ? 2u : 0u) | ((s_flag & ~(1ull << 63)) || s_tot > guess ? 4u : 0u);
	}
	cell_plan(sizes, nchunks, P, sd, base, cap);
}

// ---------------------------------------------------------------- aggregation
// One workgroup per aggregation partition.  Waves take groups of gsz
// cells (chunks) from an LDS counter and walk each group as one virtual run.
// Cell (c, p): counted layout, the partition's records from rec_base[p] with
// cell offsets offsT[p][.]; capped layout (kCap), cap[c] records from
// base[c] + p * cap[c] of which cnt[p][c] are written.  Output: the
// partition's distinct elements and their level firsts at
// dist_*[p * kAggRegion ...], cnt[p] = how many, or kAggOverflow when they do
// not fit the LDS table.
// U records per lane per batch, D batches in flight ahead of the one absorbed.
// The LDS of one aggregation workgroup: keys (residuals) in 4-slot buckets,
// the level firsts, and per wave the records whose element was not in its
// home bucket (first sight, or a probe chain), gathered across batches and
// resolved 64 at a time with every lane busy: (residual, level << 24 | serial).
struct AggLds {
	KBucket kb[kAggBuckets];
	uint32_t fl[4][kAggSlots];
	uint2 q[kAggThreads / 64][64];
	uint32_t s_n, s_ovf, s_out, s_next;
};

// Where the records of one partition are (see k_agg).
struct AggCells {
	const uint32_t* recs;
	const uint64_t* rec_base;  // counted layout
	const uint32_t* offsT;
	const uint64_t* cap_base;  // capped layout
	const uint32_t* cap_len;
	const uint32_t* cap_cnt;
	uint64_t nchunks;
	uint32_t ilog, gsz;
	const uint32_t* spill;  // nonzero: a cell spilled, the run is redone (nothing aggregated); may be null
	unsigned long long* ctr;  // if set: distinct elements (kCntDistinct) and overflowed partitions (kCntAggOvf)
};

// Aggregate partition p into the LDS table (every thread of the workgroup;
// ends with a barrier).  Returns false when its distinct elements overflow
// the table (s_ovf).
template <uint32_t U, uint32_t D, bool kCap, bool kIdx32>
__device__ __forceinline__ bool agg_partition(AggLds& L, uint32_t p, const AggCells& x, const AggGeom& g)
{
	KBucket* kb = L.kb;
	auto& fl = L.fl;
	const uint32_t* __restrict__ recs = x.recs;
	const uint64_t* __restrict__ rec_base = x.rec_base;
	const uint32_t* __restrict__ offsT = x.offsT;
	const uint64_t* __restrict__ cap_base = x.cap_base;
	const uint32_t* __restrict__ cap_len = x.cap_len;
	const uint32_t* __restrict__ cap_cnt = x.cap_cnt;
	const uint64_t nchunks = x.nchunks;
	const uint32_t ilog = x.ilog, gsz = x.gsz;
	const uint32_t lane = lane_id();
	uint2* wq = L.q[threadIdx.x >> 6];
	uint32_t qn = 0;  // entries in this wave's queue (uniform)
	// resolve the queue: find-or-insert each element, then its level first
	auto flush_queue = [&]() {
		uint32_t ins = 0;
		if (lds_flag(&L.s_ovf)) {  // overflowed: the partition is redone, skip the probes
			qn = 0;
			return;
		}
		if (lane < qn) {
			const uint2 e = wq[lane];
			const uint32_t hb = __umulhi(e.x << g.pbits, kAggBuckets);
			const uint32_t slot = agg_find_insert(kb, e.x, hb, kb[hb], &L.s_ovf, ins);
			if (slot != kAggNoSlot)
				atomicMin(&fl[e.y >> 24][slot], e.y & 0xFFFFFFu);
		}
		// inserts counted per flush (overflow = more than kAggLimit distinct)
		const uint32_t n_ins = (uint32_t)wave_sum_u64(ins);
		if (n_ins && lane == 0 && atomicAdd(&L.s_n, n_ins) + n_ins > kAggLimit)
			lds_flag_set(&L.s_ovf);
		qn = 0;
		__builtin_amdgcn_wave_barrier();
	};
	const uint64_t ngroups = (nchunks + gsz - 1) / gsz;
	for (uint32_t i = threadIdx.x; i < kAggSlots; i += blockDim.x) {
		if (i < kAggSlots)
			reinterpret_cast<uint32_t*>(kb)[i] = kAggEmpty;
		fl[0][i] = fl[1][i] = fl[2][i] = fl[3][i] = kNoFirst;
	}
	if (threadIdx.x == 0) {
		L.s_n = 0;
		L.s_ovf = 0;
		L.s_out = 0;
		L.s_next = 0;
	}
	__syncthreads();
	const uint32_t* ot = offsT + (uint64_t)p * (nchunks + 1);
	// no barrier inside: a wave leaves early once overflow is flagged
	for (;;) {
		uint32_t gi = 0;
		if (lane == 0)
			gi = atomicAdd(&L.s_next, 1u);
		gi = __builtin_amdgcn_readfirstlane(__shfl(gi, 0, 64));
		if (gi >= ngroups || lds_flag(&L.s_ovf))
			break;
		// the group's cells, one per lane 0..gsz-1: first record and
		// records.  The group is walked as one virtual run, cell after cell:
		// virtual offset v of cell i is record recs[v + delta_i].
		const uint64_t ch0 = (uint64_t)gi * gsz;
		uint64_t lbase = 0;
		uint32_t llen = 0;
		{
			const uint64_t c = ch0 + lane;
			if (lane < gsz && c < nchunks) {
				if (kCap) {
					lbase = cap_base[c] + (uint64_t)p * cap_len[c];
					llen = cap_cnt[(uint64_t)p * nchunks + c];
				} else {
					lbase = rec_base[p] + ot[c];
					llen = ot[c + 1] - ot[c];
				}
			}
		}
		uint32_t lvs = llen;  // inclusive scan over lanes 0..gsz-1, then exclusive
#pragma unroll
		for (uint32_t o = 1; o < 64; o <<= 1) {
			if (o < gsz) {
				const uint32_t y = __shfl_up(lvs, o, 64);
				if (lane >= o)
					lvs += y;
			}
		}
		const uint32_t n = __builtin_amdgcn_readlane(lvs, gsz - 1);
		if (n == 0)
			continue;
		lvs -= llen;
		const uint64_t ldelta = lbase - lvs;
		const uint32_t nl = n - 1;
		// Per batch [o0, o0 + U * 64): the cell of o0 (the last cell starting
		// at or before it: a non-empty one, as an empty cell shares its
		// successor's start) and the cells starting inside the batch.
		auto cells = [&](uint32_t o0, uint32_t& c0, uint64_t& inside) {
			c0 = (uint32_t)__popcll(__ballot(lane < gsz && lvs <= o0)) - 1;
			inside = __ballot(lane < gsz && lvs > o0 && lvs < o0 + U * 64);
		};
		auto delta_of = [&](uint32_t i) -> uint64_t {
			const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)ldelta, i);
			const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(ldelta >> 32), i);
			return (uint64_t)hi << 32 | lo;
		};
		// Records stream through registers one batch ahead of the LDS work,
		// ping-ponging between register buffers.  Loads are unconditional:
		// lanes past the group re-read its last record -- a second copy of a
		// record changes nothing (min is idempotent), so no lane needs a
		// validity test.
		auto fetch = [&](uint32_t (&buf)[U], uint32_t o0) {
			uint32_t c0;
			uint64_t inside;
			cells(min(o0, nl), c0, inside);  // a prefetch past the group reads its last record
			if constexpr (kIdx32) {
				// every cell lies below record 2^32 (host-checked): 32-bit record
				// indices, the cell deltas taken mod 2^32 (v + delta is the index)
				const uint32_t d0 = __builtin_amdgcn_readlane((uint32_t)ldelta, c0);
				uint32_t v[U], d[U];
#pragma unroll
				for (uint32_t u = 0; u < U; u++) {
					v[u] = min(o0 + u * 64 + lane, nl);
					d[u] = d0;
				}
				for (uint64_t m = inside; m; m &= m - 1) {
					const uint32_t j = __builtin_ctzll(m), vs = __builtin_amdgcn_readlane(lvs, j);
					const uint32_t dj = __builtin_amdgcn_readlane((uint32_t)ldelta, j);
#pragma unroll
					for (uint32_t u = 0; u < U; u++)
						d[u] = v[u] >= vs ? dj : d[u];
				}
#pragma unroll
				for (uint32_t u = 0; u < U; u++)
					buf[u] = __builtin_nontemporal_load(&recs[v[u] + d[u]]);
				return;
			}
			const uint64_t d0 = delta_of(c0);
			uint32_t v[U];
			uint64_t d[U];
#pragma unroll
			for (uint32_t u = 0; u < U; u++) {
				v[u] = min(o0 + u * 64 + lane, nl);
				d[u] = d0;
			}
			for (uint64_t m = inside; m; m &= m - 1) {
				const uint32_t j = __builtin_ctzll(m), vs = __builtin_amdgcn_readlane(lvs, j);
				const uint64_t dj = delta_of(j);
#pragma unroll
				for (uint32_t u = 0; u < U; u++)
					d[u] = v[u] >= vs ? dj : d[u];
			}
#pragma unroll
			for (uint32_t u = 0; u < U; u++)
				buf[u] = __builtin_nontemporal_load(&recs[v[u] + d[u]]);
		};
		auto absorb = [&](const uint32_t (&buf)[U], uint32_t o0) {
			uint32_t c0;
			uint64_t inside;
			cells(o0, c0, inside);
			uint32_t key[U], lv[U], k[U], hb[U], slot[U], c[U];
#pragma unroll
			for (uint32_t u = 0; u < U; u++)
				c[u] = (uint32_t)ch0 + c0;
			// a uniform loop over the (0-2 typically) cells starting inside the batch
			for (uint64_t m = inside; m; m &= m - 1) {
				const uint32_t vs = __builtin_amdgcn_readlane(lvs, __builtin_ctzll(m));
#pragma unroll
				for (uint32_t u = 0; u < U; u++)
					c[u] += min(o0 + u * 64 + lane, nl) >= vs;
			}
#pragma unroll
			for (uint32_t u = 0; u < U; u++) {
				const uint32_t r = buf[u];
				k[u] = ((c[u] >> ilog) << g.cbits()) | g.local(r);
				key[u] = g.resid(r);
				lv[u] = g.level(r);
				hb[u] = __umulhi(r & ~((1u << g.pbits) - 1), kAggBuckets);
			}
			// home buckets of all U records in flight together (one ds_read_b128 each)
			KBucket B[U];
#pragma unroll
			for (uint32_t u = 0; u < U; u++)
				B[u] = kb[hb[u]];
			bool any_need = false;
#pragma unroll
			for (uint32_t u = 0; u < U; u++) {
				const uint32_t f = bucket_find(B[u], key[u]);
				slot[u] = f < kAggBW ? hb[u] * kAggBW + f : kAggNoSlot;
				any_need |= f >= kAggBW;
			}
			// first sight of an element, or a chain past its home bucket: to the
			// wave's queue (the record's own level first is taken there)
			if (__builtin_amdgcn_readfirstlane((uint32_t)(__ballot(any_need) != 0))) {
#pragma unroll
				for (uint32_t u = 0; u < U; u++) {
					const bool nd = slot[u] == kAggNoSlot;
					const uint64_t m = __ballot(nd);
					if (!m)
						continue;
					const uint32_t c = (uint32_t)__popcll(m);
					if (qn + c > 64)
						flush_queue();
					if (nd)
						wq[qn + lane_rank(m)] = make_uint2(key[u], (lv[u] << 24) | k[u]);
					qn += c;
				}
				__builtin_amdgcn_wave_barrier();
			}
#pragma unroll
			for (uint32_t u = 0; u < U; u++)
				if (slot[u] != kAggNoSlot)
					atomicMin(&fl[lv[u]][slot[u]], k[u]);
		};
		// a ring of D + 1 register buffers, rotated by full unrolling (static
		// indices: no register moves that would wait for the prefetch)
		uint32_t buf[D + 1][U];
#pragma unroll
		for (uint32_t d = 0; d < D; d++)
			fetch(buf[d], d * U * 64);
		bool more = true;
		for (uint32_t o0 = 0; more;) {
#pragma unroll
			for (uint32_t t = 0; t <= D; t++) {
				if (more) {
					fetch(buf[(t + D) % (D + 1)], o0 + D * U * 64);
					absorb(buf[t], o0);
					o0 += U * 64;
					// (the overflow flag is an LDS read, and its wait would also wait
					// for this batch's ds_min: checked once per group of cells
					// -- a full table ends every probe chain at once anyway,
					// agg_find_insert)
					more = o0 < n;
				}
			}
		}
	}
	flush_queue();  // every record is absorbed before the barrier
	__syncthreads();
	return !L.s_ovf;
}

// ---------------------------------------------------------------- aggregation
// One workgroup per aggregation partition.  Waves take groups of gsz
// cells (chunks) from an LDS counter and walk each group as one virtual run.
// Cell (c, p): counted layout, the partition's records from rec_base[p] with
// cell offsets offsT[p][.]; capped layout (kCap), cap[c] records from
// base[c] + p * cap[c] of which cnt[p][c] are written.  Output: the
// partition's distinct elements and their level firsts at
// dist_*[p * kAggRegion ...], cnt[p] = how many, or kAggOverflow when they do
// not fit the LDS table.
// U records per lane per batch, D batches in flight ahead of the one absorbed.
template <uint32_t U, uint32_t D, bool kCap, bool kIdx32 = false>
__global__ __launch_bounds__(kAggThreads) void k_agg(AggCells x, AggGeom g, uint32_t* dist_e, uint4* dist_f,
                                                     uint32_t* cnt)
{
	__shared__ AggLds L;
	const uint32_t* keys = reinterpret_cast<const uint32_t*>(L.kb);
	const uint32_t P = 1u << g.pbits, lane = lane_id();
	if (x.spill && *x.spill)
		return;  // a cell spilled: the records are incomplete and the run is redone
	for (uint32_t p = blockIdx.x; p < P; p += gridDim.x) {
		if (!agg_partition<U, D, kCap, kIdx32>(L, p, x, g)) {
			if (threadIdx.x == 0) {
				cnt[p] = kAggOverflow;
				if (x.ctr)
					atomicAdd(&x.ctr[kCntAggOvf], 1ull);
			}
			__syncthreads();
			continue;
		}
		// compact the occupied slots, elements restored from (p, residual)
		const uint32_t hp = p << g.rbits();
		for (uint32_t i0 = 0; i0 < kAggSlots; i0 += kAggThreads) {
			const uint32_t i = i0 + threadIdx.x;
			const uint32_t key = i < kAggSlots ? keys[i] : kAggEmpty;
			const bool occ = key != kAggEmpty;
			const uint64_t m = __ballot(occ);
			uint32_t wb = 0;
			if (lane == 0 && m)
				wb = atomicAdd(&L.s_out, (uint32_t)__popcll(m));
			wb = __shfl(wb, 0, 64);
			if (occ) {
				const uint64_t o = (uint64_t)p * kAggRegion + wb + lane_rank(m);
				dist_e[o] = fmix32_inv(hp | key);
				dist_f[o] = make_uint4(L.fl[0][i], L.fl[1][i], L.fl[2][i], L.fl[3][i]);
			}
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			cnt[p] = L.s_out;
			if (x.ctr && L.s_out)
				atomicAdd(&x.ctr[kCntDistinct], (unsigned long long)L.s_out);
		}
		__syncthreads();
	}
}

// k_agg over records [0, extent): 32-bit record indices when they fit (fewer
// vector instructions per record: 1.45 -> 1.40 ms at C2; the
// 64-bit kernel for larger runs, and under SYZSIG_DEBUG_AGG_IDX64 for tests)
template <bool kCap>
static void launch_agg(const syzsig_ctx* ctx, uint64_t extent, uint32_t P, hipStream_t s, const AggCells& xc,
                       const AggGeom& g, void* de, void* df, void* dc)
{
	if (extent <= (1ull << 32) && !(ctx->agg_dbg & SYZSIG_DEBUG_AGG_IDX64))
		k_agg<kAggU, kAggD, kCap, true><<<P, kAggThreads, 0, s>>>(xc, g, (uint32_t*)de, (uint4*)df, (uint32_t*)dc);
	else
		k_agg<kAggU, kAggD, kCap, false><<<P, kAggThreads, 0, s>>>(xc, g, (uint32_t*)de, (uint4*)df, (uint32_t*)dc);
}

// ---- fallback: partitions whose distinct elements overflow the LDS table are
// aggregated in one HBM hash table keyed by h (gkeys[C] + gfl[4][C + 1], C a
// power of two; slot C is h = 0xFFFFFFFF).  Partitions hold disjoint
// elements, so one table serves all of them.
// One record of element hash h at `level` with run serial `serial` into the
// table: find or insert h (linear probing, a CAS on first sight), then the
// level's first by atomicMin.  bad counts a probe sequence that ran through
// the whole table (the host reports it as an internal error).
__device__ __forceinline__ void hbm_absorb(uint32_t* gkeys, uint32_t* gfl, uint64_t C, uint32_t h, uint32_t level,
                                           uint32_t serial, uint64_t& bad)
{
	uint64_t i = C;
	if (h != kAggEmpty) {
		i = fmix32(h ^ 0x632BE5ABu) & (C - 1);
		for (uint64_t step = 0;; step++) {
			uint32_t key = gkeys[i];
			if (key == kAggEmpty) {
				key = atomicCAS(&gkeys[i], kAggEmpty, h);
				if (key == kAggEmpty)
					break;
			}
			if (key == h)
				break;
			i = (i + 1) & (C - 1);
			if (step >= C) {
				bad++;
				return;
			}
		}
	}
	atomicMin(&gfl[(uint64_t)level * (C + 1) + i], serial);
}

// k_agg_global: counted cells, one wave per (partition, group of cells).
__global__ __launch_bounds__(256) void k_agg_global(const uint32_t* __restrict__ recs,
                                                    const uint64_t* __restrict__ rec_base,
                                                    const uint32_t* __restrict__ offsT, uint64_t nchunks, AggGeom g,
                                                    const uint32_t* __restrict__ ovl, uint32_t novl, uint32_t* gkeys,
                                                    uint32_t* gfl, uint64_t C, unsigned long long* err)
{
	const uint32_t lane = lane_id();
	const uint64_t ngroups = (nchunks + kAggGroup - 1) / kAggGroup, items = (uint64_t)novl * ngroups;
	const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
	uint64_t bad = 0;
	for (uint64_t it = blockIdx.x * (uint64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); it < items; it += nwaves) {
		const uint32_t p = ovl[it / ngroups];
		const uint32_t* ot = offsT + (uint64_t)p * (nchunks + 1);
		const uint32_t* pr = recs + rec_base[p];
		CellGroup cg;
		cg.load(ot, nchunks, it % ngroups);
		for (uint32_t j = cg.bnd[0] + lane; j < cg.bnd[kAggGroup]; j += 64) {
			const uint32_t r = pr[j];
			const uint32_t k = cg.serial(j, r, g), l = g.level(r);
			const uint32_t h = (p << g.rbits()) | g.resid(r);
			hbm_absorb(gkeys, gfl, C, h, l, k, bad);
		}
	}
	block_count(err, bad);
}

__global__ __launch_bounds__(256) void k_agg_global_compact(const uint32_t* __restrict__ gkeys,
                                                            const uint32_t* __restrict__ gfl, uint64_t C,
                                                            uint32_t* dist_e, uint4* dist_f,
                                                            unsigned long long* out_cnt)
{
	const uint32_t lane = lane_id();
	for (uint64_t i0 = blockIdx.x * (uint64_t)blockDim.x; i0 <= C; i0 += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t i = i0 + threadIdx.x;
		bool occ = false;
		uint32_t h = kAggEmpty;
		uint4 f = make_uint4(kNoFirst, kNoFirst, kNoFirst, kNoFirst);
		if (i <= C) {
			f = make_uint4(gfl[i], gfl[(C + 1) + i], gfl[2 * (C + 1) + i], gfl[3 * (C + 1) + i]);
			if (i < C) {
				h = gkeys[i];
				occ = h != kAggEmpty;
			} else {
				occ = (f.x & f.y & f.z & f.w) != kNoFirst;
			}
		}
		const uint64_t m = __ballot(occ);
		unsigned long long wb = 0;
		if (lane == 0 && m)
			wb = atomicAdd(out_cnt, (unsigned long long)__popcll(m));
		wb = __shfl(wb, 0, 64);
		if (occ) {
			dist_e[wb + lane_rank(m)] = fmix32_inv(h);
			dist_f[wb + lane_rank(m)] = f;
		}
	}
}

// ---------------------------------------------------------------- finalize
// checkNewSignal's decision for one distinct element e with level firsts f4,
// in pieces that the three finalize codes compose (fin_top, fin_raises and
// stair_walk are in decide.h: the records path of recs.hip composes them too):
//   fin_top      the top level present; M_final[e] can only become P = lm.val[top]
//   (the slot)   e's maxSignal slot, found or inserted -- the one step that
//                differs: global atomics (fin_commit_atomic, for k_agg_finalize
//                and k_fin_deferred) or the block's own slice (k_agg_finalize_x)
//   fin_raises   M0[e] from the slot's word; whether P raises it; the counts
//   (newSignal)  merge (e, P), by the same means as the slot
//   fin_emit     the staircase above M0[e] (stair_walk): call_new and the pairs
// Arguments of the finalize kernels (fin_tables and fin_args fill them).
struct FinArgs {
	LevelMap lm;
	uint64_t c0;
	uint64_t* slots;  // maxSignal
	uint64_t bmask;
	uint64_t* ns_slots;  // newSignal
	uint64_t ns_bmask;
	uint8_t* call_new;
	uint64_t* pairs;
	unsigned long long* npairs;
	unsigned long long* ctr;
	// the slice-exclusive finalize only: log2 of a partition's slice in buckets,
	// the deferred lists, SYZSIG_DEBUG_FIN_DEFER
	uint32_t ms_shift, ns_shift;
	uint32_t* def_e;
	uint4* def_f;
	unsigned long long* def_cnt;
	uint64_t* def_ns;
	unsigned long long* def_ns_cnt;
	uint32_t dbg;
	// a one-sync run: its void flag, and the counter of overflowed partitions
	// with the gate past which nothing is committed
	const uint32_t* spill;
	const unsigned long long* ovf_gate;
	uint32_t gate_max;
};

// The staircase above M0[e] = p0 holds e's new records: their calls are
// flagged and put(call << 32 | e) takes the pairs.
template <typename Put>
__device__ __forceinline__ void fin_emit(const FinArgs& a, uint32_t e, uint4 f4, int top, int p0, Put put)
{
	stair_walk(f4, top, [&](int l) { return (int)a.lm.val[l] <= p0; },
	           [&](int, uint32_t first) {
		           const uint64_t c = a.c0 + first;
		           a.call_new[c] = 1;
		           put((c << 32) | e);
	           });
}

// The decision up to the staircase, with the global-atomic table code: one
// probe sequence inserts M_final = P if e is absent, else reads M0[e]; then
// M_final is stored and newSignal merged.  bm, bn: the home buckets of e in
// the two tables when the caller loaded them ahead.  True (p0 set) when e's
// staircase is to be emitted.
__device__ __forceinline__ bool fin_commit_atomic(const FinArgs& a, uint32_t e, int8_t P, FinCounts& n, int& p0,
                                                  const Bucket* bm = nullptr, const Bucket* bn = nullptr)
{
	const uint64_t word = make_slot(e, P), max_probe = max_probe_for(a.bmask);
	uint64_t old = 0;
	const int64_t idx = bm ? tbl_find_or_insert_from(a.slots, a.bmask, e, word, old, max_probe, *bm)
	                       : tbl_find_or_insert(a.slots, a.bmask, e, word, old, max_probe);
	if (idx < 0) {
		n.ovf++;
		return false;
	}
	if (!fin_raises(old, P, n, p0))  // (old == 0: inserted just now)
		return false;
	if (old != 0)
		a.slots[idx] = word;  // one entry per element: no other writer
	const int rr = bn ? tbl_merge_from(a.ns_slots, a.ns_bmask, e, P, *bn) : tbl_merge(a.ns_slots, a.ns_bmask, e, P);
	n.ns_ins += rr == 1;
	n.ovf += rr < 0;
	return true;
}

// A block's pairs, gathered in LDS and appended to pairs[] with one global
// atomic per flush (a pair that finds the buffer full is appended directly).
template <uint32_t kCap>
struct PairBuf {
	uint64_t buf[kCap];
	uint32_t n;
	unsigned long long base;
	__device__ __forceinline__ void reset()  // (a barrier must follow)
	{
		if (threadIdx.x == 0)
			n = 0;
	}
	__device__ __forceinline__ void emit(uint64_t v, uint64_t* pairs, unsigned long long* npairs)
	{
		const uint32_t k = atomicAdd(&n, 1u);
		if (k < kCap)
			buf[k] = v;
		else
			pairs[atomicAdd(npairs, 1ull)] = v;
	}
	// every thread of the block, after a pass of emits
	__device__ __forceinline__ void flush_if_half(uint64_t* pairs, unsigned long long* npairs)
	{
		__syncthreads();
		const uint32_t nb = n;
		if (nb > kCap / 2)
			flush(nb, pairs, npairs);
	}
	__device__ __forceinline__ void flush_all(uint64_t* pairs, unsigned long long* npairs)
	{
		__syncthreads();
		const uint32_t nb = n;
		if (nb)
			flush(nb, pairs, npairs);
	}
	__device__ __forceinline__ void flush(uint32_t nb, uint64_t* pairs, unsigned long long* npairs)
	{
		nb = min(nb, kCap);
		if (threadIdx.x == 0)
			base = atomicAdd(npairs, (unsigned long long)nb);
		__syncthreads();
		for (uint32_t t = threadIdx.x; t < nb; t += blockDim.x)
			pairs[base + t] = buf[t];
		__syncthreads();
		reset();
		__syncthreads();
	}
};

// A thread's kIlp elements of one pass (from entry i0) over region r of n
// entries, for a block of kThreads: the element, its level firsts and top level.
template <uint32_t kIlp, uint32_t kThreads>
struct FinElems {
	uint32_t e[kIlp];
	uint4 f4[kIlp];
	int top[kIlp];  // -1: nothing to decide
	__device__ __forceinline__ void load(const uint32_t* __restrict__ dist_e, const uint4* __restrict__ dist_f,
	                                     uint32_t r, uint32_t n, uint32_t i0, const LevelMap& lm)
	{
#pragma unroll
		for (uint32_t k = 0; k < kIlp; k++) {
			const uint32_t i = i0 + k * kThreads + threadIdx.x;
			const uint64_t o = (uint64_t)r * kAggRegion + min(i, n - 1);
			e[k] = dist_e[o];
			f4[k] = dist_f[o];
			top[k] = fin_top(f4[k], lm, i < n);
		}
	}
};

// ---- the finalize with device-scope atomics: any regions, any table sizes
// (the HBM fallback's lists; tables with fewer buckets than partitions) ----
// One workgroup per region r = dist_*[r * kAggRegion, + cnt[r]): a partition's
// distinct elements, whose maxSignal/newSignal home buckets share one slice of
// each table (the same top bits of h), so a block's probes stay in one slice.
// Each thread takes kFinIlp elements per pass and issues the loads of all their
// home buckets (maxSignal and newSignal) before walking any of them: the
// kernel is bound by the latency of these dependent random reads, not by
// bandwidth, so more of them in flight per wave is what makes it faster.
constexpr uint32_t kFinThreads = 256, kFinBuf = 4 * kFinThreads * 2, kFinIlp = 2;

__global__ __launch_bounds__(kFinThreads) void k_agg_finalize(const uint32_t* __restrict__ dist_e,
                                                              const uint4* __restrict__ dist_f,
                                                              const uint32_t* __restrict__ cnt, uint32_t nregions,
                                                              FinArgs a)
{
	__shared__ PairBuf<kFinBuf> pb;
	FinCounts n;
	const auto put = [&](uint64_t v) { pb.emit(v, a.pairs, a.npairs); };
	pb.reset();
	__syncthreads();
	for (uint32_t r = blockIdx.x; r < nregions; r += gridDim.x) {
		const uint32_t nr = cnt[r] == kAggOverflow ? 0 : cnt[r];
		for (uint32_t i0 = 0; i0 < nr; i0 += kFinIlp * kFinThreads) {
			FinElems<kFinIlp, kFinThreads> t;
			t.load(dist_e, dist_f, r, nr, i0, a.lm);
			Bucket bm[kFinIlp], bn[kFinIlp];
#pragma unroll
			for (uint32_t k = 0; k < kFinIlp; k++) {
				if (t.top[k] >= 0) {
					bm[k] = load_bucket(a.slots + (home_bucket(t.e[k], a.bmask) << kBucketShift));
					bn[k] = load_bucket(a.ns_slots + (home_bucket(t.e[k], a.ns_bmask) << kBucketShift));
				}
			}
#pragma unroll
			for (uint32_t k = 0; k < kFinIlp; k++) {
				int p0 = 0;
				if (t.top[k] >= 0 && fin_commit_atomic(a, t.e[k], a.lm.val[t.top[k]], n, p0, &bm[k], &bn[k]))
					fin_emit(a, t.e[k], t.f4[k], t.top[k], p0, put);
			}
			pb.flush_if_half(a.pairs, a.npairs);
		}
	}
	pb.flush_all(a.pairs, a.npairs);
	n.report(a.ctr);
}

// ---- the finalize without device-scope atomics (the fast path) ----
// Region r < P is partition r, and the home buckets of its elements form one
// contiguous slice of maxSignal (and of newSignal) whenever the table has at
// least P buckets: slice = buckets [r << shift, (r + 1) << shift).  Inside a
// slice the block is the only writer during this launch, so a found element is
// updated with a plain store, and an absent one takes the first empty slot of
// its probe sequence that no other element of the block claimed first -- the
// claims are LDS compare-and-swaps on the slot's index, not global atomics
// (measured: device-scope CAS runs at ~20 G/s chip-wide and bounded the
// atomic finalize).  Probe sequences stop at the slice end: such an element
// (or one whose claim table is full) is deferred, and so is a newSignal merge
// that leaves its slice: k_fin_deferred takes both lists after this launch,
// with the global-atomic code.
// Correct slot choice: slots only go empty -> key, so an element present at
// launch start sits before the first slot that was empty then; a slot seen
// occupied, or claimed by another element, is occupied at launch end, so the
// occupied-prefix invariant of every probe sequence still holds.
constexpr uint32_t kFxThreads = 512, kFxSet = 8192, kFxBuf = 2048, kFxProbe = 64;
enum : int { kFxTaken = 0, kFxClaimed = 1, kFxFull = 2 };

__device__ __forceinline__ int fx_claim(uint32_t* set, uint32_t tag, uint64_t rel)
{
	const uint32_t key = (tag << 31) | (uint32_t)(rel + 1);
	uint32_t h = fmix32(key) & (kFxSet - 1);
	for (uint32_t step = 0; step < kFxProbe; step++) {
		uint32_t v = set[h];
		if (v == 0) {
			v = atomicCAS(&set[h], 0u, key);
			if (v == 0)
				return kFxClaimed;
		}
		if (v == key)
			return kFxTaken;
		h = (h + 1) & (kFxSet - 1);
	}
	return kFxFull;
}

// Walk the probe sequence of e inside [b, bend) (B = the home bucket, loaded).
// Returns the slot index with old = its word (found), or with old = 0 (claimed
// for e); -1 = defer (slice end, or the claim table is full).
__device__ __forceinline__ int64_t fx_walk(const uint64_t* tab, uint64_t b, uint64_t bend, uint64_t slice0,
                                           uint32_t e, Bucket B, uint32_t* set, uint32_t tag, uint64_t& old)
{
	for (uint64_t b0 = b; b < bend; b++) {
		if (b != b0)
			B = load_bucket(tab + (b << kBucketShift));
#pragma unroll
		for (uint32_t i = 0; i < kBucketSlots; i++) {
			const uint64_t sw = B.s[i], idx = (b << kBucketShift) + i;
			if (sw != kSlotEmpty) {
				if (slot_key(sw) == e) {
					old = sw;
					return (int64_t)idx;
				}
				continue;
			}
			const int c = fx_claim(set, tag, idx - slice0);
			if (c == kFxClaimed) {
				old = 0;
				return (int64_t)idx;
			}
			if (c == kFxFull)
				return -1;
		}
	}
	return -1;
}

template <uint32_t kFxIlp>
__global__ __launch_bounds__(kFxThreads) void k_agg_finalize_x(const uint32_t* __restrict__ dist_e,
                                                               const uint4* __restrict__ dist_f,
                                                               const uint32_t* __restrict__ cnt, uint32_t nregions,
                                                               FinArgs a)
{
	__shared__ uint32_t claim[kFxSet];
	__shared__ PairBuf<kFxBuf> pb;
	if (a.spill && *a.spill)
		return;  // a cell spilled: nothing is committed, the run is redone
	if (a.ovf_gate && *a.ovf_gate > a.gate_max)
		return;  // the partitions were too few for the run's distinct elements: redone with more
	FinCounts n;
	const auto put = [&](uint64_t v) { pb.emit(v, a.pairs, a.npairs); };
	for (uint32_t r = blockIdx.x; r < nregions; r += gridDim.x) {
		for (uint32_t i = threadIdx.x; i < kFxSet; i += blockDim.x)
			claim[i] = 0;
		pb.reset();
		__syncthreads();
		const uint64_t ms0 = (uint64_t)r << a.ms_shift, ms1 = (uint64_t)(r + 1) << a.ms_shift;
		const uint64_t ns0 = (uint64_t)r << a.ns_shift, ns1 = (uint64_t)(r + 1) << a.ns_shift;
		const uint32_t nr = cnt[r];
		if (nr == kAggOverflow)
			continue;  // past the LDS table: aggregated in HBM and committed after this launch
		for (uint32_t i0 = 0; i0 < nr; i0 += kFxIlp * kFxThreads) {
			FinElems<kFxIlp, kFxThreads> t;
			t.load(dist_e, dist_f, r, nr, i0, a.lm);
			Bucket bm[kFxIlp], bn[kFxIlp];
#pragma unroll
			for (uint32_t k = 0; k < kFxIlp; k++) {
				if (t.top[k] >= 0) {
					bm[k] = load_bucket(a.slots + (home_bucket(t.e[k], a.bmask) << kBucketShift));
					bn[k] = load_bucket(a.ns_slots + (home_bucket(t.e[k], a.ns_bmask) << kBucketShift));
				}
			}
#pragma unroll
			for (uint32_t k = 0; k < kFxIlp; k++) {
				if (t.top[k] < 0)
					continue;
				const uint32_t e = t.e[k];
				const int8_t P = a.lm.val[t.top[k]];
				const uint64_t word = make_slot(e, P);
				uint64_t old = 0;
				// (SYZSIG_DEBUG_FIN_DEFER, tests: defer every walk that leaves the home bucket)
				const uint64_t hm = home_bucket(e, a.bmask), hn = home_bucket(e, a.ns_bmask);
				const int64_t idx = fx_walk(a.slots, hm, a.dbg & SYZSIG_DEBUG_FIN_DEFER ? hm + 1 : ms1,
				                            ms0 << kBucketShift, e, bm[k], claim, 0, old);
				if (idx < 0) {  // the atomic path takes the whole element
					const uint64_t d = atomicAdd(a.def_cnt, 1ull);
					a.def_e[d] = e;
					a.def_f[d] = t.f4[k];
					continue;
				}
				int p0 = 0;
				if (!fin_raises(old, P, n, p0))
					continue;  // (a claimed slot always has P > p0)
				a.slots[idx] = word;  // the block's own slice: no other writer
				uint64_t nold = 0;
				const int64_t nidx = fx_walk(a.ns_slots, hn, a.dbg & SYZSIG_DEBUG_FIN_DEFER ? hn + 1 : ns1,
				                             ns0 << kBucketShift, e, bn[k], claim, 1, nold);
				if (nidx < 0) {
					a.def_ns[atomicAdd(a.def_ns_cnt, 1ull)] = ((uint64_t)e << 32) | prio_biased(P);
				} else if (nold == 0 || nold < word) {
					a.ns_slots[nidx] = word;
					n.ns_ins += nold == 0;
				}
				fin_emit(a, e, t.f4[k], t.top[k], p0, put);
			}
			pb.flush_if_half(a.pairs, a.npairs);
		}
		pb.flush_all(a.pairs, a.npairs);
	}
	n.report<false>(a.ctr);
}

// Deferred elements of k_agg_finalize_x, with the global-atomic table code
// (launched after it: the slices are free for everyone again).
__device__ __forceinline__ void fin_deferred(const FinArgs& a, uint32_t nblocks, uint32_t block)
{
	const uint64_t nd = *a.def_cnt;
	FinCounts n;
	for (uint64_t i = block * (uint64_t)blockDim.x + threadIdx.x; i < nd; i += (uint64_t)nblocks * blockDim.x) {
		const uint32_t e = a.def_e[i];
		const uint4 f4 = a.def_f[i];
		const int top = fin_top(f4, a.lm, true);
		int p0 = 0;
		if (top >= 0 && fin_commit_atomic(a, e, a.lm.val[top], n, p0))
			fin_emit(a, e, f4, top, p0, [&](uint64_t v) { a.pairs[atomicAdd(a.npairs, 1ull)] = v; });
	}
	n.report(a.ctr);
}

// Deferred newSignal merges of k_agg_finalize_x: (elem << 32 | prio ^ 0x80).
__device__ __forceinline__ void ns_deferred(const FinArgs& a, uint32_t nblocks, uint32_t block)
{
	const uint64_t nd = *a.def_ns_cnt;
	uint64_t ins = 0, ovf = 0;
	for (uint64_t i = block * (uint64_t)blockDim.x + threadIdx.x; i < nd; i += (uint64_t)nblocks * blockDim.x) {
		const uint64_t v = a.def_ns[i];
		const int r = tbl_merge(a.ns_slots, a.ns_bmask, (uint32_t)(v >> 32), (int8_t)((uint8_t)v ^ 0x80u));
		ins += r == 1;
		ovf += r < 0;
	}
	block_count(&a.ctr[kCntAux], ins);
	block_count(&a.ctr[kCntOverflow], ovf);
}

// Both deferred lists in one launch: the first kDeferBlocks blocks take the
// elements, the rest the newSignal merges (both sides only ever max-merge
// newSignal with atomics, so they commute).
constexpr uint32_t kDeferBlocks = 64;
__global__ __launch_bounds__(256) void k_fin_deferred(FinArgs a)
{
	if (blockIdx.x < kDeferBlocks)
		fin_deferred(a, kDeferBlocks, blockIdx.x);
	else
		ns_deferred(a, gridDim.x - kDeferBlocks, blockIdx.x - kDeferBlocks);
}

// ---------------------------------------------------------------- one-sync run
// (Round 3 measured aggregation and finalize in one launch -- the distinct
// elements kept in registers, the freed LDS as claim set -- at 1.18 ms against
// 0.64 + 0.27 for the two launches at C2, and removed it: one 1024-thread
// workgroup per CU held the LDS through its random probes.)

// Fallback of the one-sync run: the records of the partitions that overflowed
// the LDS table, aggregated in one HBM table keyed by h (as k_agg_global) from
// their capped cells.  One wave per (partition, chunk).
__global__ __launch_bounds__(256) void k_agg_global_cap(const uint32_t* __restrict__ recs,
                                                        const uint64_t* __restrict__ cap_base,
                                                        const uint32_t* __restrict__ cap_len,
                                                        const uint32_t* __restrict__ cap_cnt, uint64_t nchunks,
                                                        AggGeom g, const uint32_t* __restrict__ ovl, uint32_t novl,
                                                        uint32_t* gkeys, uint32_t* gfl, uint64_t C,
                                                        unsigned long long* err)
{
	const uint32_t lane = lane_id();
	const uint64_t items = (uint64_t)novl * nchunks, nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
	uint64_t bad = 0;
	for (uint64_t it = blockIdx.x * (uint64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); it < items; it += nwaves) {
		const uint32_t p = ovl[it / nchunks];
		const uint64_t c = it % nchunks;
		const uint32_t* pr = recs + cap_base[c] + (uint64_t)p * cap_len[c];
		const uint32_t n = cap_cnt[(uint64_t)p * nchunks + c];
		for (uint32_t j = lane; j < n; j += 64) {
			const uint32_t r = pr[j];
			const uint32_t k = ((uint32_t)c << g.cbits()) | g.local(r), l = g.level(r);
			const uint32_t h = (p << g.rbits()) | g.resid(r);
			hbm_absorb(gkeys, gfl, C, h, l, k, bad);
		}
	}
	block_count(err, bad);
}

// ---------------------------------------------------------------- new bits
__device__ __forceinline__ uint64_t pair_hash(uint64_t k)
{
	k ^= k >> 33;
	k *= 0xff51afd7ed558ccdull;
	k ^= k >> 33;
	k *= 0xc4ceb9fe1a85ec53ull;
	k ^= k >> 33;
	return k;
}

// Insert pairs into a set of capacity C (power of two, empty = ~0).
// Duplicates are dropped; `uniq` counts distinct ones.
__global__ __launch_bounds__(256) void k_pairs_set(const uint64_t* __restrict__ pairs, uint64_t n, uint64_t* set,
                                                   uint64_t C, unsigned long long* uniq)
{
	uint64_t u = 0;
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t v = pairs[t];
		uint64_t i = pair_hash(v) & (C - 1);
		for (uint64_t step = 0; step < C; step++) {
			uint64_t k = set[i];
			if (k == ~0ull) {
				k = atomicCAS((unsigned long long*)&set[i], ~0ull, (unsigned long long)v);
				if (k == ~0ull) {
					u++;
					break;
				}
			}
			if (k == v)
				break;
			i = (i + 1) & (C - 1);
		}
	}
	block_count(uniq, u);
}

__device__ __forceinline__ bool pairs_has(const uint64_t* set, uint64_t C, uint64_t v)
{
	uint64_t i = pair_hash(v) & (C - 1);
	for (uint64_t step = 0; step < C; step++) {
		const uint64_t k = set[i];
		if (k == v)
			return true;
		if (k == ~0ull)
			return false;
		i = (i + 1) & (C - 1);
	}
	return false;
}

// one wave per call: bit r = (call, sigs[r]) is a new pair
__global__ __launch_bounds__(256) void k_pairs_mark(const uint32_t* __restrict__ sigs,
                                                    const uint64_t* __restrict__ call_start,
                                                    const uint32_t* __restrict__ call_len, uint64_t c0, uint64_t c1,
                                                    const uint8_t* __restrict__ call_new, const uint64_t* set,
                                                    uint64_t C, uint32_t* new_bits)
{
	const uint32_t lane = lane_id();
	const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
	for (uint64_t c = c0 + blockIdx.x * (uint64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); c < c1; c += nwaves) {
		if (!call_new[c])
			continue;
		const uint64_t st = call_start[c];
		const uint32_t len = call_len[c];
		for (uint32_t j = lane; j < len; j += 64)
			if (pairs_has(set, C, (c << 32) | sigs[st + j]))
				atomicOr(&new_bits[(st + j) >> 5], 1u << ((st + j) & 31));
	}
}

// dedupped pairs from the set (compaction)
__global__ __launch_bounds__(256) void k_pairs_compact(const uint64_t* __restrict__ set, uint64_t C, uint64_t* out,
                                                       unsigned long long* n)
{
	const uint32_t lane = lane_id();
	for (uint64_t i0 = blockIdx.x * (uint64_t)blockDim.x; i0 < C; i0 += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t i = i0 + threadIdx.x;
		const uint64_t v = i < C ? set[i] : ~0ull;
		const bool occ = v != ~0ull;
		const uint64_t m = __ballot(occ);
		unsigned long long wb = 0;
		if (lane == 0 && m)
			wb = atomicAdd(n, (unsigned long long)__popcll(m));
		wb = __shfl(wb, 0, 64);
		if (occ)
			out[wb + lane_rank(m)] = v;
	}
}

// pairs from per-record bits of calls [c0, c1) (per-call path); may repeat a pair
__global__ __launch_bounds__(256) void k_bits_to_pairs(const uint32_t* __restrict__ sigs,
                                                       const uint64_t* __restrict__ call_start,
                                                       const uint32_t* __restrict__ call_len, uint64_t c0, uint64_t c1,
                                                       const uint8_t* __restrict__ call_new,
                                                       const uint32_t* __restrict__ bits, uint64_t* pairs,
                                                       unsigned long long* n)
{
	const uint32_t lane = lane_id();
	const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
	for (uint64_t c = c0 + blockIdx.x * (uint64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); c < c1; c += nwaves) {
		if (!call_new[c])
			continue;
		const uint64_t st = call_start[c];
		const uint32_t len = call_len[c];
		for (uint32_t j0 = 0; j0 < len; j0 += 64) {
			const uint32_t j = j0 + lane;
			const bool on = j < len && ((bits[(st + j) >> 5] >> ((st + j) & 31)) & 1);
			const uint64_t m = __ballot(on);
			unsigned long long wb = 0;
			if (lane == 0 && m)
				wb = atomicAdd(n, (unsigned long long)__popcll(m));
			wb = __shfl(wb, 0, 64);
			if (on)
				pairs[wb + lane_rank(m)] = (c << 32) | sigs[st + j];
		}
	}
}

// ---------------------------------------------------------------- host
static uint64_t pow2_at_least(uint64_t x)
{
	uint64_t p = 1;
	while (p < x)
		p <<= 1;
	return p;
}

static AggGeom agg_geom_for(syzsig_ctx* ctx, uint64_t nrec, double distinct_hint, double load = kAggTargetLoad)
{
	AggGeom g;
	if (ctx->agg_parts) {
		g.pbits = 31 - __builtin_clz(ctx->agg_parts);  // validated power of two in [8, 2048]
		return g;
	}
	// expected distinct elements: the caller's hint, else the ratio seen on the
	// previous large batch (1/32 before the first); big runs keep >= 256
	// partitions (one per CU)
	const double ratio = ctx->agg_distinct_ratio > 0 ? ctx->agg_distinct_ratio : 1.0 / 32;
	const double d = distinct_hint > 0 ? distinct_hint : ratio * (double)nrec;
	uint32_t pb = nrec >= (1ull << 24) ? 8 : kAggMinBits;
	while (pb < kAggMaxBits && d > load * kAggSlots * (double)(1u << pb))
		pb++;
	g.pbits = pb;
	return g;
}

// k_agg's cells per wave work item: ~64 items per partition (4 per wave),
// at least kAggGroup and at most one cell per lane
static uint32_t agg_group_size(uint64_t ncells)
{
	uint32_t gz = kAggGroup;
	while (gz < 64 && ncells / gz > 64)
		gz <<= 1;
	return gz;
}

// The distinct lists and region counts of a run of P partitions.
static int agg_lists(syzsig_ctx* ctx, uint32_t P, void** de, void** df, void** dc)
{
	SYZ_TRY(ws_get(ctx, kWsAggDistE, (uint64_t)P * kAggRegion * 4 + 64, de));
	SYZ_TRY(ws_get(ctx, kWsAggDistF, (uint64_t)P * kAggRegion * 16 + 64, df));
	return ws_get(ctx, kWsAggCnt, (uint64_t)(P + 1) * 4 + 64, dc);
}

// ---- the capped-cell front end: layout, plan, scatter and k_agg of one run,
// shared by agg_capped, the one-sync run (agg_triage_fused) and the sharded
// step's fast path (syzsig_step_send_dev).
struct CapRun {
	uint64_t nchunks;  // work items
	uint32_t S;        // cells per work item (= partitions)
	float sd;          // the cells' slack, in standard deviations
	uint64_t bound;    // records reserved for the cells; the dummy lines follow
	uint32_t* recs;
	uint64_t *sizes, *cbase;              // per work item: records, first record of its cells
	uint32_t *ccap, *ccnt, *ovf, *tiles;  // cell capacity, records per cell, the spill flag, k_scat3 tiles
	void *de, *df, *dc;                   // k_agg's output (agg_lists)
};

// Workspaces of a run's capped cells: the records, then kWsAggCells carved in
// one fixed layout.
static int cap_layout(syzsig_ctx* ctx, uint64_t run_recs, uint64_t nchunks, uint32_t S, float sd, CapRun* r)
{
	r->nchunks = nchunks;
	r->S = S;
	r->sd = sd;
	// upper bound of sum_c S * cap[c] (k_cell_plan): 1.25 records + per cell
	// sd^2 + 128; a multiple of 64 records, because the dummy lines after it
	// take 16-B stores
	r->bound = (run_recs + run_recs / 4 + nchunks * S * (uint64_t)(sd * sd + 128.0f) + 127) & ~63ull;
	void *recs, *cm;
	SYZ_TRY(ws_get(ctx, kWsAggRecs, (r->bound + kDummyLines * kBlk) * 4, &recs));
	SYZ_TRY(ws_get(ctx, kWsAggCells, nchunks * 24 + (uint64_t)S * nchunks * 4 + 256, &cm));
	r->recs = (uint32_t*)recs;
	r->sizes = (uint64_t*)cm;
	r->cbase = r->sizes + nchunks;
	r->ccap = (uint32_t*)(r->cbase + nchunks);
	r->ccnt = r->ccap + nchunks;
	r->ovf = r->ccnt + (uint64_t)S * nchunks;
	r->tiles = r->ovf + 1;
	return agg_lists(ctx, S, &r->de, &r->df, &r->dc);
}

// The two launches before the scatter.  fast_ctr == nullptr: the planned pair
// (the caller validated the batch; `tile` = records per k_scat3 tile).  Else
// the fast pair, which checks the run's assumptions against lm and b->nrec,
// zeroes b->call_new and the counter block fast_ctr (npairs0 preset) and keeps
// the run's void flag there: r->ovf becomes the low word of fast_ctr[kCntSpill].
static int cap_plan(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t c0, uint64_t c1, const LevelMap& lm,
                    const AggGeom& g, uint64_t run_recs, CapRun* r, uint32_t tile, unsigned long long* fast_ctr = nullptr,
                    uint64_t npairs0 = 0)
{
	const hipStream_t s = ctx->stream;
	if (fast_ctr) {
		void* dpart;
		SYZ_TRY(ws_get(ctx, kWsFastPart, r->nchunks * 16 + 64, &dpart));
		r->ovf = (uint32_t*)&fast_ctr[kCntSpill];
		k_fast_prep<<<(uint32_t)r->nchunks, 256, 0, s>>>(b->call_start, b->call_len, b->call_prio, c0, c1, g.ibits,
		                                                 b->nrec, r->sizes, (uint64_t*)dpart, b->call_new, lm, r->tiles);
		k_cell_plan_fast<<<1, 1024, 0, s>>>(r->sizes, r->nchunks, r->S, r->sd, r->cbase, r->ccap,
		                                    (const uint64_t*)dpart, run_recs, npairs0, fast_ctr);
	} else {
		const bool tight = ctx->agg_dbg & SYZSIG_DEBUG_CAP_SPILL;
		SYZ_HIP(hipMemsetAsync(r->ovf, 0, 4, s));
		k_chunk_sizes<<<(uint32_t)r->nchunks, 256, 0, s>>>(b->call_len, c0, c1, g.ibits, r->sizes, r->tiles, tile);
		k_cell_plan<<<1, 1024, 0, s>>>(r->sizes, r->nchunks, r->S, tight ? -1.0f : r->sd, r->cbase, r->ccap);
	}
	return SYZSIG_OK;
}

// Scatter the run's records into its cells, then k_agg.  xp: Minimize's
// per-record extras (nullptr: a triage run).  ctr: the counter block k_agg
// reports into and whose void flag (r.ovf) it obeys (nullptr: neither).
// ev: the context's timing events to record after each of the two (or nullptr).
static int cap_scatter_agg(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t c0, uint64_t c1, const LevelMap& lm,
                           const AggGeom& g, const CapRun& r, uint32_t tile, const AggSrc* xp, unsigned long long* ctr,
                           hipEvent_t* ev)
{
	const hipStream_t s = ctx->stream;
	const CapCells cc{r.cbase, r.ccap, r.ccnt, r.ovf, r.nchunks, r.recs + r.bound, r.sizes, r.tiles, false, tile};
	launch_capped_scatter(s, b, c0, c1, lm, g, cc, r.recs, xp);
	SYZ_HIP(hipGetLastError());
	if (ev && ctx->timing)
		SYZ_HIP(hipEventRecord(ev[1], s));
	const AggCells xc{r.recs, nullptr, nullptr, r.cbase, r.ccap, r.ccnt, r.nchunks, g.items_per_chunk_log2(),
	                  agg_group_size(r.nchunks), ctr ? r.ovf : nullptr, ctr};
	launch_agg<true>(ctx, r.bound, r.S, s, xc, g, r.de, r.df, r.dc);
	SYZ_HIP(hipGetLastError());
	if (ev && ctx->timing)
		SYZ_HIP(hipEventRecord(ev[2], s));
	return SYZSIG_OK;
}

// The count-free attempt: scatter into capped cells (no count pass, no scan),
// then aggregate.  Cells belong to work items of 2^g.ibits calls (chunks for a
// triage run, smaller items for Minimize: xp != nullptr).  *done = false when
// the run must be redone with counted cells: a cell overflowed (the slack is
// doubled for the next run of the kind, and capped cells are given up past
// kCapSdMax), or a partition overflowed the LDS table (its HBM fallback reads
// counted cells).
constexpr float kCapSdMax = 24.0f;
void cap_slack_after_spill(float& slack)
{
	slack = slack * 2 > kCapSdMax ? 0.0f : slack * 2;
}

// After novf of a run's P LDS partitions overflowed (D distinct elements
// counted in the others): the distinct-ratio guess was low, and the next runs
// are sized for at least what was seen -- an overflowed partition held more
// than kAggLimit; when most overflowed, what they held is unknown, so for the
// worst case, one distinct element per record.
void distinct_ratio_after_overflow(syzsig_ctx* ctx, uint64_t P, uint64_t novf, uint64_t D, uint64_t recs)
{
	const double seen = novf * 2 >= P ? (double)recs : (double)D + 2.0 * (double)novf * kAggLimit;
	ctx->agg_distinct_ratio = std::max(ctx->agg_distinct_ratio, seen / (double)std::max<uint64_t>(recs, 1));
}

// With timing on: the device times between the context's recorded events
// ev[first] .. ev[last] into st -- ev[0..1] partitioning, ev[1..2] k_agg,
// ev[2..3] the finalize.  After the synchronisation that follows them.
int stage_times(syzsig_ctx* ctx, int first, int last, syzsig_batch_stats* st)
{
	double* const ms[3] = {&st->part_ms, &st->probe_ms, &st->decide_ms};
	for (int i = first; ctx->timing && i < last; i++) {
		float t = 0;
		SYZ_HIP(hipEventElapsedTime(&t, ctx->ev[i], ctx->ev[i + 1]));
		*ms[i] += t;
	}
	return SYZSIG_OK;
}

static int agg_capped(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t c0, uint64_t c1, const LevelMap& lm,
                      uint64_t run_recs, const AggGeom& g, const AggSrc* xp, syzsig_batch_stats* st, AggOut* out,
                      bool* done)
{
	*done = false;
	const uint32_t P = 1u << g.pbits;
	const bool tight = ctx->agg_dbg & SYZSIG_DEBUG_CAP_SPILL;
	float& slack = xp ? ctx->cap_sd_entry : ctx->cap_sd;
	CapRun r;
	SYZ_TRY(cap_layout(ctx, run_recs, nchunks_of(c1 - c0, g.ibits), P, tight ? 0.0f : slack, &r));
	const hipStream_t s = ctx->stream;
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[0], s));
	const uint32_t tile = xp ? kScat3TileEntry : kScat3Tile;
	SYZ_TRY(cap_plan(ctx, b, c0, c1, lm, g, run_recs, &r, tile));
	SYZ_TRY(cap_scatter_agg(ctx, b, c0, c1, lm, g, r, tile, xp, nullptr, ctx->ev));
	uint32_t* hov = (uint32_t*)(ctx->h_pin + kPinCounts);
	uint32_t* hcp = hov + 16;
	SYZ_HIP(hipMemcpyAsync(hcp, r.dc, P * 4, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipMemcpyAsync(hov, r.ovf, 4, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipStreamSynchronize(s));
	SYZ_TRY(stage_times(ctx, 0, 2, st));
	if (*hov) {
		st->retries++;
		if (!tight)
			cap_slack_after_spill(slack);
		return SYZSIG_OK;
	}
	uint64_t D = 0;
	for (uint32_t p = 0; p < P; p++) {
		if (hcp[p] == kAggOverflow) {
			st->retries++;
			return SYZSIG_OK;
		}
		D += hcp[p];
	}
	st->distinct += D;
	st->parts = P;
	st->survivors += D;
	if (!xp)
		ctx->agg_distinct_ratio = run_recs ? (double)D / (double)run_recs : 0;
	*out = AggOut{(const uint32_t*)r.de, (const uint4*)r.df, (const uint32_t*)r.dc, P, P, D};
	*done = true;
	return SYZSIG_OK;
}

// The HBM fallback for the partitions `ovl` (ovrec records in all) that
// overflowed the LDS table: launch(ol, gk, gf, C, err) aggregates their cells
// into the table (gk, gf) of C slots -- k_agg_global or k_agg_global_cap over
// the device copy ol of ovl, raising *err on an internal error -- and the
// table's distinct list is compacted to (dist_e, dist_f), which hold at least
// ovrec entries.  *gcnt = its length, also appended to *rc in pieces of
// kAggRegion.  Resets the counters; synchronises.
template <typename Launch>
static int agg_hbm_fallback(syzsig_ctx* ctx, const std::vector<uint32_t>& ovl, uint64_t ovrec, uint32_t* dist_e,
                            uint4* dist_f, Launch launch, uint64_t* gcnt, std::vector<uint32_t>* rc)
{
	const hipStream_t s = ctx->stream;
	const uint64_t C = pow2_at_least(std::max<uint64_t>(2 * ovrec, 1024));
	void *gk, *ol;
	SYZ_TRY(ws_get(ctx, kWsAggHbmTable, C * 4 + (C + 1) * 16 + 64, &gk));
	uint32_t* gf = (uint32_t*)((char*)gk + C * 4);
	SYZ_TRY(ws_get(ctx, kWsAggOvfList, ovl.size() * 4 + 64, &ol));
	SYZ_HIP(hipMemsetAsync(gk, 0xff, C * 4 + (C + 1) * 16, s));
	SYZ_HIP(hipMemcpyAsync(ol, ovl.data(), ovl.size() * 4, hipMemcpyHostToDevice, s));
	SYZ_TRY(counters_reset(ctx));
	launch((const uint32_t*)ol, (uint32_t*)gk, gf, C, &ctx->d_cnt[kCntError]);
	k_agg_global_compact<<<grid_for(C + 1, 256, 8192), 256, 0, s>>>((const uint32_t*)gk, gf, C, dist_e, dist_f,
	                                                                 &ctx->d_cnt[kCntAux2]);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "triage: aggregation table overflow (internal error)");
	*gcnt = ctx->h_cnt[kCntAux2];
	for (uint64_t left = *gcnt; left; left -= std::min<uint64_t>(left, kAggRegion))
		rc->push_back((uint32_t)std::min<uint64_t>(left, kAggRegion));
	return SYZSIG_OK;
}

// Count, scatter and aggregate (plus the HBM fallback) one run of calls
// [c0, c1) with level map lm: every distinct element of the run with its level
// firsts (run serials), in regions of kAggRegion entries.  A triage run tries
// capped cells first (agg_capped), counted cells are the exact path.
int agg_aggregate(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t c0, uint64_t c1, const LevelMap& lm,
                  uint64_t run_recs, syzsig_batch_stats* st, AggOut* out, const AggSrc* xp)
{
	const AggSrc x = xp ? *xp : AggSrc{nullptr, 1, 0, 0};
	const bool entry = xp != nullptr;
	// Minimize: fuller LDS tables, so half the partitions and whole 128-B
	// scatter blocks (C3: 2.70-2.78 -> 2.65 ms; a triage run's finalize and
	// k_agg lose more than its scatter gains)
	AggGeom g = agg_geom_for(ctx, run_recs, x.distinct_hint, entry ? kAggTargetLoadEntry : kAggTargetLoad);
	const uint32_t P = 1u << g.pbits;
	const uint64_t nchunks = (c1 - c0 + (1ull << g.cbits()) - 1) >> g.cbits();
	// Work items of the count/scatter: whole chunks for a batch (its calls are
	// alike), smaller ones for Minimize, whose calls (contexts in Len-desc
	// order) make the first chunks far heavier than the last: >= ~2048 items.
	g.ibits = g.cbits();
	if (entry)
		while (g.ibits > 0 && ((c1 - c0) >> g.ibits) < kMinItems)
			g.ibits--;
	const bool counted_once = ctx->agg_counted_once;
	ctx->agg_counted_once = false;
	if (((entry ? ctx->cap_sd_entry : ctx->cap_sd) > 0 || (ctx->agg_dbg & SYZSIG_DEBUG_CAP_SPILL)) &&
	    !(ctx->agg_dbg & SYZSIG_DEBUG_EXACT_CELLS) && !counted_once) {
		bool done = false;
		SYZ_TRY(agg_capped(ctx, b, c0, c1, lm, run_recs, g, xp, st, out, &done));
		if (done)
			return SYZSIG_OK;
	}
	const uint32_t ilog = g.items_per_chunk_log2();
	const uint64_t nitems = (c1 - c0 + (1ull << g.ibits) - 1) >> g.ibits;
	void *recs, *cm, *pm, *de, *df, *dc;
	SYZ_TRY(ws_get(ctx, kWsAggRecs, run_recs * 4 + 64, &recs));
	SYZ_TRY(ws_get(ctx, kWsAggCells, (2 * nitems * P + (uint64_t)P * (nchunks + 1)) * 4 + 64, &cm));
	SYZ_TRY(ws_get(ctx, kWsAggTotals, (kAggMaxParts + 1) * 8 * 2, &pm));
	uint32_t* counts = (uint32_t*)cm;
	uint32_t* offs = counts + nitems * P;
	uint32_t* offsT = offs + nitems * P;
	uint64_t* totals = (uint64_t*)pm;
	uint64_t* rec_base = totals + kAggMaxParts + 1;
	const hipStream_t s = ctx->stream;
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[0], s));
	const int pg = (int)std::min<uint64_t>(nitems, 2048);
	if (x.nshards > 1)
		k_agg_count<true><<<pg, kAggThreads, 0, s>>>(b->sigs, b->call_start, b->call_len, c0, c1, g, x, counts);
	else
		k_agg_count<false><<<pg, kAggThreads, 0, s>>>(b->sigs, b->call_start, b->call_len, c0, c1, g, x, counts);
	k_agg_scan_chunks<<<P, 1024, 0, s>>>(counts, nitems, ilog, P, offs, offsT, totals);
	k_agg_scan_totals<<<1, 1024, 0, s>>>(totals, P, rec_base);
	if (entry)
		k_agg_scatter<true><<<pg, kAggThreads, 0, s>>>(b->sigs, b->call_start, b->call_len, b->call_prio, lm, c0, c1,
		                                               g, x, offs, rec_base, (uint32_t*)recs);
	else
		k_agg_scatter<false><<<pg, kAggThreads, 0, s>>>(b->sigs, b->call_start, b->call_len, b->call_prio, lm, c0, c1,
		                                                g, x, offs, rec_base, (uint32_t*)recs);
	SYZ_HIP(hipGetLastError());
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[1], s));
	// aggregation
	SYZ_TRY(agg_lists(ctx, P, &de, &df, &dc));
	const AggCells xc{(const uint32_t*)recs, rec_base, offsT, nullptr, nullptr, nullptr, nchunks, 0,
	                  agg_group_size(nchunks)};
	launch_agg<false>(ctx, run_recs, P, s, xc, g, de, df, dc);
	SYZ_HIP(hipGetLastError());
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[2], s));
	static_assert(kPinCounts + kAggMaxParts * 4 + (kAggMaxParts + 1) * 8 <= kPinBytes, "pinned staging");
	uint64_t* hbp = (uint64_t*)(ctx->h_pin + kPinCounts);
	uint32_t* hcp = (uint32_t*)(hbp + kAggMaxParts + 1);
	SYZ_HIP(hipMemcpyAsync(hcp, dc, P * 4, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipMemcpyAsync(hbp, rec_base, (P + 1) * 8, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipStreamSynchronize(s));
	const std::vector<uint32_t> hc(hcp, hcp + P);
	const std::vector<uint64_t> hb(hbp, hbp + P + 1);
	SYZ_TRY(stage_times(ctx, 0, 2, st));
	uint64_t D = 0, ovrec = 0;
	std::vector<uint32_t> ovl;
	for (uint32_t p = 0; p < P; p++) {
		if (hc[p] == kAggOverflow) {
			ovl.push_back(p);
			ovrec += hb[p + 1] - hb[p];
		} else {
			D += hc[p];
		}
	}
	uint32_t nregions = P;
	void* dist_e = de;
	void* dist_f = df;
	if (!ovl.empty()) {
		// fallback: HBM aggregation table for the overflowed partitions; their
		// distinct list is appended as extra regions after the P LDS regions
		const uint64_t extra_regions = (ovrec + kAggRegion - 1) / kAggRegion + 1;
		// distinct lists must be contiguous with the regions: a bigger pair, the LDS part copied in front
		const uint64_t tot_e = ((uint64_t)P + extra_regions) * kAggRegion;
		void *de2, *df2;
		SYZ_TRY(ws_get(ctx, kWsAggDistE2, tot_e * 4 + 64, &de2));
		SYZ_TRY(ws_get(ctx, kWsAggDistF2, tot_e * 16 + 64, &df2));
		SYZ_HIP(hipMemcpyAsync(de2, de, (uint64_t)P * kAggRegion * 4, hipMemcpyDeviceToDevice, s));
		SYZ_HIP(hipMemcpyAsync(df2, df, (uint64_t)P * kAggRegion * 16, hipMemcpyDeviceToDevice, s));
		// region counts: LDS partitions (overflowed = 0), then the fallback list in kAggRegion pieces
		std::vector<uint32_t> rc(hc);
		for (uint32_t p : ovl)
			rc[p] = 0;
		const uint64_t items = ovl.size() * ((nchunks + kAggGroup - 1) / kAggGroup);
		const auto launch = [&](const uint32_t* ol, uint32_t* gk, uint32_t* gf, uint64_t C, unsigned long long* err) {
			k_agg_global<<<grid_for(items * 64, 256, 8192), 256, 0, s>>>((const uint32_t*)recs, rec_base,
			                                                              (const uint32_t*)offsT, nchunks, g, ol,
			                                                              (uint32_t)ovl.size(), gk, gf, C, err);
		};
		uint64_t gcnt = 0;
		SYZ_TRY(agg_hbm_fallback(ctx, ovl, ovrec, (uint32_t*)de2 + (uint64_t)P * kAggRegion,
		                         (uint4*)df2 + (uint64_t)P * kAggRegion, launch, &gcnt, &rc));
		D += gcnt;
		nregions = (uint32_t)rc.size();
		void* dc2;
		SYZ_TRY(ws_get(ctx, kWsAggCnt, rc.size() * 4 + 64, &dc2));
		SYZ_HIP(hipMemcpyAsync(dc2, rc.data(), rc.size() * 4, hipMemcpyHostToDevice, s));
		SYZ_HIP(hipStreamSynchronize(s));  // rc is a host temporary
		dc = dc2;
		dist_e = de2;
		dist_f = df2;
		st->overflow_parts += ovl.size();
	}
	st->distinct += D;
	st->parts = P;
	st->survivors += D;
	if (!entry)
		ctx->agg_distinct_ratio = run_recs ? (double)D / (double)run_recs : 0;
	*out = AggOut{(const uint32_t*)dist_e, (const uint4*)dist_f, (const uint32_t*)dc, nregions, P, D};
	return SYZSIG_OK;
}

// Distinct elements per partition (top pbits of fmix32) over regions [r0, r1).
__global__ __launch_bounds__(256) void k_part_hist(const uint32_t* __restrict__ dist_e,
                                                   const uint32_t* __restrict__ cnt, uint32_t r0, uint32_t r1,
                                                   uint32_t pbits, uint32_t* hist)
{
	for (uint32_t r = r0 + blockIdx.x; r < r1; r += gridDim.x) {
		const uint32_t n = cnt[r] == kAggOverflow ? 0 : cnt[r];
		for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
			atomicAdd(&hist[fmix32(dist_e[(uint64_t)r * kAggRegion + i]) >> (32 - pbits)], 1u);
	}
}

// The finalize probes a partition's elements from its own slice of a table
// (home buckets = the top bits of the same h).  The HBM fallback's partitions
// hold more than kAggLimit distinct elements, possibly many more when the
// elements are not spread by the hash: their slice must take them at most 3/4
// full, or their probe sequences pile up past the probe limit.  Grows s so
// that every such partition's slice does.  Synchronises.
static int reserve_slices(syzsig_ctx* ctx, syzsig_set* s, const uint32_t* dist_e, const uint32_t* d_cnt, uint32_t r0,
                          uint32_t r1, uint32_t pbits)
{
	if (!s || r1 <= r0)
		return SYZSIG_OK;
	const uint32_t P = 1u << pbits;
	void* wh;
	SYZ_TRY(ws_get(ctx, kWsPartHist, (uint64_t)P * 4 + 64, &wh));
	const hipStream_t st = ctx->stream;
	SYZ_HIP(hipMemsetAsync(wh, 0, (uint64_t)P * 4, st));
	k_part_hist<<<std::min<uint32_t>(r1 - r0, 2048), 256, 0, st>>>(dist_e, d_cnt, r0, r1, pbits, (uint32_t*)wh);
	SYZ_HIP(hipGetLastError());
	std::vector<uint32_t> h(P);
	SYZ_HIP(hipMemcpyAsync(h.data(), wh, (uint64_t)P * 4, hipMemcpyDeviceToHost, st));
	SYZ_HIP(hipStreamSynchronize(st));
	const uint64_t mx = *std::max_element(h.begin(), h.end());
	const uint64_t need = pow2_at_least((uint64_t)((double)P * (double)mx / (kBucketSlots * kMaxLoad)) + 1);
	if (need > s->nbuckets)
		SYZ_TRY(set_rehash(s, need, false));
	return SYZSIG_OK;
}

// Zero the counters, with the pair cursor (kCntAux2) at npairs: the finalize
// kernels append the run's pairs after the batch's earlier ones.
static int seed_pair_counter(syzsig_ctx* ctx, uint64_t npairs)
{
	SYZ_TRY(counters_reset(ctx));
	memcpy(ctx->h_pin + kPinPairs, &npairs, 8);  // consumed before the caller's next counters_fetch
	SYZ_HIP(hipMemcpyAsync(&ctx->d_cnt[kCntAux2], ctx->h_pin + kPinPairs, 8, hipMemcpyHostToDevice, ctx->stream));
	return SYZSIG_OK;
}

// What every finalize kernel takes: the run, the two tables, the outputs.
static FinArgs fin_tables(syzsig_ctx* ctx, const syzsig_set* ms, const syzsig_set* nsp, const LevelMap& lm, uint64_t c0,
                          const syzsig_batch* b, uint64_t* pairs)
{
	FinArgs fa{};
	fa.lm = lm;
	fa.c0 = c0;
	fa.slots = ms->slots;
	fa.bmask = ms->nbuckets - 1;
	fa.ns_slots = nsp->slots;
	fa.ns_bmask = nsp->nbuckets - 1;
	fa.call_new = b->call_new;
	fa.pairs = pairs;
	fa.npairs = &ctx->d_cnt[kCntAux2];
	fa.ctr = ctx->d_cnt;
	return fa;
}

// The slice-exclusive finalize's arguments for a run of 2^pbits partitions and
// at most n distinct elements (the deferred lists' capacity): both tables have
// at least a bucket per partition.
static int fin_args(syzsig_ctx* ctx, const syzsig_set* ms, const syzsig_set* nsp, uint32_t pbits, const LevelMap& lm,
                    uint64_t c0, const syzsig_batch* b, uint64_t* pairs, uint64_t n, FinArgs* fa)
{
	void *dd, *dn;
	SYZ_TRY(ws_get(ctx, kWsFinDefer, n * 20 + 64, &dd));
	SYZ_TRY(ws_get(ctx, kWsFinDeferNs, n * 8 + 64, &dn));
	*fa = fin_tables(ctx, ms, nsp, lm, c0, b, pairs);
	fa->ms_shift = (63 - __builtin_clzll(ms->nbuckets)) - pbits;
	fa->ns_shift = (63 - __builtin_clzll(nsp->nbuckets)) - pbits;
	fa->def_e = (uint32_t*)dd;
	fa->def_f = (uint4*)((char*)dd + ((n * 4 + 15) & ~15ull));
	fa->def_cnt = &ctx->d_cnt[kCntDefer];
	fa->def_ns = (uint64_t*)dn;
	fa->def_ns_cnt = &ctx->d_cnt[kCntDeferNs];
	fa->dbg = ctx->agg_dbg;
	return SYZSIG_OK;
}

// The slice-exclusive finalize over the regions (all partitions), then the
// deferred lists.
// (The deferred lists in a launch of their own: taken by the finalize's last
// block instead, they made the finalize 1.03 ms instead of 0.27 at C2.)
static int fin_launch(syzsig_ctx* ctx, const FinArgs& fa, const uint32_t* dist_e, const uint4* dist_f,
                      const uint32_t* cnt, uint32_t nregions)
{
	const hipStream_t s = ctx->stream;
	k_agg_finalize_x<2><<<nregions, kFxThreads, 0, s>>>(dist_e, dist_f, cnt, nregions, fa);
	SYZ_HIP(hipGetLastError());
	k_fin_deferred<<<2 * kDeferBlocks, 256, 0, s>>>(fa);
	SYZ_HIP(hipGetLastError());
	return SYZSIG_OK;
}

// The atomic finalize over any regions and tables (newSignal exists: the
// callers have distinct elements to commit).
static int fin_launch_atomic(syzsig_ctx* ctx, const syzsig_set* ms, const syzsig_set* nsp, const LevelMap& lm,
                             uint64_t c0, const syzsig_batch* b, uint64_t* pairs, const uint32_t* dist_e,
                             const uint4* dist_f, const uint32_t* cnt, uint32_t nregions)
{
	k_agg_finalize<<<nregions, kFinThreads, 0, ctx->stream>>>(dist_e, dist_f, cnt, nregions,
	                                                          fin_tables(ctx, ms, nsp, lm, c0, b, pairs));
	SYZ_HIP(hipGetLastError());
	return SYZSIG_OK;
}

// One triage run with one host synchronisation at the end ("the
// one-sync triage run"): scatter into capped cells, k_agg, the slice-exclusive
// finalize and the deferred lists.  maxSignal and newSignal are reserved for
// the run's largest possible distinct count D_max = min(records, P * kAggLimit)
// (a growth only when len + D_max would pass 90 % of the table; the usual
// policy loads apply to the expected count), so the kernels never wait for
// the host.  fast: the caller skipped the presence pass (k_fast_prep checks its
// assumptions).  *done = false: nothing was committed (*assumed_bad: the
// assumptions failed; *regeom: too few partitions, redo; else a cell spilled:
// counted cells next, the slack doubled).
static int agg_triage_fused(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const syzsig_batch* b, uint64_t c0,
                            uint64_t c1, const LevelMap& lm, uint64_t run_recs, syzsig_batch_stats* st,
                            uint64_t** pairs_out, uint64_t* npairs_io, bool* done, bool fast, bool* assumed_bad,
                            bool* regeom)
{
	*done = *regeom = *assumed_bad = false;
	AggGeom g = agg_geom_for(ctx, run_recs, 0);
	g.ibits = g.cbits();  // work items are whole chunks
	const uint32_t S = 1u << g.pbits, P = S;
	const uint64_t nchunks = nchunks_of(c1 - c0, g.ibits);
	// distinct elements the run can commit: an LDS partition holds at
	// most kAggLimit (one that overflows is committed after the sync)
	const uint64_t d_max = std::min<uint64_t>(run_recs, (uint64_t)P * kAggLimit);
	const double ratio = ctx->agg_distinct_ratio > 0 ? ctx->agg_distinct_ratio : 1.0 / 32;
	const uint64_t d_est = std::min<uint64_t>(d_max, (uint64_t)(ratio * (double)run_recs) + 1);
	// capacity for every possible change, before anything is committed
	SYZ_TRY(set_reserve(ms, d_est));
	SYZ_TRY(set_reserve_load(ms, d_max, kHardLoad));
	FreshNs fresh(ns, !*ns);
	if (fresh.armed)
		SYZ_TRY(syzsig_set_make(ctx, d_est, ns));
	syzsig_set* nsp = *ns;
	// at most half full for the expected changes (short probe chains: 0.34 ->
	// 0.28 ms at C2), never past kHardLoad for the largest possible count
	SYZ_TRY(set_reserve_load(nsp, d_est, kTargetLoad));
	SYZ_TRY(set_reserve_load(nsp, d_max, kHardLoad));
	if (ms->nbuckets < P || nsp->nbuckets < P)  // slices need a bucket per partition
		return SYZSIG_OK;
	CapRun r;
	SYZ_TRY(cap_layout(ctx, run_recs, nchunks, S, ctx->cap_sd, &r));
	void* pr;
	if (fast && *npairs_io == 0 && b->new_pairs && b->new_pairs_cap >= 4 * d_max) {
		pr = b->new_pairs;  // every possible pair fits the caller's buffer: no copy afterwards
	} else {
		SYZ_TRY(ws_grow_keep(ctx, kWsPairs, (*npairs_io + 4 * d_max) * 8 + 64, *npairs_io * 8, &pr));
	}
	*pairs_out = (uint64_t*)pr;
	const uint32_t pb = g.pbits;
	FinArgs fa;
	SYZ_TRY(fin_args(ctx, ms, nsp, pb, lm, c0, b, (uint64_t*)pr, d_max, &fa));
	const hipStream_t s = ctx->stream;
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[0], s));
	if (fast) {
		// per-chunk sizes and checks (call_new zeroed too), then the cell plan,
		// which also zeroes the counters and sets the run's void flag
		SYZ_TRY(cap_plan(ctx, b, c0, c1, lm, g, run_recs, &r, kScat3Tile, ctx->d_cnt, *npairs_io));
	} else {
		SYZ_TRY(seed_pair_counter(ctx, *npairs_io));
		SYZ_TRY(cap_plan(ctx, b, c0, c1, lm, g, run_recs, &r, kScat3Tile));
	}
	// k_agg's distinct lists go through HBM (5 M x 20 B at C2) to the
	// slice-exclusive finalize: a workgroup of the finalize is small, so many
	// run per CU and their random probes overlap
	SYZ_TRY(cap_scatter_agg(ctx, b, c0, c1, lm, g, r, kScat3Tile, nullptr, ctx->d_cnt, ctx->ev));
	// more overflowed partitions than this and the split path commits nothing:
	// the run is redone with partitions sized from what k_agg counted
	const uint32_t gate = P / 8;
	fa.spill = r.ovf;
	fa.ovf_gate = &ctx->d_cnt[kCntAggOvf];
	fa.gate_max = gate;
	SYZ_TRY(fin_launch(ctx, fa, (const uint32_t*)r.de, (const uint4*)r.df, (const uint32_t*)r.dc, P));
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[3], s));
	uint32_t* hov = (uint32_t*)(ctx->h_pin + kPinCounts);
	if (!fast)
		SYZ_HIP(hipMemcpyAsync(hov, r.ovf, 4, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));  // the run's one synchronisation
	if (fast) {
		*hov = (uint32_t)ctx->h_cnt[kCntSpill];
		st->records = ctx->h_cnt[kCntRecords];
	}
	SYZ_TRY(stage_times(ctx, 0, 3, st));
	if (*hov & 6) {  // an optimistic run's assumptions failed: nothing committed
		*assumed_bad = true;
		return SYZSIG_OK;
	}
	if (*hov) {  // a cell spilled: nothing committed, redo with counted cells
		st->retries++;
		cap_slack_after_spill(ctx->cap_sd);
		return SYZSIG_OK;
	}
	if (ctx->h_cnt[kCntOverflow])
		return fail(SYZSIG_EIO, "triage: table overflow after reserve (internal error; one-sync run)");
	uint64_t D = ctx->h_cnt[kCntDistinct];
	uint64_t inserted = ctx->h_cnt[kCntInserted], changed = ctx->h_cnt[kCntChanged], ns_ins = ctx->h_cnt[kCntAux];
	uint64_t inserted_done = 0;  // already added to maxSignal's length
	uint64_t npairs = ctx->h_cnt[kCntAux2];
	const uint64_t novf = ctx->h_cnt[kCntAggOvf];
	if (novf > gate) {
		// too few partitions: nothing was committed; the next attempt sizes them
		// for at least what was seen
		distinct_ratio_after_overflow(ctx, P, novf, D, run_recs);
		st->retries++;
		*regeom = true;
		return SYZSIG_OK;
	}
	if (novf) {
		// partitions past the LDS table: aggregated in HBM from their cells,
		// then finalized with the atomic code (their elements are disjoint from
		// every committed partition's).  The committed partitions' inserts count
		// first: the reservations below start from the tables' true lengths.
		ms->len += inserted;
		nsp->len += ns_ins;
		inserted_done += inserted;
		inserted = ns_ins = 0;
		std::vector<uint32_t> hc(P);
		SYZ_HIP(hipMemcpy(hc.data(), r.dc, P * 4, hipMemcpyDeviceToHost));
		std::vector<uint32_t> ovl;
		uint64_t ovrec = 0;
		std::vector<uint32_t> hcnt((uint64_t)P * nchunks);
		SYZ_HIP(hipMemcpy(hcnt.data(), r.ccnt, hcnt.size() * 4, hipMemcpyDeviceToHost));
		for (uint32_t q = 0; q < P; q++) {
			if (hc[q] != kAggOverflow)
				continue;
			ovl.push_back(q);
			for (uint64_t c = 0; c < nchunks; c++)
				ovrec += hcnt[(uint64_t)q * nchunks + c];
		}
		void *de2, *df2, *dc2;
		SYZ_TRY(ws_get(ctx, kWsAggDistE2, ovrec * 4 + 64, &de2));
		SYZ_TRY(ws_get(ctx, kWsAggDistF2, ovrec * 16 + 64, &df2));
		const auto launch = [&](const uint32_t* ol, uint32_t* gk, uint32_t* gf, uint64_t C, unsigned long long* err) {
			k_agg_global_cap<<<grid_for(ovl.size() * nchunks * 64, 256, 8192), 256, 0, s>>>(
			    r.recs, r.cbase, r.ccap, r.ccnt, nchunks, g, ol, (uint32_t)ovl.size(), gk, gf, C, err);
		};
		uint64_t gcnt = 0;
		std::vector<uint32_t> rc;
		SYZ_TRY(agg_hbm_fallback(ctx, ovl, ovrec, (uint32_t*)de2, (uint4*)df2, launch, &gcnt, &rc));
		D += gcnt;
		if (!rc.empty()) {
			// the reservations above covered the committed partitions (<= kAggLimit
			// distinct each); these elements come on top
			SYZ_TRY(set_reserve(ms, gcnt));
			SYZ_TRY(set_reserve_load(nsp, gcnt, kHardLoad));
			SYZ_TRY(ws_get(ctx, kWsAggHbmCnt, rc.size() * 4 + 64, &dc2));
			SYZ_HIP(hipMemcpyAsync(dc2, rc.data(), rc.size() * 4, hipMemcpyHostToDevice, s));
			SYZ_TRY(reserve_slices(ctx, ms, (const uint32_t*)de2, (const uint32_t*)dc2, 0, (uint32_t)rc.size(), pb));
			SYZ_TRY(reserve_slices(ctx, nsp, (const uint32_t*)de2, (const uint32_t*)dc2, 0, (uint32_t)rc.size(), pb));
			if (pr == b->new_pairs) {
				// the run wrote its pairs straight into the caller's buffer: keep
				// appending there while it has room, else move them to kWsPairs
				// first (ws_grow_keep keeps only what that workspace held)
				if (b->new_pairs_cap < npairs + 4 * gcnt) {
					void* w;
					SYZ_TRY(ws_get(ctx, kWsPairs, (npairs + 4 * gcnt) * 8 + 64, &w));
					if (npairs)
						SYZ_HIP(hipMemcpyAsync(w, pr, npairs * 8, hipMemcpyDeviceToDevice, s));
					pr = w;
				}
			} else {
				SYZ_TRY(ws_grow_keep(ctx, kWsPairs, (npairs + 4 * gcnt) * 8 + 64, npairs * 8, &pr));
			}
			*pairs_out = (uint64_t*)pr;
			SYZ_TRY(seed_pair_counter(ctx, npairs));
			SYZ_TRY(fin_launch_atomic(ctx, ms, nsp, lm, c0, b, (uint64_t*)pr, (const uint32_t*)de2, (const uint4*)df2,
			                          (const uint32_t*)dc2, (uint32_t)rc.size()));
			SYZ_TRY(counters_fetch(ctx));  // (synchronizes: rc is consumed)
			if (ctx->h_cnt[kCntOverflow])
				return fail(SYZSIG_EIO, "triage: table overflow after reserve (internal error; one-sync run, HBM partitions)");
			inserted += ctx->h_cnt[kCntInserted];
			changed += ctx->h_cnt[kCntChanged];
			ns_ins += ctx->h_cnt[kCntAux];
			npairs = ctx->h_cnt[kCntAux2];
		}
		st->overflow_parts += novf;
	}
	commit_run(ms, nsp, fresh, inserted, changed, ns_ins, st);
	st->inserted += inserted_done;
	st->distinct += D;
	st->parts = P;
	st->survivors += D;
	ctx->agg_distinct_ratio = run_recs ? (double)D / (double)run_recs : 0;
	*npairs_io = npairs;
	*done = true;
	return SYZSIG_OK;
}

// The one-sync run where capped cells are in use, attempted once more when the
// first attempt asks for more partitions.  *done = false with agg_counted_once
// set after a spilled cell: the run is redone with counted cells, not capped
// ones again.
static int agg_triage_one_sync(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const syzsig_batch* b, uint64_t c0,
                               uint64_t c1, const LevelMap& lm, uint64_t run_recs, syzsig_batch_stats* st,
                               uint64_t** pairs, uint64_t* npairs, bool fast, bool* done)
{
	*done = false;
	if (ctx->cap_sd <= 0 || ctx->agg_counted_once ||
	    (ctx->agg_dbg & (SYZSIG_DEBUG_EXACT_CELLS | SYZSIG_DEBUG_CAP_SPILL)))
		return SYZSIG_OK;
	bool bad = false, regeom = false;
	uint64_t retries0 = st->retries;
	SYZ_TRY(agg_triage_fused(ctx, ms, ns, b, c0, c1, lm, run_recs, st, pairs, npairs, done, fast, &bad, &regeom));
	if (regeom) {  // once more with partitions for what the first attempt counted
		retries0 = st->retries;
		SYZ_TRY(agg_triage_fused(ctx, ms, ns, b, c0, c1, lm, run_recs, st, pairs, npairs, done, fast, &bad, &regeom));
	}
	ctx->agg_counted_once = !*done && st->retries != retries0;
	return SYZSIG_OK;
}

// One run of calls [c0, c1) with level map lm.  Pairs are appended at
// pairs[*npairs_io ...] (internal buffer, grown as needed).
int agg_triage_run(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const syzsig_batch* b, uint64_t c0, uint64_t c1,
                   const LevelMap& lm, uint64_t run_recs, syzsig_batch_stats* st, uint64_t** pairs_out,
                   uint64_t* npairs_io)
{
	bool done = false;
	SYZ_TRY(agg_triage_one_sync(ctx, ms, ns, b, c0, c1, lm, run_recs, st, pairs_out, npairs_io, false, &done));
	if (done)
		return SYZSIG_OK;
	AggOut a;
	SYZ_TRY(agg_aggregate(ctx, b, c0, c1, lm, run_recs, st, &a));
	const uint64_t D = a.D;
	const hipStream_t s = ctx->stream;
	void* pr;
	// capacity for every possible change, then finalize (never retried)
	SYZ_TRY(set_reserve(ms, D));
	FreshNs fresh(ns, D && !*ns);
	if (fresh.armed)
		SYZ_TRY(syzsig_set_make(ctx, D, ns));
	// newSignal takes up to D changes per batch: kept at most half full, so its
	// probe chains stay short in the finalize (0.34 -> 0.28 ms at C2)
	if (D)
		SYZ_TRY(set_reserve_load(*ns, D, kTargetLoad));
	if (a.nregions > a.parts) {  // the HBM fallback's partitions: room in their slices
		const uint32_t pb = 31 - __builtin_clz(a.parts);
		SYZ_TRY(reserve_slices(ctx, ms, a.dist_e, a.cnt, a.parts, a.nregions, pb));
		SYZ_TRY(reserve_slices(ctx, *ns, a.dist_e, a.cnt, a.parts, a.nregions, pb));
	}
	const uint64_t need_pairs = *npairs_io + 4 * D;
	SYZ_TRY(ws_grow_keep(ctx, kWsPairs, need_pairs * 8 + 64, *npairs_io * 8, &pr));
	*pairs_out = (uint64_t*)pr;
	SYZ_TRY(seed_pair_counter(ctx, *npairs_io));
	syzsig_set* nsp = *ns;
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[2], s));
	// the slice-exclusive finalize when every region is a partition and both
	// tables have at least one bucket per partition; else the atomic one
	const bool fx = D && a.nregions == a.parts && ms->nbuckets >= a.parts && nsp->nbuckets >= a.parts;
	if (fx) {
		FinArgs fa;
		SYZ_TRY(fin_args(ctx, ms, nsp, 31 - __builtin_clz(a.parts), lm, c0, b, (uint64_t*)pr, D, &fa));
		SYZ_TRY(fin_launch(ctx, fa, a.dist_e, a.dist_f, a.cnt, a.nregions));
	} else if (D) {
		SYZ_TRY(fin_launch_atomic(ctx, ms, nsp, lm, c0, b, (uint64_t*)pr, a.dist_e, a.dist_f, a.cnt, a.nregions));
	}
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev[3], s));
	SYZ_TRY(counters_fetch(ctx));
	SYZ_TRY(stage_times(ctx, 2, 3, st));
	if (ctx->h_cnt[kCntOverflow])
		return fail(SYZSIG_EIO, "triage: table overflow after reserve (internal error; planned run)");
	commit_run(ms, nsp, fresh, ctx->h_cnt[kCntInserted], ctx->h_cnt[kCntChanged], ctx->h_cnt[kCntAux], st);
	*npairs_io = ctx->h_cnt[kCntAux2];
	return SYZSIG_OK;
}

int agg_triage_optimistic(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const syzsig_batch* b,
                          syzsig_batch_stats* st, uint64_t** pairs, uint64_t* npairs, bool* done)
{
	LevelMap lm;
	const int8_t lv[4] = {0, 1, 2, 3};
	SYZ_TRY(level_map_from_levels(lv, 4, &lm));
	return agg_triage_one_sync(ctx, ms, ns, b, 0, b->ncalls, lm, b->nrec, st, pairs, npairs, true, done);
}

// Per-record bits of calls [c0, c1) from the run's pairs [p0, p1).
int agg_mark_bits(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t c0, uint64_t c1, const uint64_t* pairs,
                  uint64_t p0, uint64_t p1)
{
	if (p1 == p0 || !b->new_bits)
		return SYZSIG_OK;
	const uint64_t n = p1 - p0, C = pow2_at_least(2 * n + 16);
	void* set;
	SYZ_TRY(ws_get(ctx, kWsPairSet, C * 8, &set));
	const hipStream_t s = ctx->stream;
	SYZ_HIP(hipMemsetAsync(set, 0xff, C * 8, s));
	SYZ_TRY(counters_reset(ctx));
	k_pairs_set<<<grid_for(n, 256, 8192), 256, 0, s>>>(pairs + p0, n, (uint64_t*)set, C, &ctx->d_cnt[kCntAux]);
	k_pairs_mark<<<grid_for((c1 - c0) * 64, 256, 8192), 256, 0, s>>>(b->sigs, b->call_start, b->call_len, c0, c1,
	                                                                  b->call_new, (const uint64_t*)set, C, b->new_bits);
	SYZ_HIP(hipGetLastError());
	return SYZSIG_OK;
}

// Pairs of the per-call path from its bits: collect, then dedup through a set.
int pairs_from_bits(syzsig_ctx* ctx, const syzsig_batch* b, const uint32_t* bits, uint64_t c0, uint64_t c1,
                    uint64_t bound, uint64_t** pairs_io, uint64_t* npairs_io)
{
	const hipStream_t s = ctx->stream;
	void *raw, *set, *out;
	SYZ_TRY(ws_get(ctx, kWsPairsRaw, bound * 8 + 64, &raw));
	SYZ_TRY(counters_reset(ctx));
	k_bits_to_pairs<<<grid_for((c1 - c0) * 64, 256, 8192), 256, 0, s>>>(b->sigs, b->call_start, b->call_len, c0, c1,
	                                                                     b->call_new, bits, (uint64_t*)raw,
	                                                                     &ctx->d_cnt[kCntAux]);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	const uint64_t n = ctx->h_cnt[kCntAux];
	if (n == 0)
		return SYZSIG_OK;
	const uint64_t C = pow2_at_least(2 * n + 16);
	SYZ_TRY(ws_get(ctx, kWsPairSet, C * 8, &set));
	SYZ_HIP(hipMemsetAsync(set, 0xff, C * 8, s));
	SYZ_TRY(ws_grow_keep(ctx, kWsPairs, (*npairs_io + n) * 8 + 64, *npairs_io * 8, &out));
	*pairs_io = (uint64_t*)out;
	SYZ_TRY(seed_pair_counter(ctx, *npairs_io));
	k_pairs_set<<<grid_for(n, 256, 8192), 256, 0, s>>>((const uint64_t*)raw, n, (uint64_t*)set, C,
	                                                   &ctx->d_cnt[kCntAux]);
	k_pairs_compact<<<grid_for(C, 256, 8192), 256, 0, s>>>((const uint64_t*)set, C, (uint64_t*)out,
	                                                       &ctx->d_cnt[kCntAux2]);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	*npairs_io = ctx->h_cnt[kCntAux2];
	return SYZSIG_OK;
}

// ---------------------------------------------------------------- sharded batches
// A GPU's batch is aggregated locally and only each distinct element's
// staircase is routed to the element's owner: level l with first serial f[l]
// is on it iff f[l] < f[l'] for every higher level l'.  Any other record of e
// has an earlier local record of at least its level, so it is never new and
// never raises M_final -- and whatever dominates a staircase record in the
// whole batch, some staircase record (of any GPU) dominates it too.  So the
// owner's records-mode triage of the staircases gives checkNewSignal's exact
// result, at <= 4 records per distinct element instead of every record
// (SURVEY.md 8(e) "local filter").
constexpr uint32_t kMaxShardsAgg = 64;

// ---- the stream-ordered step's source side (syzsig_step_send_dev / _back_dev)
// Staircase records into fixed buckets: owner g's at send[g * (cap + 1) + 1 ...],
// cursor[g] = its true count (records past cap are counted, not written).
// Nothing is written when the run is void (gate: its spill flag or an LDS
// partition overflow).
__global__ __launch_bounds__(256) void k_stair_bucket(const uint32_t* __restrict__ dist_e,
                                                      const uint4* __restrict__ dist_f,
                                                      const uint32_t* __restrict__ cnt, uint32_t nregions,
                                                      uint32_t nlev, uint32_t nshards, uint64_t serial_base,
                                                      uint64_t cap, unsigned long long* cursor, uint64_t* send,
                                                      const unsigned long long* gate)
{
	__shared__ uint32_t h[kMaxShardsAgg];
	__shared__ unsigned long long base[kMaxShardsAgg];
	if (gate[kCntSpill] || gate[kCntAggOvf])
		return;
	for (uint32_t r = blockIdx.x; r < nregions; r += gridDim.x) {
		if (threadIdx.x < kMaxShardsAgg)
			h[threadIdx.x] = 0;
		__syncthreads();
		const uint32_t n = cnt[r] == kAggOverflow ? 0 : cnt[r];
		for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
			const uint64_t o = (uint64_t)r * kAggRegion + i;
			const uint32_t m = stair_levels(dist_f[o], nlev);
			if (m)
				atomicAdd(&h[owner_of(dist_e[o], nshards)], (uint32_t)__popc(m));
		}
		__syncthreads();
		if (threadIdx.x < nshards) {
			base[threadIdx.x] = h[threadIdx.x] ? atomicAdd(&cursor[threadIdx.x], (unsigned long long)h[threadIdx.x]) : 0;
			h[threadIdx.x] = 0;
		}
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
			const uint64_t o = (uint64_t)r * kAggRegion + i;
			const uint4 f4 = dist_f[o];
			const uint32_t m = stair_levels(f4, nlev);
			if (!m)
				continue;
			const uint32_t e = dist_e[o], g = owner_of(e, nshards);
			const uint32_t f[4] = {f4.x, f4.y, f4.z, f4.w};
			uint64_t pos = base[g] + atomicAdd(&h[g], (uint32_t)__popc(m));
			uint64_t* bk = send + (uint64_t)g * (cap + 1) + 1;
#pragma unroll
			for (uint32_t l = 0; l < 4; l++)
				if ((m >> l) & 1) {
					if (pos < cap)
						bk[pos] = ((uint64_t)e << 32) | ((uint64_t)l << 24) | ((serial_base + f[l]) & kSerialMask);
					pos++;
				}
		}
		__syncthreads();
	}
}

// bucket headers; the source's sent records and its largest bucket
__global__ void k_stair_heads(const unsigned long long* __restrict__ cursor, uint32_t nshards, uint64_t cap,
                              uint64_t* send, unsigned long long* sc)
{
	if (threadIdx.x != 0)
		return;
	const bool vd = sc[kCntSpill] != 0 || sc[kCntAggOvf] != 0;
	uint64_t tot = 0, mx = 0;
	for (uint32_t g = 0; g < nshards; g++) {
		const uint64_t c = vd ? 0 : cursor[g];
		tot += c;
		mx = max(mx, c);
	}
	// an overflow toward any owner is flagged to every owner, so that all of
	// them skip the step alike
	for (uint32_t g = 0; g < nshards; g++) {
		const uint64_t c = vd ? 0 : cursor[g];
		send[(uint64_t)g * (cap + 1)] = (c & SYZSIG_STEP_HDR_COUNT) | (vd ? SYZSIG_STEP_HDR_VOID : 0) |
		                                (mx > cap ? SYZSIG_STEP_HDR_OVF : 0);
	}
	sc[kCntCandidates] = tot;
	sc[kCntTouched] = mx;
}

// The owners' flags back at the source (blockIdx.y = owner g): the owner's
// status byte (1: the step is void, 2: the owner skipped) and, when 0, every
// flagged record of bucket g as the pair (call = serial - serial_base, e).
__global__ __launch_bounds__(256) void k_step_back(const uint64_t* __restrict__ send, const uint8_t* __restrict__ back,
                                                   uint64_t cap, uint64_t serial_base, uint8_t* call_new,
                                                   uint64_t* pairs, uint64_t pairs_cap, unsigned long long* bc)
{
	const uint32_t g = blockIdx.y, lane = lane_id();
	const uint64_t s0 = (uint64_t)g * (cap + 1);
	const uint8_t st = back[s0];
	if (st) {
		if (blockIdx.x == 0 && threadIdx.x == 0) {
			if (st == 1)
				atomicOr(&bc[kCntError], 1ull);
			else
				atomicOr(&bc[kCntAux], 1ull << g);
		}
		return;
	}
	// one device atomic per block and pass (a per-wave atomic on the one
	// counter serialised the kernel: 176 us at C4)
	__shared__ uint32_t wcnt[4];
	__shared__ unsigned long long s_base;
	const uint32_t w = threadIdx.x >> 6;
	const uint64_t n = min<uint64_t>(send[s0] & SYZSIG_STEP_HDR_COUNT, cap);
	for (uint64_t i0 = blockIdx.x * (uint64_t)blockDim.x; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t i = i0 + threadIdx.x;
		const bool on = i < n && back[s0 + 1 + i];
		uint64_t v = 0;
		if (on) {
			const uint64_t r = send[s0 + 1 + i];
			const uint64_t c = (r & kSerialMask) - serial_base;
			call_new[c] = 1;
			v = (c << 32) | (r >> 32);
		}
		const uint64_t m = __ballot(on);
		if (lane == 0)
			wcnt[w] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = 0, tot = 0;
		for (uint32_t k = 0; k < 4; k++) {
			before += k < w ? wcnt[k] : 0;
			tot += wcnt[k];
		}
		if (threadIdx.x == 0)
			s_base = tot ? atomicAdd(&bc[kCntAux2], (unsigned long long)tot) : 0;
		__syncthreads();
		const uint64_t o = s_base + before + lane_rank(m);
		if (on && pairs && o < pairs_cap)
			pairs[o] = v;
		__syncthreads();  // wcnt / s_base are rewritten by the next pass
	}
}

}  // namespace syz

using namespace syz;

extern "C" {

int syzsig_step_send_dev(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t serial_base, const int8_t* levels,
                         uint32_t nlevels, uint32_t nshards, uint64_t cap, uint64_t* d_send, int exact)
{
	SYZ_LOCK(ctx);
	if (!ctx || !b || !d_send || (b->nrec && !b->sigs) ||
	    (b->ncalls && (!b->call_start || !b->call_len || !b->call_prio || !b->call_new)))
		return fail(SYZSIG_EINVAL, "step_send: NULL argument");
	if (nshards == 0 || nshards > kMaxShardsAgg || cap == 0 || cap > SYZSIG_STEP_HDR_COUNT)
		return fail(SYZSIG_EINVAL, "step_send: need 1 <= nshards <= 64 and 1 <= cap < 2^40");
	if (b->nrec >= (1ull << 32))
		return fail(SYZSIG_ERANGE, "step_send: >= 2^32 records per GPU");
	if (serial_base + b->ncalls > kSerialMask + 1ull)
		return fail(SYZSIG_ERANGE, "step_send: batch serial order exceeds 2^24 calls");
	LevelMap lm;
	SYZ_TRY(level_map_from_levels(levels, nlevels, &lm));
	const hipStream_t s = ctx->stream;
	unsigned long long* sc = ctx->d_step + kStepSrc;
	void* wcur;
	SYZ_TRY(ws_get(ctx, kWsStepCursor, kMaxShardsAgg * 8 + 64, &wcur));
	unsigned long long* cursor = (unsigned long long*)wcur;
	ctx->step_src_timed = ctx->timing;
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev_step[0], s));
	// the flags-back counters start the step; the source counters are zeroed
	// below (or by k_cell_plan_fast)
	SYZ_HIP(hipMemsetAsync(ctx->d_step + kStepBack, 0, kNumCounters * 8, s));
	SYZ_HIP(hipMemsetAsync(cursor, 0, kMaxShardsAgg * 8, s));
	if (b->new_bits)
		SYZ_HIP(hipMemsetAsync(b->new_bits, 0, ((b->nrec + 31) / 32) * 4, s));
	const bool fast = !exact && ctx->cap_sd > 0 && !ctx->agg_counted_once && b->ncalls && b->nrec &&
	                  !(ctx->agg_dbg & (SYZSIG_DEBUG_EXACT_CELLS | SYZSIG_DEBUG_CAP_SPILL));
	if (fast) {
		// one capped-cell run with its assumptions checked on device (as the
		// one-sync triage run): prios among `levels`, valid ranges, <= nrec records
		AggGeom g = agg_geom_for(ctx, b->nrec, 0);
		g.ibits = g.cbits();
		const uint32_t P = 1u << g.pbits;
		ctx->step_src_parts = P;
		CapRun r;
		SYZ_TRY(cap_layout(ctx, b->nrec, nchunks_of(b->ncalls, g.ibits), P, ctx->cap_sd, &r));
		SYZ_TRY(cap_plan(ctx, b, 0, b->ncalls, lm, g, b->nrec, &r, kScat3Tile, sc));
		SYZ_TRY(cap_scatter_agg(ctx, b, 0, b->ncalls, lm, g, r, kScat3Tile, nullptr, sc, nullptr));
		k_stair_bucket<<<(int)std::min<uint32_t>(P, 2048), 256, 0, s>>>(
		    (const uint32_t*)r.de, (const uint4*)r.df, (const uint32_t*)r.dc, P, lm.n, nshards, serial_base, cap, cursor,
		    d_send, sc);
		SYZ_HIP(hipGetLastError());
	} else {
		// the exact path: validated, counted cells, the HBM fallback (host round trips)
		unsigned long long* hs = ctx->h_step + kStepSrc;
		memset(hs, 0, kNumCounters * 8);
		if (b->ncalls)
			SYZ_HIP(hipMemsetAsync(b->call_new, 0, b->ncalls, s));
		if (b->ncalls && b->nrec) {
			uint64_t total = 0;
			uint32_t mask[8];
			SYZ_TRY(batch_total_records(ctx, b, &total, mask));
			for (int p = 0; p < 256; p++)
				if (((mask[p >> 5] >> (p & 31)) & 1) && lm.lvl[p] == 0xff)
					return fail(SYZSIG_EINVAL, "step_send: a call's prio is not among `levels`");
			hs[kCntRecords] = total;
			if (total) {
				syzsig_batch_stats st;
				memset(&st, 0, sizeof(st));
				AggOut a;
				SYZ_TRY(agg_aggregate(ctx, b, 0, b->ncalls, lm, total, &st, &a));
				hs[kCntDistinct] = a.D;
				SYZ_HIP(hipMemcpyAsync(sc, hs, kNumCounters * 8, hipMemcpyHostToDevice, s));
				k_stair_bucket<<<(int)std::min<uint32_t>(a.nregions, 2048), 256, 0, s>>>(
				    a.dist_e, a.dist_f, a.cnt, a.nregions, lm.n, nshards, serial_base, cap, cursor, d_send, sc);
				SYZ_HIP(hipGetLastError());
			}
		}
		SYZ_HIP(hipMemcpyAsync(sc, hs, kNumCounters * 8, hipMemcpyHostToDevice, s));
		SYZ_HIP(hipStreamSynchronize(s));  // hs is consumed
	}
	k_stair_heads<<<1, 64, 0, s>>>(cursor, nshards, cap, d_send, sc);
	SYZ_HIP(hipGetLastError());
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev_step[1], s));
	return SYZSIG_OK;
}

int syzsig_step_back_dev(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t serial_base, const uint64_t* d_send,
                         uint32_t nshards, uint64_t cap, const uint8_t* d_back)
{
	SYZ_LOCK(ctx);
	if (!ctx || !b || !d_send || !d_back || (b->ncalls && !b->call_new) || (b->new_pairs_cap && !b->new_pairs))
		return fail(SYZSIG_EINVAL, "step_back: NULL argument");
	if (nshards == 0 || nshards > kMaxShardsAgg || cap == 0 || cap > SYZSIG_STEP_HDR_COUNT)
		return fail(SYZSIG_EINVAL, "step_back: need 1 <= nshards <= 64 and 1 <= cap < 2^40");
	const hipStream_t s = ctx->stream;
	unsigned long long* bc = ctx->d_step + kStepBack;
	ctx->step_back_timed = ctx->timing;
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev_step[4], s));
	const dim3 grid(grid_for(cap, 256, std::max(1, 2048 / (int)nshards)), nshards);
	if (!b->new_bits) {
		k_step_back<<<grid, 256, 0, s>>>(d_send, d_back, cap, serial_base, b->call_new, b->new_pairs,
		                                 b->new_pairs ? b->new_pairs_cap : 0, bc);
		SYZ_HIP(hipGetLastError());
	} else {
		// per-record bits need the pairs' count on the host: this call synchronises
		unsigned long long* hb = ctx->h_step + kStepBack;
		SYZ_HIP(hipMemcpyAsync(hb, bc, kNumCounters * 8, hipMemcpyDeviceToHost, s));
		SYZ_HIP(hipStreamSynchronize(s));
		const uint64_t np0 = hb[kCntAux2], bound = np0 + (uint64_t)nshards * cap;
		void* wp;
		SYZ_TRY(ws_grow_keep(ctx, kWsStepPairs, bound * 8 + 64, np0 * 8, &wp));
		k_step_back<<<grid, 256, 0, s>>>(d_send, d_back, cap, serial_base, b->call_new, (uint64_t*)wp, bound, bc);
		SYZ_HIP(hipGetLastError());
		SYZ_HIP(hipMemcpyAsync(hb, bc, kNumCounters * 8, hipMemcpyDeviceToHost, s));
		SYZ_HIP(hipStreamSynchronize(s));
		const uint64_t np1 = hb[kCntAux2];
		SYZ_TRY(agg_mark_bits(ctx, b, 0, b->ncalls, (const uint64_t*)wp, np0, np1));
		if (b->new_pairs && np1 > np0 && np0 < b->new_pairs_cap)
			SYZ_HIP(hipMemcpyAsync(b->new_pairs + np0, (const uint64_t*)wp + np0,
			                       (std::min(np1, b->new_pairs_cap) - np0) * 8, hipMemcpyDeviceToDevice, s));
	}
	if (ctx->timing)
		SYZ_HIP(hipEventRecord(ctx->ev_step[5], s));
	return SYZSIG_OK;
}

}  // extern "C"
