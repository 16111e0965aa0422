// items.hip -- the triage items of a batch, on device: what lies between
// checkNewSignal's verdict and triageInput's re-runs, and addInputToCorpus.
//
// References:
//   syz-fuzzer/proc.go:232-245    execute: one WorkTriage per call that
//       checkNewSignal returned, in call order, with the call's info.Signal;
//   syz-fuzzer/proc.go:107-111    triageInput's head: inputSignal =
//       FromRaw(item.info.Signal, signalPrio(...)), newSignal =
//       corpusSignalDiff(inputSignal), return when it is empty
//       (syzsig_triage_items_dev);
//   syz-fuzzer/fuzzer.go:446-460  addInputToCorpus: corpusSignal.Merge(sign);
//       maxSignal.Merge(sign) for a non-empty sign (syzsig_corpus_add_inputs_dev).
//
// FromRaw of a call is its distinct elements, each with the call's prio
// (signal.go:31-40: the prio is one value, so duplicates only collapse), and
// Diff (signal.go:73-88) keeps the elements e with corpus[e] absent or below
// that prio as int8.  Per item that is segsort.h's sort-unique over the call's
// own range of sigs (no gather copy: SuSegs points into the batch, R = 1) with
// an output policy that probes corpusSignal once per distinct element: the
// weight of a survivor is 1 << 32 | is_new, so one block scan places it in both
// the inputSignal and the newSignal stage, and put() reads the verdict from the
// weight instead of probing again.  Ascending order is one fixed instance of
// Serialize's map order.
//
// The tile is segsort.h's plain u32 tile (SuU32Tile, T = kItTile keys,
// SYZSIG_ITEMS_TILE; 4 T bytes of LDS): cover.hip's tuned tile writes its
// survivors itself, four per thread, and has no place for a weight.
//   k_it_count   validates every call's range, counts the flagged calls per
//                block of 256 calls
//   k_su_scan    over those block counts: the item list's offsets.  (k_su_scan
//                is one workgroup that walks its input 256 values at a time
//                with a running 64-bit sum, so it holds any count; the calls go
//                through it a block count at a time -- ncalls / 256 values --
//                and the items' three per-item scans directly, as the items of
//                triage_cover and the calls of comp_map do.)
//   k_it_prep    item i = the i-th flagged call: its call, prio, range of sigs
//                (the SuSegs arrays) and the long-segment counts
//   k_su_scan    the items' lengths -> their offsets in the two stages
//   su_sort_unique<ItTile, ItOut>, k_su_scan x 2 (the two counts -> the CSR
//   offsets), k_su_gather x 2, k_it_finish (calls, prios)
// Every loop is bounded by a length, a count or the table's bucket count known
// at launch; no kernel takes a device atomic per key.
#include <algorithm>

#include "segsort.h"

namespace syz {

#ifndef SYZ_ITEMS_TILE
#define SYZ_ITEMS_TILE SYZSIG_ITEMS_TILE
#endif
constexpr uint32_t kItTile = SYZ_ITEMS_TILE;
constexpr uint32_t kItThreads = kSuThreads;
constexpr uint32_t kItMaxSeg = 0x7fffffffu;  // records per flagged call
static_assert((kItTile & (kItTile - 1)) == 0 && kItTile >= kItThreads, "tile: a power of two, at least one sweep");
static_assert(kItTile * 4 <= 64 * 1024, "a workgroup's LDS stays at or below 64 KB");

using ItTile = SuU32Tile<kItTile>;

// output policy: a distinct element goes to the item's inputSignal stage and,
// when corpusSignal does not hold it at the item's prio or above, to its
// newSignal stage; both stages share the item's offset (a call's records bound both)
struct ItOut {
	uint32_t* stage_in;
	uint32_t* stage_new;
	const uint64_t* stage_off;
	uint32_t* cnt_in;
	uint32_t* cnt_new;
	const uint64_t* tbl;  // nullptr: a nil corpusSignal
	uint64_t bmask;
	const int8_t* item_prio;
	// inputSignal elements << 32 | newSignal elements; signal.go:79-83
	__device__ __forceinline__ uint64_t weight(uint64_t seg, uint32_t e) const
	{
		uint64_t v = 0;
		const bool known = tbl && tbl_lookup(tbl, bmask, e, v) >= 0 && slot_live(v) && slot_prio(v) >= item_prio[seg];
		return (1ull << 32) | (known ? 0u : 1u);
	}
	__device__ __forceinline__ void put(uint64_t seg, uint64_t pos, uint32_t e, uint64_t wt) const
	{
		const uint64_t o = stage_off[seg];
		stage_in[o + (pos >> 32)] = e;
		if (wt & 1)
			stage_new[o + (uint32_t)pos] = e;
	}
	__device__ __forceinline__ void finish(uint64_t seg, uint64_t total) const
	{
		cnt_in[seg] = (uint32_t)(total >> 32);
		cnt_new[seg] = (uint32_t)total;
	}
};

enum : uint32_t { kItNone = 0, kItItem, kItBadRange, kItTooLong };

// proc.go:232-245: a call is an item iff checkNewSignal returned it
__device__ __forceinline__ uint32_t it_class(uint64_t start, uint32_t len, uint8_t flag, uint64_t nrec)
{
	if (start > nrec || len > nrec - start)
		return kItBadRange;
	if (!flag)
		return kItNone;
	return len > kItMaxSeg ? kItTooLong : kItItem;
}

// this thread's rank among the workgroup's threads with f, and their number
__device__ __forceinline__ uint32_t it_rank(bool f, uint32_t& total)
{
	__shared__ uint32_t s_w[kItThreads / 64];
	const uint64_t m = __ballot(f);
	const uint32_t w = threadIdx.x >> 6;
	if (lane_id() == 0)
		s_w[w] = (uint32_t)__popcll(m);
	__syncthreads();
	uint32_t base = 0;
	total = 0;
#pragma unroll
	for (uint32_t x = 0; x < kItThreads / 64; x++) {
		base += x < w ? s_w[x] : 0;
		total += s_w[x];
	}
	__syncthreads();
	return base + lane_rank(m);
}

__global__ __launch_bounds__(kItThreads) void k_it_count(const uint64_t* __restrict__ call_start,
                                                         const uint32_t* __restrict__ call_len,
                                                         const uint8_t* __restrict__ call_new, uint64_t ncalls,
                                                         uint64_t nrec, uint32_t* blk_cnt, unsigned long long* cnt)
{
	const uint64_t c = (uint64_t)blockIdx.x * kItThreads + threadIdx.x;
	const uint32_t cls = c < ncalls ? it_class(call_start[c], call_len[c], call_new[c], nrec) : kItNone;
	uint32_t total;
	it_rank(cls == kItItem, total);
	if (threadIdx.x == 0)
		blk_cnt[blockIdx.x] = total;
	block_count(&cnt[kCntError], cls == kItBadRange);
	block_count(&cnt[kCntOverflow], cls == kItTooLong);
}

// item blk_off[block] + rank = the call; FromRaw casts the prio to int8 (signal.go:35)
__global__ __launch_bounds__(kItThreads) void k_it_prep(const uint64_t* __restrict__ call_start,
                                                        const uint32_t* __restrict__ call_len,
                                                        const uint8_t* __restrict__ call_prio,
                                                        const uint8_t* __restrict__ call_new, uint64_t ncalls,
                                                        uint64_t nrec, const uint64_t* __restrict__ blk_off,
                                                        uint32_t* item_call, int8_t* item_prio, uint64_t* seg_start,
                                                        uint32_t* seg_len, unsigned long long* cnt)
{
	uint64_t nl = 0, nt = 0, nk = 0, tot = 0;
	const uint64_t c = (uint64_t)blockIdx.x * kItThreads + threadIdx.x;
	const uint64_t start = c < ncalls ? call_start[c] : 0;
	const uint32_t len = c < ncalls ? call_len[c] : 0;
	const bool f = c < ncalls && it_class(start, len, call_new[c], nrec) == kItItem;
	uint32_t total;
	const uint64_t i = blk_off[blockIdx.x] + it_rank(f, total);
	if (f) {  // (i < the scan's total <= ncalls, the arrays' size)
		item_call[i] = (uint32_t)c;
		item_prio[i] = (int8_t)call_prio[c];
		seg_start[i] = start;
		seg_len[i] = len;
		tot = len;
		su_count_large<kItTile, ItTile::kAlign>(len, nl, nt, nk, cnt);
	}
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
	block_count(&cnt[kSuTotal], tot);
}

// the items' calls and prios, and every newSignal element's prio: its item's
__global__ __launch_bounds__(kItThreads) void k_it_finish(const uint32_t* __restrict__ ws_call,
                                                          const int8_t* __restrict__ ws_prio,
                                                          const uint64_t* __restrict__ new_off, uint64_t nitems,
                                                          uint32_t* item_call, int8_t* item_prio, int8_t* prios)
{
	for (uint64_t i = blockIdx.x; i < nitems; i += gridDim.x) {
		const uint64_t a = new_off[i], n = new_off[i + 1] - a;
		const int8_t p = ws_prio[i];
		if (threadIdx.x == 0) {
			item_call[i] = ws_call[i];
			item_prio[i] = p;
		}
		for (uint64_t x = threadIdx.x; x < n; x += kItThreads)
			prios[a + x] = p;
	}
}

// ---- syzsig_corpus_add_inputs_dev ----

// fuzzer.go:454 `!sign.Empty()` per kept item: the entries the commit will merge
__global__ __launch_bounds__(kItThreads) void k_it_kept(const uint64_t* __restrict__ input_off, uint64_t nitems,
                                                        uint64_t ninput, const uint8_t* __restrict__ item_keep,
                                                        unsigned long long* cnt)
{
	uint64_t err = 0, tot = 0;
	const uint64_t i = (uint64_t)blockIdx.x * kItThreads + threadIdx.x;
	if (i < nitems) {
		const uint64_t a = input_off[i], b = input_off[i + 1];
		if (a > b || b > ninput)
			err++;
		else if (!item_keep || item_keep[i])
			tot = b - a;
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kSuTotal], tot);
}

// fuzzer.go:456-457 for every kept item (tbl_merge2).  Max-merge commutes, so
// the order the workgroups run in does not show.
__global__ __launch_bounds__(kItThreads) void k_it_commit(const uint64_t* __restrict__ input_off,
                                                          const uint32_t* __restrict__ elems,
                                                          const int8_t* __restrict__ item_prio, uint64_t nitems,
                                                          const uint8_t* __restrict__ item_keep, uint64_t* corpus,
                                                          uint64_t c_bmask, uint64_t* max, uint64_t m_bmask,
                                                          unsigned long long* cnt)
{
	uint64_t ins_c = 0, ins_m = 0, ovf = 0;
	for (uint64_t i = blockIdx.x; i < nitems; i += gridDim.x) {
		if (item_keep && !item_keep[i])
			continue;
		const uint64_t a = input_off[i], b = input_off[i + 1];
		const int8_t p = item_prio[i];
		for (uint64_t j = a + threadIdx.x; j < b; j += kItThreads)
			tbl_merge2(corpus, c_bmask, max, m_bmask, elems[j], p, true, ins_c, ins_m, ovf);
	}
	block_count(&cnt[kCntInserted], ins_c);
	block_count(&cnt[kCntAux], ins_m);
	block_count(&cnt[kCntOverflow], ovf);
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_triage_items_dev(syzsig_ctx* ctx, const uint32_t* d_sigs, uint64_t nrec,
                                       const uint64_t* d_call_start, const uint32_t* d_call_len,
                                       const uint8_t* d_call_prio, uint64_t ncalls, const uint8_t* d_call_new,
                                       const syzsig_set* corpus_signal, uint32_t* d_item_call, int8_t* d_item_prio,
                                       uint64_t item_cap, uint64_t* d_input_off, uint32_t* d_input_elems,
                                       uint64_t input_cap, uint64_t* d_item_off, uint32_t* d_elems, int8_t* d_prios,
                                       uint64_t new_cap, uint64_t* n_items, uint64_t* n_input, uint64_t* n_new)
{
	SYZ_LOCK(ctx);
	if (n_items)
		*n_items = 0;
	if (n_input)
		*n_input = 0;
	if (n_new)
		*n_new = 0;
	if (!ctx || !n_items || !n_input || !n_new || !d_input_off || !d_item_off ||
	    (ncalls && (!d_call_start || !d_call_len || !d_call_prio || !d_call_new)) || (nrec && !d_sigs) ||
	    (item_cap && (!d_item_call || !d_item_prio)) || (input_cap && !d_input_elems) ||
	    (new_cap && (!d_elems || !d_prios)))
		return fail(SYZSIG_EINVAL, "triage_items: NULL argument");
	if (ncalls >> 32)
		return fail(SYZSIG_ERANGE, "triage_items: 2^32 or more calls");
	SYZ_TRY(set_check_idle(corpus_signal));
	const hipStream_t s = ctx->stream;
	std::fill(ctx->it_stats, ctx->it_stats + 4, 0);
	if (ncalls == 0) {
		SYZ_HIP(hipMemsetAsync(d_input_off, 0, 8, s));
		SYZ_HIP(hipMemsetAsync(d_item_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	// the item arrays are sized by the calls: the item count reaches the host
	// with the prep kernel's counts, in one round trip
	const uint64_t nb = (ncalls + kItThreads - 1) / kItThreads;
	char* d;
	size_t o = 0;
	const auto take = [&o](size_t bytes) {
		const size_t at = o;
		o += align256(bytes);
		return at;
	};
	const size_t o_bcnt = take(nb * 4), o_boff = take((nb + 1) * 8), o_call = take(ncalls * 4), o_prio = take(ncalls),
	             o_start = take(ncalls * 8), o_len = take(ncalls * 4), o_soff = take((ncalls + 1) * 8),
	             o_cin = take(ncalls * 4), o_cnew = take(ncalls * 4), o_ioff = take((ncalls + 1) * 8),
	             o_noff = take((ncalls + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsSuMeta, o, (void**)&d));
	uint32_t *blk_cnt = (uint32_t*)(d + o_bcnt), *ws_call = (uint32_t*)(d + o_call), *seg_len = (uint32_t*)(d + o_len),
	         *cnt_in = (uint32_t*)(d + o_cin), *cnt_new = (uint32_t*)(d + o_cnew);
	uint64_t *blk_off = (uint64_t*)(d + o_boff), *seg_start = (uint64_t*)(d + o_start), *stage_off = (uint64_t*)(d + o_soff),
	         *in_off = (uint64_t*)(d + o_ioff), *new_off = (uint64_t*)(d + o_noff);
	int8_t* ws_prio = (int8_t*)(d + o_prio);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_it_count<<<(int)nb, kItThreads, 0, s>>>(d_call_start, d_call_len, d_call_new, ncalls, nrec, blk_cnt, ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(blk_cnt, nb, blk_off);
	k_it_prep<<<(int)nb, kItThreads, 0, s>>>(d_call_start, d_call_len, d_call_prio, d_call_new, ncalls, nrec, blk_off,
	                                         ws_call, ws_prio, seg_start, seg_len, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	uint64_t ni = 0, tot[2] = {0, 0};
	SYZ_HIP(hipMemcpyAsync(&ni, blk_off + nb, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "triage_items: a call's range lies outside the records");
	if (ctx->h_cnt[kCntOverflow])
		return fail(SYZSIG_ERANGE, "triage_items: a flagged call holds 2^31 or more records");
	void *stage_in = nullptr, *stage_new = nullptr;
	if (ni) {
		const uint64_t total = ctx->h_cnt[kSuTotal], maxlen = ctx->h_cnt[kSuMaxLen];
		SYZ_TRY(ws_get(ctx, kWsSuStage, total * 4 + 256, &stage_in));
		SYZ_TRY(ws_get(ctx, kWsSuStage2, total * 4 + 256, &stage_new));
		k_su_scan<<<1, kSuThreads, 0, s>>>(seg_len, ni, stage_off);
		const SuSegs S{d_sigs, 1, seg_start, seg_len, 1, seg_len, ni};
		const ItOut pol{(uint32_t*)stage_in,
		                (uint32_t*)stage_new,
		                stage_off,
		                cnt_in,
		                cnt_new,
		                corpus_signal ? corpus_signal->slots : nullptr,
		                corpus_signal ? corpus_signal->nbuckets - 1 : 0,
		                ws_prio};
		ctx->it_stats[1] = ctx->h_cnt[kSuLarge];
		for (uint64_t w = kItTile; w < maxlen; w <<= 1)
			ctx->it_stats[2]++;  // su_sort_unique's merge loop
		SYZ_TRY((su_sort_unique<ItTile, ItOut>(ctx, S, pol)));
		k_su_scan<<<1, kSuThreads, 0, s>>>(cnt_in, ni, in_off);
		k_su_scan<<<1, kSuThreads, 0, s>>>(cnt_new, ni, new_off);
		SYZ_HIP(hipGetLastError());
		SYZ_HIP(hipMemcpyAsync(&tot[0], in_off + ni, 8, hipMemcpyDeviceToHost, s));
		SYZ_HIP(hipMemcpyAsync(&tot[1], new_off + ni, 8, hipMemcpyDeviceToHost, s));
		SYZ_TRY(counters_fetch(ctx));
		if (ctx->h_cnt[kCntError])
			return fail(SYZSIG_EIO, "triage_items: internal: a long segment did not fit its workspace");
	}
	ctx->it_stats[0] = ni;
	ctx->it_stats[3] = corpus_signal ? tot[0] : 0;  // one probe per distinct element
	*n_items = ni;
	*n_input = tot[0];
	*n_new = tot[1];
	if (ni > item_cap || tot[0] > input_cap || tot[1] > new_cap)
		return fail(SYZSIG_ERANGE, "triage_items: the items need more than the given capacities");
	if (ni) {
		k_su_gather<<<grid_cap(ni), kSuThreads, 0, s>>>((const uint32_t*)stage_in, stage_off, 1, 1, in_off, ni, d_input_elems,
		                                                d_input_off);
		k_su_gather<<<grid_cap(ni), kSuThreads, 0, s>>>((const uint32_t*)stage_new, stage_off, 1, 1, new_off, ni, d_elems,
		                                                d_item_off);
		k_it_finish<<<grid_cap(ni), kItThreads, 0, s>>>(ws_call, ws_prio, new_off, ni, d_item_call, d_item_prio, d_prios);
		SYZ_HIP(hipGetLastError());
	} else {
		SYZ_HIP(hipMemsetAsync(d_input_off, 0, 8, s));
		SYZ_HIP(hipMemsetAsync(d_item_off, 0, 8, s));
	}
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

extern "C" int syzsig_triage_items_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::it_stats, out, "triage_items_stats");
}

extern "C" int syzsig_corpus_add_inputs_dev(syzsig_ctx* ctx, const uint64_t* d_input_off, const uint32_t* d_input_elems,
                                            uint64_t n_input, const int8_t* d_item_prio, uint64_t n_items,
                                            const uint8_t* d_item_keep, syzsig_set** corpus_signal,
                                            syzsig_set** max_signal)
{
	SYZ_LOCK(ctx);
	if (!ctx || !corpus_signal || !max_signal || (n_items && (!d_input_off || !d_item_prio)) ||
	    (n_input && !d_input_elems))
		return fail(SYZSIG_EINVAL, "corpus_add_inputs: NULL argument");
	if (corpus_signal == max_signal || (*corpus_signal && *corpus_signal == *max_signal))
		return fail(SYZSIG_EINVAL, "corpus_add_inputs: corpusSignal and maxSignal are one set");
	SYZ_TRY(set_check_idle(*corpus_signal));
	SYZ_TRY(set_check_idle(*max_signal));
	if (n_items == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	SYZ_TRY(counters_reset(ctx));
	k_it_kept<<<(int)((n_items + kItThreads - 1) / kItThreads), kItThreads, 0, s>>>(d_input_off, n_items, n_input,
	                                                                               d_item_keep, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "corpus_add_inputs: an item's range is reversed or lies outside the elements");
	const uint64_t total = ctx->h_cnt[kSuTotal];
	if (total == 0)
		return SYZSIG_OK;  // nothing kept, or only empty signs: nil receivers stay nil (fuzzer.go:454)
	// room in both tables first (a nil receiver: its table, signal.go:121-125);
	// nothing below the reservations can fail short of the device itself
	Receiver cs, ms;
	SYZ_TRY(cs.open(ctx, corpus_signal, total));
	SYZ_TRY(ms.open(ctx, max_signal, total));
	SYZ_TRY(counters_reset(ctx));
	k_it_commit<<<grid_cap(n_items, 1u << 16), kItThreads, 0, s>>>(d_input_off, d_input_elems, d_item_prio, n_items,
	                                                               d_item_keep, cs.slots(), cs.bmask(), ms.slots(),
	                                                               ms.bmask(), ctx->d_cnt);
	SYZ_TRY(commit_tail(ctx, "corpus_add_inputs"));
	cs.commit(ctx->h_cnt[kCntInserted]);
	ms.commit(ctx->h_cnt[kCntAux]);
	return SYZSIG_OK;
}
