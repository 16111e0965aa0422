// pollres.hip -- the reply to a fuzzer's poll, applied on device: addMaxSignal
// and the inputs of other fuzzers, over a batch of Serials.
//
// References:
//   syz-fuzzer/fuzzer.go:344-350  the poll loop: maxSignal := r.MaxSignal.
//       Deserialize(); fuzzer.addMaxSignal(maxSignal); for every r.NewInputs
//       (at most 100 per poll, syz-manager/manager.go:1053-1057)
//       fuzzer.addInputFromAnotherFuzzer(inp);
//   syz-fuzzer/fuzzer.go:468-475  addMaxSignal: return when sign.Len() == 0,
//       else maxSignal.Merge(sign);
//   syz-fuzzer/fuzzer.go:433-444  addInputFromAnotherFuzzer: sign :=
//       inp.Signal.Deserialize(); addInputToCorpus(p, sign, sig);
//   syz-fuzzer/fuzzer.go:446-460  addInputToCorpus: corpusSignal.Merge(sign);
//       maxSignal.Merge(sign) for a non-empty sign;
//   pkg/signal/signal.go:58-71    Deserialize: s[e] = p entry after entry, so the
//       LAST entry of an element gives its prio, also when it is the lower one.
//
// A segment is one Serial.  D = Deserialize(segment) keeps, per element, the
// prio of its last entry; Merge (signal.go:117-131) is a max per element, which
// commutes and is idempotent.  So after the whole batch
//   maxSignal[e]    = max(M0[e], max over the segments s that carry e of last_s(e))
//   corpusSignal[e] = max(C0[e], the same over the INPUT segments)
// whatever order the segments run in; only the entry order inside one segment
// counts.  "Last" is an argmax over the entry index, so nothing is sorted:
//   k_pr_route   validates every segment, routes it (empty / short / long) and
//                counts the entries that reach each table; a long segment gets
//                its chunks and the buckets of its scratch table
//   k_su_scan x2 the chunks' and the scratch tables' offsets
//   k_pr_short   one workgroup per segment of at most kPrTile entries: every
//                entry claims its element's slot of an open-addressed LDS table
//                (kPrSlots = 2 kPrTile slots: at most half full) and raises the
//                slot's entry index with an LDS atomic max; after the barrier
//                entry i is its element's winner iff the slot holds i, and the
//                winners are merged into the HBM tables
//   k_pr_long_index / k_pr_long_commit   the same argmax for the longer segments
//                through a scratch table per segment in the context's workspace,
//                as k_deser_index resolves it for one Serial: element << 32 |
//                1 << 31 | index under atomicMax, then entry i is the winner iff
//                its element's slot holds i
// Every loop is bounded by a length, a count, kPrSlots or a table's bucket
// count.  An LDS table that cannot take an entry flags its segment, which then
// takes the long path in a second round; nothing waits for another wave.  The
// device atomics are the tables' inserts and maxes and the counters.
#include <algorithm>

#include "segsort.h"

namespace syz {

constexpr uint32_t kPrTile = SYZSIG_POLLRES_TILE;
constexpr uint32_t kPrThreads = 1024;  // k_pr_short: 16 waves; two workgroups fill a CU
constexpr uint32_t kPrPer = kPrTile / kPrThreads;
constexpr uint32_t kPrSlotBits = 13;
constexpr uint32_t kPrSlots = 1u << kPrSlotBits;
#ifndef SYZ_POLLRES_PROBES
#define SYZ_POLLRES_PROBES kPrSlots  // an experiment build lowers it to reach the flagged path
#endif
constexpr uint32_t kPrProbes = SYZ_POLLRES_PROBES;
constexpr uint32_t kPrChunk = 4096;           // entries of a long segment per workgroup turn
constexpr uint64_t kPrMaxSeg = 0x7fffffffu;   // a segment's entry index has 31 bits in its scratch slot
static_assert(kPrTile % kPrThreads == 0 && kPrSlots == 2 * kPrTile, "the LDS table is at most half full");
static_assert(kPrTile * 4 + kPrSlots * 4 <= 48 * 1024, "keys and slots of one segment: 48 KB of LDS");
static_assert(kPrProbes >= 1 && kPrProbes <= kPrSlots, "a probe sequence visits a slot at most once");

// the context's counters as this file uses them (zeroed per round)
constexpr int kPrInsC = kCntInserted, kPrInsM = kCntAux, kPrShort = kCntCandidates, kPrLong = kCntTouched,
              kPrTotM = kCntChanged, kPrTotC = kCntAux2, kPrLosers = kCntDefer, kPrLdsFail = kCntDeferNs,
              kPrTooLong = kCntDistinct;

// Routing.  flag == nullptr: a segment is long iff it has more than kPrTile
// entries.  flag != nullptr (the second round): iff k_pr_short flagged it.
__global__ __launch_bounds__(kSuThreads) void k_pr_route(const uint64_t* __restrict__ seg_off,
                                                         const uint8_t* __restrict__ seg_kind, uint64_t nseg,
                                                         uint64_t n_entries, const uint8_t* __restrict__ flag,
                                                         uint32_t* chunks, uint64_t* nbk, unsigned long long* cnt)
{
	uint64_t err = 0, big = 0, ns = 0, nl = 0, tm = 0, tc = 0;
	const uint64_t s = (uint64_t)blockIdx.x * kSuThreads + threadIdx.x;
	if (s < nseg) {
		const uint64_t a = seg_off[s], b = seg_off[s + 1];
		const uint8_t kind = seg_kind[s];
		uint32_t ch = 0;
		uint64_t nb = 0;
		if (a > b || b > n_entries || kind > SYZSIG_SEG_INPUT) {
			err++;
		} else if (b - a > kPrMaxSeg) {
			big++;
		} else if (b != a) {  // (an empty Serial deserializes to nil: fuzzer.go:469, :454)
			const uint64_t len = b - a;
			if (flag ? flag[s] != 0 : len > kPrTile) {
				nl++;
				ch = (uint32_t)((len + kPrChunk - 1) / kPrChunk);
				nb = pow2_at_least<uint64_t>(len + 1, 2);  // buckets_for(len): at most half full
			} else {
				ns++;
			}
			tm += len;                                  // fuzzer.go:474, :457
			tc += kind == SYZSIG_SEG_INPUT ? len : 0;   // fuzzer.go:456
		}
		chunks[s] = ch;
		nbk[s] = nb;
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kPrTooLong], big);
	block_count(&cnt[kPrShort], ns);
	block_count(&cnt[kPrLong], nl);
	block_count(&cnt[kPrTotM], tm);
	block_count(&cnt[kPrTotC], tc);
}

// home slot of an element in k_pr_short's LDS table (tests/pollres_keys.py restates it)
__device__ __forceinline__ uint32_t pr_lds_home(uint32_t e)
{
	return (e * 0x9E3779B1u) >> (32 - kPrSlotBits);
}

// Entry i (element e = keys[i]) claims its element's slot.  A slot holds 0
// (empty) or 1 + an entry index of its element; it only goes 0 -> index -> a
// larger index of the same element, so any value read names the slot's element.
// Returns the slot, or kPrSlots when kPrProbes slots held other elements.
__device__ __forceinline__ uint32_t pr_lds_claim(uint32_t* tab, const uint32_t* keys, uint32_t e, uint32_t i)
{
	uint32_t x = pr_lds_home(e);
	for (uint32_t n = 0; n < kPrProbes; n++) {
		uint32_t w = tab[x];
		if (w == 0) {
			w = atomicCAS(&tab[x], 0u, i + 1);
			if (w == 0)
				return x;
		}
		if (keys[w - 1] == e) {
			atomicMax(&tab[x], i + 1);
			return x;
		}
		x = (x + 1) & (kPrSlots - 1);
	}
	return kPrSlots;
}

__global__ __launch_bounds__(kPrThreads) void k_pr_short(const uint64_t* __restrict__ seg_off,
                                                         const uint8_t* __restrict__ seg_kind, uint64_t nseg,
                                                         const uint32_t* __restrict__ elems,
                                                         const int8_t* __restrict__ prios, uint64_t* corpus,
                                                         uint64_t c_bmask, uint64_t* max, uint64_t m_bmask,
                                                         uint8_t* flag, unsigned long long* cnt)
{
	__shared__ uint32_t s_key[kPrTile];
	__shared__ uint32_t s_tab[kPrSlots];
	__shared__ uint32_t s_fail;
	uint64_t ins_c = 0, ins_m = 0, ovf = 0, losers = 0, nfail = 0;
	for (uint64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
		const uint64_t a = seg_off[s];
		const uint64_t len64 = seg_off[s + 1] - a;
		if (len64 == 0 || len64 > kPrTile)
			continue;  // (the same for every thread of the workgroup)
		const uint32_t len = (uint32_t)len64;
		const bool input = seg_kind[s] == SYZSIG_SEG_INPUT;
		uint32_t e[kPrPer], slot[kPrPer];
		for (uint32_t x = threadIdx.x; x < kPrSlots; x += kPrThreads)
			s_tab[x] = 0;
		if (threadIdx.x == 0)
			s_fail = 0;
#pragma unroll
		for (uint32_t k = 0; k < kPrPer; k++) {
			const uint32_t i = threadIdx.x + k * kPrThreads;
			e[k] = i < len ? elems[a + i] : 0;
			if (i < len)
				s_key[i] = e[k];
		}
		__syncthreads();
#pragma unroll
		for (uint32_t k = 0; k < kPrPer; k++) {
			const uint32_t i = threadIdx.x + k * kPrThreads;
			slot[k] = i < len ? pr_lds_claim(s_tab, s_key, e[k], i) : 0;
			if (slot[k] == kPrSlots)
				s_fail = 1;
		}
		__syncthreads();
		if (s_fail) {  // nothing of this segment is committed here: the long path takes it
			if (threadIdx.x == 0) {
				flag[s] = 1;
				nfail++;
			}
		} else {
#pragma unroll
			for (uint32_t k = 0; k < kPrPer; k++) {
				const uint32_t i = threadIdx.x + k * kPrThreads;
				if (i >= len)
					continue;
				if (s_tab[slot[k]] != i + 1) {  // a later entry of the element: signal.go:68 overwrites
					losers++;
					continue;
				}
				tbl_merge2(corpus, c_bmask, max, m_bmask, e[k], prios[a + i], input, ins_c, ins_m, ovf);
			}
		}
		__syncthreads();  // the next segment clears the table
	}
	block_count(&cnt[kPrInsC], ins_c);
	block_count(&cnt[kPrInsM], ins_m);
	block_count(&cnt[kCntOverflow], ovf);
	block_count(&cnt[kPrLosers], losers);
	block_count(&cnt[kPrLdsFail], nfail);
}

// chunk c of the long path -> its segment: the last s with chunk_off[s] <= c
// (chunk_off[0] = 0 <= c < chunk_off[nseg]; a halving search over at most 2^64 segments)
__device__ __forceinline__ uint64_t pr_seg_of(const uint64_t* __restrict__ chunk_off, uint64_t nseg, uint64_t c)
{
	uint64_t lo = 0, hi = nseg;
	for (uint32_t it = 0; it < 64 && hi - lo > 1; it++) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (chunk_off[mid] <= c)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// signal.go:58-71 per long segment, pass 1: the slot of an element holds its largest entry index
__global__ __launch_bounds__(kSuThreads) void k_pr_long_index(const uint64_t* __restrict__ seg_off,
                                                              const uint32_t* __restrict__ elems, uint64_t nseg,
                                                              const uint64_t* __restrict__ chunk_off, uint64_t nchunks,
                                                              const uint64_t* __restrict__ tab_off,
                                                              const uint64_t* __restrict__ nbk, uint64_t* tab,
                                                              unsigned long long* cnt)
{
	uint64_t ovf = 0;
	for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
		const uint64_t s = pr_seg_of(chunk_off, nseg, c);
		const uint64_t a = seg_off[s], len = seg_off[s + 1] - a, i0 = (c - chunk_off[s]) * kPrChunk;
		const uint64_t i1 = i0 + kPrChunk < len ? i0 + kPrChunk : len;
		uint64_t* t = tab + (tab_off[s] << kBucketShift);
		const uint64_t bmask = nbk[s] - 1;
		for (uint64_t i = i0 + threadIdx.x; i < i1; i += kSuThreads) {
			const uint32_t e = elems[a + i];
			const uint64_t v = ((uint64_t)e << 32) | 0x80000000ull | i;
			uint64_t old;
			const int64_t idx = tbl_find_or_insert(t, bmask, e, v, old, max_probe_for(bmask));
			if (idx < 0)
				ovf++;
			else if (old != 0 && old < v)
				atomicMax(reinterpret_cast<unsigned long long*>(t + idx), (unsigned long long)v);
		}
	}
	block_count(&cnt[kCntOverflow], ovf);
}

// pass 2: entry i is its element's winner iff the slot holds i; the winners are merged
__global__ __launch_bounds__(kSuThreads) void k_pr_long_commit(
    const uint64_t* __restrict__ seg_off, const uint8_t* __restrict__ seg_kind, const uint32_t* __restrict__ elems,
    const int8_t* __restrict__ prios, uint64_t nseg, const uint64_t* __restrict__ chunk_off, uint64_t nchunks,
    const uint64_t* __restrict__ tab_off, const uint64_t* __restrict__ nbk, const uint64_t* __restrict__ tab,
    uint64_t* corpus, uint64_t c_bmask, uint64_t* max, uint64_t m_bmask, unsigned long long* cnt)
{
	uint64_t ins_c = 0, ins_m = 0, ovf = 0, losers = 0;
	for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
		const uint64_t s = pr_seg_of(chunk_off, nseg, c);
		const uint64_t a = seg_off[s], len = seg_off[s + 1] - a, i0 = (c - chunk_off[s]) * kPrChunk;
		const uint64_t i1 = i0 + kPrChunk < len ? i0 + kPrChunk : len;
		const uint64_t* t = tab + (tab_off[s] << kBucketShift);
		const uint64_t bmask = nbk[s] - 1;
		const bool input = seg_kind[s] == SYZSIG_SEG_INPUT;
		for (uint64_t i = i0 + threadIdx.x; i < i1; i += kSuThreads) {
			const uint32_t e = elems[a + i];
			uint64_t v = 0;
			if (tbl_lookup(t, bmask, e, v) < 0) {
				ovf++;  // (pass 1 placed every element or counted an overflow itself)
				continue;
			}
			if ((v & 0x7fffffffull) != i) {
				losers++;
				continue;
			}
			tbl_merge2(corpus, c_bmask, max, m_bmask, e, prios[a + i], input, ins_c, ins_m, ovf);
		}
	}
	block_count(&cnt[kPrInsC], ins_c);
	block_count(&cnt[kPrInsM], ins_m);
	block_count(&cnt[kCntOverflow], ovf);
	block_count(&cnt[kPrLosers], losers);
}

namespace {

struct PrMeta {
	uint32_t* chunks;
	uint64_t *nbk, *chunk_off, *tab_off;
	uint8_t* flag;
};

struct PrArgs {
	const uint64_t* seg_off;
	const uint8_t* seg_kind;
	uint64_t nseg;
	const uint32_t* elems;
	const int8_t* prios;
	uint64_t n_entries;
};

// routes the segments (by length, or by `flag`) and fetches the counters;
// *nchunks / *nbuckets = the long path's chunks and scratch buckets
int pr_route(syzsig_ctx* ctx, const PrArgs& A, const PrMeta& M, const uint8_t* flag, uint64_t* nchunks,
             uint64_t* nbuckets)
{
	const hipStream_t s = ctx->stream;
	SYZ_TRY(counters_reset(ctx));
	k_pr_route<<<(int)((A.nseg + kSuThreads - 1) / kSuThreads), kSuThreads, 0, s>>>(
	    A.seg_off, A.seg_kind, A.nseg, A.n_entries, flag, M.chunks, M.nbk, ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(M.chunks, A.nseg, M.chunk_off);
	k_su_scan<<<1, kSuThreads, 0, s>>>(M.nbk, A.nseg, M.tab_off);
	SYZ_HIP(hipGetLastError());
	SYZ_HIP(hipMemcpyAsync(nchunks, M.chunk_off + A.nseg, 8, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipMemcpyAsync(nbuckets, M.tab_off + A.nseg, 8, hipMemcpyDeviceToHost, s));
	return counters_fetch(ctx);
}

// enqueues the long path over the routed segments; tab = nbuckets zeroed buckets
int pr_long(syzsig_ctx* ctx, const PrArgs& A, const PrMeta& M, uint64_t nchunks, uint64_t nbuckets, uint64_t* tab,
            const Receiver& cs, const Receiver& ms)
{
	const hipStream_t s = ctx->stream;
	SYZ_HIP(hipMemsetAsync(tab, 0, nbuckets * kBucketSlots * sizeof(uint64_t), s));
	k_pr_long_index<<<grid_cap(nchunks), kSuThreads, 0, s>>>(A.seg_off, A.elems, A.nseg, M.chunk_off, nchunks,
	                                                         M.tab_off, M.nbk, tab, ctx->d_cnt);
	k_pr_long_commit<<<grid_cap(nchunks), kSuThreads, 0, s>>>(
	    A.seg_off, A.seg_kind, A.elems, A.prios, A.nseg, M.chunk_off, nchunks, M.tab_off, M.nbk, tab,
	    cs.slots(), cs.bmask(), ms.slots(), ms.bmask(), ctx->d_cnt);
	return SYZSIG_OK;
}

}  // namespace

}  // namespace syz

using namespace syz;

extern "C" int syzsig_fuzzer_poll_res_dev(syzsig_ctx* ctx, const uint64_t* d_seg_off, const uint8_t* d_seg_kind,
                                          uint64_t nseg, const uint32_t* d_elems, const int8_t* d_prios,
                                          uint64_t n_entries, syzsig_set** corpus_signal, syzsig_set** max_signal)
{
	SYZ_LOCK(ctx);
	if (!ctx || !corpus_signal || !max_signal || (nseg && (!d_seg_off || !d_seg_kind)) ||
	    (n_entries && (!d_elems || !d_prios)))
		return fail(SYZSIG_EINVAL, "fuzzer_poll_res: NULL argument");
	if (corpus_signal == max_signal || (*corpus_signal && *corpus_signal == *max_signal))
		return fail(SYZSIG_EINVAL, "fuzzer_poll_res: corpusSignal and maxSignal are one set");
	if (nseg >> 32)
		return fail(SYZSIG_ERANGE, "fuzzer_poll_res: 2^32 or more segments");
	SYZ_TRY(set_check_idle(*corpus_signal));
	SYZ_TRY(set_check_idle(*max_signal));
	std::fill(ctx->pr_stats, ctx->pr_stats + 4, 0);
	if (nseg == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	char* d;
	size_t o = 0;
	const auto take = [&o](size_t bytes) {
		const size_t at = o;
		o += align256(bytes);
		return at;
	};
	const size_t o_ch = take(nseg * 4), o_nbk = take(nseg * 8), o_coff = take((nseg + 1) * 8),
	             o_toff = take((nseg + 1) * 8), o_flag = take(nseg);
	SYZ_TRY(ws_get(ctx, kWsPrMeta, o, (void**)&d));
	const PrMeta M{(uint32_t*)(d + o_ch), (uint64_t*)(d + o_nbk), (uint64_t*)(d + o_coff), (uint64_t*)(d + o_toff),
	               (uint8_t*)(d + o_flag)};
	const PrArgs A{d_seg_off, d_seg_kind, nseg, d_elems, d_prios, n_entries};
	SYZ_TRY(su_time_begin(ctx));
	uint64_t nchunks = 0, nbuckets = 0;
	SYZ_TRY(pr_route(ctx, A, M, nullptr, &nchunks, &nbuckets));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "fuzzer_poll_res: a segment's range is reversed or ends past the entries, or its "
		                           "kind is unknown");
	if (ctx->h_cnt[kPrTooLong])
		return fail(SYZSIG_ERANGE, "fuzzer_poll_res: a segment of 2^31 or more entries");
	const uint64_t n_short = ctx->h_cnt[kPrShort], n_long = ctx->h_cnt[kPrLong], tot_m = ctx->h_cnt[kPrTotM],
	               tot_c = ctx->h_cnt[kPrTotC];
	if (tot_m == 0)
		return SYZSIG_OK;  // only empty Serials: nil receivers stay nil (fuzzer.go:469, :454)
	// the scratch tables and room in both tables first (a nil receiver: its table,
	// signal.go:121-125); nothing below the reservations can fail short of the device itself
	void* tab = nullptr;
	if (n_long)
		SYZ_TRY(ws_get(ctx, kWsPrTable, nbuckets * kBucketSlots * sizeof(uint64_t), &tab));
	Receiver cs, ms;
	if (tot_c)  // (not opened when no INPUT segment has an entry: no kernel then touches corpusSignal)
		SYZ_TRY(cs.open(ctx, corpus_signal, tot_c));
	SYZ_TRY(ms.open(ctx, max_signal, tot_m));
	SYZ_TRY(counters_reset(ctx));
	SYZ_HIP(hipMemsetAsync(M.flag, 0, nseg, s));
	if (n_short)
		k_pr_short<<<grid_cap(nseg, 1u << 16), kPrThreads, 0, s>>>(d_seg_off, d_seg_kind, nseg, d_elems, d_prios,
		                                                           cs.slots(), cs.bmask(), ms.slots(), ms.bmask(), M.flag,
		                                                           ctx->d_cnt);
	if (n_long)
		SYZ_TRY(pr_long(ctx, A, M, nchunks, nbuckets, (uint64_t*)tab, cs, ms));
	SYZ_TRY(commit_tail(ctx, "fuzzer_poll_res"));
	cs.commit(ctx->h_cnt[kPrInsC]);
	ms.commit(ctx->h_cnt[kPrInsM]);
	const uint64_t n_flagged = ctx->h_cnt[kPrLdsFail];
	uint64_t losers = ctx->h_cnt[kPrLosers], tab_bytes = n_long ? nbuckets * kBucketSlots * sizeof(uint64_t) : 0;
	if (n_flagged) {  // the segments whose LDS table had no room: the long path, in a second round
		SYZ_TRY(pr_route(ctx, A, M, M.flag, &nchunks, &nbuckets));
		SYZ_TRY(ws_get(ctx, kWsPrTable, nbuckets * kBucketSlots * sizeof(uint64_t), &tab));
		SYZ_TRY(counters_reset(ctx));
		SYZ_TRY(pr_long(ctx, A, M, nchunks, nbuckets, (uint64_t*)tab, cs, ms));
		SYZ_TRY(commit_tail(ctx, "fuzzer_poll_res"));
		cs.commit(ctx->h_cnt[kPrInsC]);  // (the sets are the caller's since the first round: the lengths only)
		ms.commit(ctx->h_cnt[kPrInsM]);
		losers += ctx->h_cnt[kPrLosers];
		tab_bytes = std::max<uint64_t>(tab_bytes, nbuckets * kBucketSlots * sizeof(uint64_t));
	}
	ctx->pr_stats[0] = n_short - n_flagged;
	ctx->pr_stats[1] = n_long + n_flagged;
	ctx->pr_stats[2] = losers;
	ctx->pr_stats[3] = tab_bytes;
	SYZ_TRY(su_time_end(ctx));
	return SYZSIG_OK;
}

extern "C" int syzsig_poll_res_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::pr_stats, out, "poll_res_stats");
}
