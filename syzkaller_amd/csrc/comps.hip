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
//   prog/hints.go:164-218         shrinkExpand (syzsig_shrink_expand_dev; its
//       per-candidate rule is shrinkexpand.h's, and se_queries, its body over
//       device-resident queries, is also the fallback of hints.hip).
// All three reduce to one operation per segment -- sort ascending, drop equal
// neighbours, write the survivors -- over keys of 3, 2 and 1 u64 words: the
// comparison triple; the (key, value) pair of the map; a replacer.
//
// The segmented sort-unique is segsort.h's, over its plain tile of W-word keys
// (T = kCmTile keys, SYZSIG_COMPS_TILE; 8 W T bytes of LDS, 48 KB at W = 3; a
// call has up to 65535 records, 131070 pairs, so segments do pass T).  What a
// survivor turns into is the output policy's business: SuOutKeys writes the
// key itself; CmOutComps applies ignore() and write(), so a survivor weighs 0,
// 3 or 5 output words, and the block scan runs over (count << 32 | words).
#include <algorithm>
#include <vector>

#include "shrinkexpand.h"

namespace syz {

#ifndef SYZ_COMPS_TILE
#define SYZ_COMPS_TILE SYZSIG_COMPS_TILE
#endif
constexpr uint32_t kCmTile = SYZ_COMPS_TILE;
constexpr uint32_t kCmThreads = kSuThreads;
constexpr uint32_t kCmMaxComps = 65535;       // executor.h:581-582: 8 + 32 n bytes fit kCoverSize * 8
constexpr uint64_t kCmMaxOutput = 16ull << 20;  // executor.h kMaxOutput
constexpr uint32_t kCmpConst = 1, kCmpSizeMask = 6, kCmpSize1 = 0, kCmpSize2 = 2, kCmpSize8 = 6;  // executor.h:147-152
static_assert((kCmTile & (kCmTile - 1)) == 0 && kCmTile >= kCmThreads, "tile: a power of two, at least one sweep");
static_assert(kCmTile * 3 * 8 <= 64 * 1024, "the widest key's tile stays at or below 64 KB of LDS");

template <int W>
using CmTile = SuWordsTile<W, kCmTile>;

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
	__device__ __forceinline__ uint64_t weight(uint64_t, const SuWords<3>& k) const
	{
		if (ignore(k.w[0], k.w[1], k.w[2]))
			return 0;
		return (1ull << 32) | ((k.w[0] & kCmpSizeMask) == kCmpSize8 ? 5u : 3u);
	}
	// executor.h:823-859.  The low 32 bits of a sign extension from 1, 2 or 4
	// bytes are what leaves for those sizes.
	__device__ __forceinline__ void put(uint64_t seg, uint64_t pos, const SuWords<3>& k, uint64_t) const
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
			su_count_large<kCmTile, 1>(len, nl, nt, nk, cnt);
		}
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
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
		su_count_large<kCmTile, 1>((uint32_t)total, nl, nt, nk, cnt);
	}
	block_count(&cnt[kCntOverflow], ovf);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
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

// (the per-candidate rule -- cm_variant, cm_mutant, cm_values, cm_replacer -- is shrinkexpand.h's)

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
			uint64_t first;
			vcnt[g] = cm_values(pairs, a, b, cm_mutant(q_val[q], width, expand, be), first);
			vlo[g] = first;
		}
	}
	block_count(&cnt[kCntError], err);
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
		uint32_t run = 0;
		for (uint32_t base = 0; base < n; base += 64) {
			const uint32_t i = base + lane;
			uint64_t rep = 0;
			const bool acc = i < n && cm_replacer(v, pairs[2 * (lo + i) + 1], width, be, special, nspecial, rep);
			const uint64_t m = __ballot(acc);
			if (acc)
				o[run + lane_rank(m)] = rep;
			run += (uint32_t)__popcll(m);
		}
		if (lane == 0)
			src_len[g] = run;
	}
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
	k_su_scan<<<1, kCmThreads, 0, s>>>(cnt, nseg, off);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, off + nseg, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, std::string(what) + ": internal: a long segment did not fit its workspace");
	*n_out = total;
	if (total > cap)
		return fail(SYZSIG_ERANGE, std::string(what) + ": the result needs more than the given capacity");
	k_su_gather<<<grid_cap(nseg), kCmThreads, 0, s>>>(stage, stage_pos, pos_stride, W, off, nseg, d_out, d_off);
	SYZ_HIP(hipGetLastError());
	if (d_status)
		SYZ_HIP(hipMemcpyAsync(d_status, status, nseg * 4, hipMemcpyDeviceToDevice, s));
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

// shrinkexpand.h: the body of syzsig_shrink_expand_dev over device-resident queries
int se_queries(syzsig_ctx* ctx, const char* what, const uint64_t* d_map_off, const uint64_t* d_pairs, uint64_t ncalls,
               uint64_t npairs, const uint32_t* d_q_call, const uint64_t* d_q_val, uint64_t nq,
               const uint64_t* special_ints, uint32_t nspecial, bool timed, SeOut* out)
{
	const hipStream_t s = ctx->stream;
	const std::string who = what;
	const uint64_t nv = nq * kCmVariants;
	// vlo[nv], voff[nv + 1], vcnt[nv], src_len[nv], seg_len[nq], cnt[nq], off[nq + 1], special[nspecial]
	char* d;
	const size_t o_voff = align256(nv * 8), o_vcnt = o_voff + align256((nv + 1) * 8), o_sl = o_vcnt + align256(nv * 4),
	             o_seg = o_sl + align256(nv * 4), o_cnt = o_seg + align256(nq * 4), o_off = o_cnt + align256(nq * 4),
	             o_sp = o_off + align256((nq + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsSuMeta, o_sp + align256((size_t)nspecial * 8 + 8), (void**)&d));
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
	if (timed)
		SYZ_TRY(su_time_begin(ctx));
	k_se_count<<<(int)((nv + 255) / 256), 256, 0, s>>>(d_map_off, d_pairs, ncalls, npairs, d_q_call, d_q_val, nq, vlo,
	                                                   vcnt, ctx->d_cnt);
	k_su_scan<<<1, kCmThreads, 0, s>>>(vcnt, nv, voff);
	SYZ_HIP(hipGetLastError());
	uint64_t ncand = 0;
	SYZ_HIP(hipMemcpyAsync(&ncand, voff + nv, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, who + ": a query's call is outside the map, or the map's offsets are not "
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
		return fail(SYZSIG_ERANGE, who + ": a query has 2^31 or more candidates");
	const SuSegs S{cand, 1, voff, src_len, kCmVariants, seg_len, nq};
	// a query's survivors go to the head of its own candidate range in stage2
	const SuOutKeys<SuU64<1>> pol{(uint64_t*)stage2, voff, kCmVariants, cnt};
	SYZ_TRY((su_sort_unique<CmTile<1>, SuOutKeys<SuU64<1>>>(ctx, S, pol)));
	*out = SeOut{(const uint64_t*)stage2, voff, cnt, seg_len, off};
	return SYZSIG_OK;
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
	SYZ_TRY(su_time_begin(ctx));
	k_cm_prep_calls<<<(int)((ncalls + 255) / 256), 256, 0, s>>>(d_call_start, d_call_len, ncalls, ncmp,
	                                                            (uint32_t*)seg_len, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "exec_comps: a call's records lie outside the buffer, or a call has more than "
		                           "65535 comparisons");
	const SuSegs S{d_comps, 4, d_call_start, (const uint32_t*)seg_len, 1, (const uint32_t*)seg_len, ncalls};
	const CmOutComps pol{d_out, d_call_start, d_out_words, d_comps_cnt, out_start};
	SYZ_TRY((su_sort_unique<CmTile<3>, CmOutComps>(ctx, S, pol)));
	SYZ_TRY(su_time_end(ctx));
	SYZ_TRY(counters_fetch(ctx));
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
	const size_t o_ps = align256((ncalls + 1) * 8), o_pl = o_ps + align256(ncalls * 8), o_sl = o_pl + align256(ncalls * 4),
	             o_cnt = o_sl + align256(ncalls * 4), o_off = o_cnt + align256(ncalls * 4), o_st = o_off + align256((ncalls + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsSuMeta, o_st + align256(ncalls * 4), (void**)&d));
	uint64_t *rec_base = (uint64_t*)d, *pair_start = (uint64_t*)(d + o_ps), *off = (uint64_t*)(d + o_off);
	uint32_t *pair_len = (uint32_t*)(d + o_pl), *seg_len = (uint32_t*)(d + o_sl), *cnt = (uint32_t*)(d + o_cnt);
	int32_t* status = (int32_t*)(d + o_st);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	const int cb = (int)((ncalls + 255) / 256);
	k_cm_check_regions<<<cb, 256, 0, s>>>(d_comps_start, d_comps_cnt, d_comps_end, ncalls, nwords, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "comp_map: a call's comparisons start outside its region, a region ends outside "
		                           "the buffer, or a call has more than 65535 comparisons");
	k_su_scan<<<1, kCmThreads, 0, s>>>(d_comps_cnt, ncalls, rec_base);
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
	const SuSegs S{stage, 2, pair_start, pair_len, 1, seg_len, ncalls};
	const SuOutKeys<SuU64<2>> pol{(uint64_t*)stage2, pair_start, 1, cnt};
	SYZ_TRY((su_sort_unique<CmTile<2>, SuOutKeys<SuU64<2>>>(ctx, S, pol)));
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
	SeOut o;
	SYZ_TRY(se_queries(ctx, "shrink_expand", d_map_off, d_pairs, ncalls, npairs, d_q_call, d_q_val, nq, special_ints,
	                   nspecial, true, &o));
	return cm_emit_csr<1>(ctx, "shrink_expand", o.stage, o.voff, kCmVariants, o.cnt, o.off, nq, d_rep_off, d_rep, cap,
	                      n_out);
}
