// hints.hip -- hint mutants on device: checkConstArg and checkDataArg over a
// batch of args (syzsig_hint_mutants_dev).
//
// References:
//   prog/hints.go:82-103    generateHints: the type filter is the caller's, the
//       switch on ConstArg / DataArg is arg_kind;
//   prog/hints.go:105-112   checkConstArg: one shrinkExpand of arg.Val;
//   prog/hints.go:114-132   checkDataArg: one shrinkExpand per byte offset i <
//       min(len, maxDataLength = 100 (:38)) of the 8 bytes from i on, zero-padded
//       past the arg's end (:122-124), each replacer copied back truncated to
//       the arg's end (:126-127);
//   prog/hints.go:164-218   shrinkExpand: shrinkexpand.h.
//
// An arg is at most 100 windows of 12 variants: 1200 lookups, almost all of
// them empty, so the per-query kernels of syzsig_shrink_expand_dev (12 ranges
// scanned and one sort workgroup per query) are the wrong shape.  Here one
// workgroup owns an arg:
//   k_hm_count   stages the arg's head (<= 107 bytes, byte loads) in LDS; its
//                lanes run the (window, variant) lookups -- cm_values: one
//                bounded search, a second where the key is present -- and count
//                the accepted candidates.  More than kHmList of them, or one
//                key with more than kHmList values, sends the arg to the
//                fallback.
//   k_su_scan    the candidates' offsets in the staging buffer
//   k_hm_list    the lookups again; the (window, replacer) candidates go to a
//                list of kHmList keys of two words in LDS at the block scan of
//                the lanes' counts, the list is sorted (su_bitonic) and its
//                distinct keys are staged (su_unique_write)
//   fallback     k_hm_queries writes the windows of the flagged args as
//                (call, value) queries; se_queries -- the body of
//                syzsig_shrink_expand_dev, long segments included -- leaves
//                each window's sorted distinct replacers
//   k_hm_arg_counts, k_su_scan, k_hm_emit   mutants per arg -> mut_off -> the
//                three output arrays, from either staging
// Count, scan, write; no atomic per key (the counters take one add per
// workgroup); every loop is bounded by the task count of an arg (<= 1200), a
// value range that was checked against kHmList, a window count, or the
// kSuSearchSteps of a search; the list's order before the sort is the task
// order, so nothing depends on scheduling.
#include <algorithm>
#include <vector>

#include "shrinkexpand.h"

namespace syz {

constexpr uint32_t kHmList = SYZSIG_HINT_LIST;
constexpr uint32_t kHmMaxData = SYZSIG_HINT_MAX_DATA;  // hints.go:38
constexpr uint32_t kHmHead = kHmMaxData + 7;           // window 99 reads bytes 99 .. 106
constexpr uint32_t kHmHeadLds = 112;
constexpr uint64_t kHmMaxArgs = 1ull << 25;            // 100 queries each stay below shrink_expand's 2^32
constexpr int kHmFast = kCntInserted, kHmFallback = kCntChanged, kHmWindows = kCntTouched, kHmCands = kCntCandidates;
static_assert((kHmList & (kHmList - 1)) == 0 && kHmList >= kSuThreads, "list: a power of two, at least one sweep");
static_assert(kHmList * 16 + 1024 <= 64 * 1024, "the list and the head stay below 64 KB of LDS");
static_assert(kHmHead + 1 <= kHmHeadLds, "head");

using HmTile = SuWordsTile<2, kHmList>;  // key = (window, replacer)

struct HmIn {
	const uint64_t* map_off;
	const uint64_t* pairs;
	uint64_t ncalls, npairs;
	const uint32_t* arg_call;
	const uint8_t* arg_kind;
	const uint64_t* arg_val;
	const uint64_t* arg_off;
	const uint8_t* data;
	uint64_t narg, nbytes;
	const uint64_t* special;
	uint32_t nspecial;
};

struct HmArg {
	uint64_t a, b;  // the call's pairs
	uint64_t val, off, len;
	uint32_t call, kind, nwin;
};

// arg i as the entry point takes it; false: SYZSIG_EINVAL (uniform per workgroup)
__device__ __forceinline__ bool hm_arg(const HmIn& A, uint64_t i, HmArg& g)
{
	g = HmArg{};
	g.call = A.arg_call[i];
	g.kind = A.arg_kind[i];
	g.val = A.arg_val[i];
	g.off = A.arg_off[i];
	const uint64_t end = A.arg_off[i + 1];
	if (g.call >= A.ncalls || g.kind > 1 || g.off > end || end > A.nbytes || (g.kind == 0 && g.off != end))
		return false;
	g.a = A.map_off[g.call];
	g.b = A.map_off[g.call + 1];
	if (g.a > g.b || g.b > A.npairs || g.b - g.a > kCmMaxSeg)
		return false;
	g.len = end - g.off;
	g.nwin = g.kind ? (uint32_t)(g.len < kHmMaxData ? g.len : kHmMaxData) : 1;  // hints.go:117-121
	return true;
}

// head[0 .. kHmHeadLds) = the arg's first bytes, zero from its end on
// (hints.go:122-123); barriers on both sides
__device__ __forceinline__ void hm_stage(const HmIn& A, const HmArg& g, uint8_t* head)
{
	__syncthreads();
	const uint32_t n = (uint32_t)(g.len < kHmHead ? g.len : kHmHead);
	for (uint32_t i = threadIdx.x; i < kHmHeadLds; i += kSuThreads)
		head[i] = i < n ? A.data[g.off + i] : 0;
	__syncthreads();
}

// window i's value: hints.go:124 (i < nwin <= 100: bytes i .. i + 7 < kHmHeadLds), or arg.Val (:106)
__device__ __forceinline__ uint64_t hm_window(const HmArg& g, const uint8_t* head, uint32_t i)
{
	if (!g.kind)
		return g.val;
	uint64_t v = 0;
#pragma unroll
	for (uint32_t j = 0; j < 8; j++)
		v |= (uint64_t)head[i + j] << (8 * j);
	return v;
}

// task t = window t / 12, variant t % 12: the values under its mutant
struct HmTask {
	uint64_t v, first;
	uint32_t win, n, width;
	bool be;
};

__device__ __forceinline__ HmTask hm_task(const HmIn& A, const HmArg& g, const uint8_t* head, uint32_t t)
{
	HmTask k;
	bool expand;
	k.win = t / kCmVariants;
	cm_variant(t % kCmVariants, k.width, expand, k.be);
	k.v = hm_window(g, head, k.win);
	k.n = cm_values(A.pairs, g.a, g.b, cm_mutant(k.v, k.width, expand, k.be), k.first);
	return k;
}

// the task's accepted candidates, in the order of the pairs (k.n <= kHmList)
template <typename F>
__device__ __forceinline__ uint32_t hm_accepted(const HmIn& A, const HmTask& k, F f)
{
	uint32_t c = 0;
	for (uint32_t j = 0; j < k.n; j++) {
		uint64_t rep;
		if (cm_replacer(k.v, A.pairs[2 * (k.first + j) + 1], k.width, k.be, A.special, A.nspecial, rep)) {
			f(c, rep);
			c++;
		}
	}
	return c;
}

// the sum of x over the lanes below this one and over the workgroup
// (uniform); every thread calls it
__device__ __forceinline__ uint32_t hm_block_scan(uint32_t x, uint32_t& total)
{
	__shared__ uint32_t s_w[kSuThreads / 64];
	const uint32_t w = threadIdx.x >> 6, incl = wave_incl_scan(x);
	__syncthreads();  // the last call's sums are read
	if (lane_id() == 63)
		s_w[w] = incl;
	__syncthreads();
	uint32_t wb = 0;
	total = 0;
#pragma unroll
	for (uint32_t k = 0; k < kSuThreads / 64; k++) {
		wb += k < w ? s_w[k] : 0;
		total += s_w[k];
	}
	return wb + incl - x;
}

// Per arg: validated; ncand = its accepted candidates if the list takes them
// (else 0), fbwin = its windows if it goes to the fallback (else 0).
__global__ __launch_bounds__(kSuThreads) void k_hm_count(HmIn A, uint32_t* ncand, uint32_t* fbwin,
                                                         unsigned long long* cnt)
{
	__shared__ uint8_t head[kHmHeadLds];
	uint64_t err = 0, nfast = 0, nfb = 0, nwin = 0, ncands = 0;  // (thread 0's count)
	for (uint64_t arg = blockIdx.x; arg < A.narg; arg += gridDim.x) {
		HmArg g;
		const bool ok = hm_arg(A, arg, g);
		uint32_t c = 0;
		bool big = false;
		if (ok) {
			hm_stage(A, g, head);
			for (uint32_t t = threadIdx.x; t < g.nwin * kCmVariants; t += kSuThreads) {
				const HmTask k = hm_task(A, g, head, t);
				if (k.n > kHmList)
					big = true;
				else
					c += hm_accepted(A, k, [](uint32_t, uint64_t) {});
			}
		}
		uint32_t total;
		hm_block_scan(c, total);
		const bool fb = __syncthreads_or(big) || total > kHmList;
		if (threadIdx.x == 0) {
			ncand[arg] = ok && !fb ? total : 0;
			fbwin[arg] = ok && fb ? g.nwin : 0;
			err += !ok;
			nfast += ok && !fb;
			nfb += ok && fb;
			nwin += g.nwin;
			ncands += ok && !fb ? total : 0;
		}
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kHmFast], nfast);
	block_count(&cnt[kHmFallback], nfb);
	block_count(&cnt[kHmWindows], nwin);
	block_count(&cnt[kHmCands], ncands);
}

// Per arg of the fast path: its candidates listed, sorted and made unique in
// LDS; the distinct (window, replacer) keys to stage[2 * coff[arg] ..], their
// count to ucnt[arg] (0 for every other arg).
__global__ __launch_bounds__(kSuThreads) void k_hm_list(HmIn A, const uint32_t* __restrict__ ncand,
                                                        const uint64_t* __restrict__ coff, uint64_t* stage,
                                                        uint32_t* ucnt)
{
	__shared__ uint8_t head[kHmHeadLds];
	__shared__ HmTile::Lds t;
	const SuOutKeys<SuU64<2>> pol{stage, coff, 1, ucnt};
	for (uint64_t arg = blockIdx.x; arg < A.narg; arg += gridDim.x) {
		if (ncand[arg] == 0) {  // (a valid arg: k_hm_count found it so)
			if (threadIdx.x == 0)
				ucnt[arg] = 0;
			continue;
		}
		HmArg g;
		hm_arg(A, arg, g);
		hm_stage(A, g, head);
		const uint32_t ntask = g.nwin * kCmVariants;
		uint32_t run = 0;
		for (uint32_t base = 0; base < ntask; base += kSuThreads) {
			HmTask k = {};
			uint32_t c = 0;
			if (base + threadIdx.x < ntask) {
				k = hm_task(A, g, head, base + threadIdx.x);
				if (k.n > kHmList)
					k.n = 0;  // (k_hm_count sent such an arg to the fallback)
				c = hm_accepted(A, k, [](uint32_t, uint64_t) {});
			}
			uint32_t total;
			const uint32_t pos = run + hm_block_scan(c, total);
			if (c)
				hm_accepted(A, k, [&](uint32_t j, uint64_t rep) {
					if (pos + j < kHmList)  // (at most ncand[arg] <= kHmList in all)
						t.set(pos + j, SuWords<2>{{k.win, rep}});
				});
			run += total;
		}
		const uint32_t n = run < kHmList ? run : kHmList;
		HmTile::sort(t, n, pow2_at_least(n, 1u));
		const uint64_t c = HmTile::unique_lds(n, arg, pol, t);
		if (threadIdx.x == 0)
			pol.finish(arg, c);
		__syncthreads();  // t is refilled for the next arg
	}
}

// the windows of the fallback's args as queries qbase[arg] .. + fbwin[arg]
__global__ __launch_bounds__(kSuThreads) void k_hm_queries(HmIn A, const uint32_t* __restrict__ fbwin,
                                                           const uint64_t* __restrict__ qbase, uint32_t* q_call,
                                                           uint64_t* q_val)
{
	__shared__ uint8_t head[kHmHeadLds];
	for (uint64_t arg = blockIdx.x; arg < A.narg; arg += gridDim.x) {
		if (fbwin[arg] == 0)
			continue;
		HmArg g;
		hm_arg(A, arg, g);
		hm_stage(A, g, head);
		for (uint32_t i = threadIdx.x; i < g.nwin; i += kSuThreads) {
			q_call[qbase[arg] + i] = g.call;
			q_val[qbase[arg] + i] = hm_window(g, head, i);
		}
	}
}

// acnt[arg] = its mutants: the list's distinct keys, or the fallback's over its windows
__global__ __launch_bounds__(256) void k_hm_arg_counts(const uint32_t* __restrict__ ucnt,
                                                       const uint32_t* __restrict__ fbwin,
                                                       const uint64_t* __restrict__ qbase,
                                                       const uint32_t* __restrict__ q_cnt, uint64_t narg,
                                                       uint64_t* acnt)
{
	const uint64_t arg = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (arg >= narg)
		return;
	uint64_t n = ucnt[arg];
	const uint32_t w = fbwin[arg];  // <= kHmMaxData
	for (uint32_t i = 0; i < w; i++)
		n += q_cnt[qbase[arg] + i];
	acnt[arg] = n;
}

// Arg a's mutants to entries off[a] .. off[a + 1] of the outputs (the total
// passed the capacity check): hints.go:126-127 gives at and nb.
__global__ __launch_bounds__(kSuThreads) void k_hm_emit(HmIn A, const uint64_t* __restrict__ off,
                                                        const uint64_t* __restrict__ stage,
                                                        const uint64_t* __restrict__ coff,
                                                        const uint32_t* __restrict__ fbwin,
                                                        const uint64_t* __restrict__ qbase, SeOut fb, uint64_t cap,
                                                        uint64_t* mut_off, uint32_t* mut_at, uint8_t* mut_nb,
                                                        uint64_t* mut_rep)
{
	for (uint64_t arg = blockIdx.x; arg < A.narg; arg += gridDim.x) {
		const uint64_t o = off[arg], n = off[arg + 1] - o;
		const bool data = A.arg_kind[arg] != 0;
		const uint64_t len = A.arg_off[arg + 1] - A.arg_off[arg];
		auto put = [&](uint64_t x, uint32_t win, uint64_t rep) {
			if (x >= cap)
				return;
			mut_at[x] = win;
			mut_nb[x] = (uint8_t)(data && len - win < 8 ? len - win : 8);
			mut_rep[x] = rep;
		};
		const uint32_t w = fbwin[arg];
		if (w == 0) {
			const uint64_t* s = stage + 2 * coff[arg];
			for (uint64_t x = threadIdx.x; x < n; x += kSuThreads)
				put(o + x, (uint32_t)s[2 * x], s[2 * x + 1]);
		} else {
			uint64_t run = o;
			for (uint32_t i = 0; i < w; i++) {  // <= kHmMaxData
				const uint64_t q = qbase[arg] + i;
				const uint32_t m = fb.cnt[q];
				const uint64_t* s = fb.stage + fb.voff[q * kCmVariants];
				for (uint32_t x = threadIdx.x; x < m; x += kSuThreads)
					put(run + x, i, s[x]);
				run += m;
			}
		}
		if (threadIdx.x == 0)
			mut_off[arg] = o;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
		mut_off[A.narg] = off[A.narg];
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_hint_mutants_dev(syzsig_ctx* ctx, const uint64_t* d_map_off, const uint64_t* d_pairs,
                                       uint64_t ncalls, uint64_t npairs, const uint32_t* d_arg_call,
                                       const uint8_t* d_arg_kind, const uint64_t* d_arg_val,
                                       const uint64_t* d_arg_off, const uint8_t* d_data, uint64_t narg,
                                       uint64_t nbytes, const uint64_t* special_ints, uint32_t nspecial,
                                       uint64_t* d_mut_off, uint32_t* d_mut_at, uint8_t* d_mut_nb,
                                       uint64_t* d_mut_rep, uint64_t cap, uint64_t* n_out)
{
	SYZ_LOCK(ctx);
	if (n_out)
		*n_out = 0;
	if (!ctx || !d_mut_off || !n_out || !d_map_off || (npairs && !d_pairs) ||
	    (narg && (!d_arg_call || !d_arg_kind || !d_arg_val || !d_arg_off)) || (nbytes && !d_data) ||
	    (nspecial && !special_ints) || (cap && (!d_mut_at || !d_mut_nb || !d_mut_rep)))
		return fail(SYZSIG_EINVAL, "hint_mutants: NULL argument");
	if (nspecial > kCmMaxSpecial)
		return fail(SYZSIG_ERANGE, "hint_mutants: at most 4096 special ints");
	if (narg > kHmMaxArgs)
		return fail(SYZSIG_EINVAL, "hint_mutants: arg count out of range");
	const hipStream_t s = ctx->stream;
	std::fill(ctx->hm_stats, ctx->hm_stats + 4, 0);
	if (narg == 0) {
		SYZ_HIP(hipMemsetAsync(d_mut_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	// ncand[narg], fbwin[narg], ucnt[narg], coff[narg + 1], qbase[narg + 1], acnt[narg], off[narg + 1],
	// special[nspecial]
	char* d;
	const size_t o_fb = align256(narg * 4), o_uc = o_fb + align256(narg * 4), o_coff = o_uc + align256(narg * 4),
	             o_qb = o_coff + align256((narg + 1) * 8), o_ac = o_qb + align256((narg + 1) * 8),
	             o_off = o_ac + align256(narg * 8), o_sp = o_off + align256((narg + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsHmMeta, o_sp + align256((size_t)nspecial * 8 + 8), (void**)&d));
	uint32_t *ncand = (uint32_t*)d, *fbwin = (uint32_t*)(d + o_fb), *ucnt = (uint32_t*)(d + o_uc);
	uint64_t *coff = (uint64_t*)(d + o_coff), *qbase = (uint64_t*)(d + o_qb), *acnt = (uint64_t*)(d + o_ac),
	         *off = (uint64_t*)(d + o_off), *special = (uint64_t*)(d + o_sp);
	std::vector<uint64_t> sp(special_ints, special_ints + nspecial);
	std::sort(sp.begin(), sp.end());
	SYZ_TRY(counters_reset(ctx));
	if (nspecial) {  // (pageable: the copy has left sp when the call returns)
		SYZ_HIP(hipMemcpyAsync(special, sp.data(), (size_t)nspecial * 8, hipMemcpyHostToDevice, s));
		SYZ_HIP(hipStreamSynchronize(s));
	}
	const HmIn A{d_map_off, d_pairs, ncalls, npairs, d_arg_call, d_arg_kind, d_arg_val, d_arg_off, d_data, narg, nbytes,
	             special, nspecial};
	const int grid = grid_cap(narg), tb = (int)((narg + 255) / 256);
	SYZ_TRY(su_time_begin(ctx));
	k_hm_count<<<grid, kSuThreads, 0, s>>>(A, ncand, fbwin, ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(ncand, narg, coff);
	k_su_scan<<<1, kSuThreads, 0, s>>>(fbwin, narg, qbase);
	SYZ_HIP(hipGetLastError());
	uint64_t nlist = 0, nq = 0;
	SYZ_HIP(hipMemcpyAsync(&nlist, coff + narg, 8, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipMemcpyAsync(&nq, qbase + narg, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "hint_mutants: an arg's call is outside the maps, a kind is not 0 or 1, arg_off "
		                           "decreases or passes nbytes, a const arg has bytes, or the map's offsets are not "
		                           "ascending inside its pairs");
	uint64_t stats[4] = {ctx->h_cnt[kHmFast], ctx->h_cnt[kHmFallback], ctx->h_cnt[kHmWindows], ctx->h_cnt[kHmCands]};
	void* stage;
	SYZ_TRY(ws_get(ctx, kWsHmStage, nlist * 16 + 256, &stage));
	k_hm_list<<<grid, kSuThreads, 0, s>>>(A, ncand, coff, (uint64_t*)stage, ucnt);
	SYZ_HIP(hipGetLastError());
	SeOut fb{};
	if (nq) {
		char* q;
		SYZ_TRY(ws_get(ctx, kWsHmQuery, align256(nq * 8) + nq * 4 + 256, (void**)&q));
		uint64_t* q_val = (uint64_t*)q;
		uint32_t* q_call = (uint32_t*)(q + align256(nq * 8));
		k_hm_queries<<<grid, kSuThreads, 0, s>>>(A, fbwin, qbase, q_call, q_val);
		SYZ_HIP(hipGetLastError());
		SYZ_TRY(se_queries(ctx, "hint_mutants", d_map_off, d_pairs, ncalls, npairs, q_call, q_val, nq, special_ints,
		                   nspecial, false, &fb));
		k_su_scan<<<1, kSuThreads, 0, s>>>(fb.seg_len, nq, fb.off);  // its candidates, for the stats
		SYZ_HIP(hipGetLastError());
		uint64_t fbc = 0;
		SYZ_HIP(hipMemcpyAsync(&fbc, fb.off + nq, 8, hipMemcpyDeviceToHost, s));
		SYZ_TRY(counters_fetch(ctx));
		if (ctx->h_cnt[kCntError])
			return fail(SYZSIG_EIO, "hint_mutants: internal: a long segment did not fit its workspace");
		stats[3] += fbc;
	}
	k_hm_arg_counts<<<tb, 256, 0, s>>>(ucnt, fbwin, qbase, fb.cnt, narg, acnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(acnt, narg, off);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, off + narg, 8, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipStreamSynchronize(s));
	std::copy(stats, stats + 4, ctx->hm_stats);
	*n_out = total;
	if (total > cap)
		return fail(SYZSIG_ERANGE, "hint_mutants: the result needs more than the given capacity");
	k_hm_emit<<<grid, kSuThreads, 0, s>>>(A, off, (const uint64_t*)stage, coff, fbwin, qbase, fb, cap, d_mut_off,
	                                      d_mut_at, d_mut_nb, d_mut_rep);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

extern "C" int syzsig_hint_mutants_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::hm_stats, out, "hint_mutants_stats");
}
