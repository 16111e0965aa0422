// prio.hip -- call-to-call priorities over the whole corpus and the ChoiceTable
// on device: the numeric part of prog/prio.go.
//
// References:
//   prog/prio.go:27-36     CalculatePriorities: dynamic[i][j] *= static[i][j]
//   prog/prio.go:118-129   calcStaticPriorities' tail: pp[c0] = the row's max,
//                          then normalizePrio
//   prog/prio.go:133-149   calcDynamicPrio: prios[id0][id1] += 1.0 for every
//                          ordered pair of call positions of every program
//   prog/prio.go:153-187   normalizePrio, row by row
//   prog/prio.go:198-228   BuildChoiceTable: run[i][j] = running sum of
//                          int(prios[i][j] * 1000) over the enabled j
//   prog/prio.go:230-245   Choose: sort.SearchInts(run[call], x)
//   syz-manager/manager.go:896, syz-fuzzer/fuzzer.go:173   the callers
//
// A cell of the dynamic matrix is the number of (position of a, position of b)
// pairs over all programs, so row a needs only the programs that hold a:
//   k_prio_prep    the offsets and ids checked (nothing else runs when one is
//                  bad), the sum of len^2 in 64 bits, the histogram over ids
//   k_su_scan      histogram -> the postings' offsets (segsort.h)
//   k_prio_plan    per row: 0 = counted whole, else its slices of `split`
//                  postings; k_su_scan again -> the slices' offsets
//   k_prio_fill    one posting per occurrence: call id -> the program.  The
//                  order inside an id is whatever the atomics give; only
//                  integer sums are taken over it.
//   k_prio_slice   one workgroup per slice of a long row: its postings counted
//                  into a row of u32 in LDS, written to the workspace
//   k_prio_row     one workgroup per row: the row of u32 counters in LDS, zeroed;
//                  for each posting (a, p) every call of p adds 1 to its cell (LDS
//                  atomics); a split row sums its slices' partial rows instead.
//                  Then min(count, 2^24) as float (what float32 `+= 1.0` leaves),
//                  the block reduction of max / min over non-zero cells / nzero,
//                  normalizePrio's expression, the static factor, and the row
//                  written coalesced.  No device-scope atomic touches a cell.
// The sum of len^2 below 2^32 makes every u32 counter and every sum of partial
// rows exact.  The same row kernel without the counting stage is the static
// tail, in place on a given matrix.
//
// Arithmetic.  The reference on amd64 rounds after every float32 operation.
// hipcc contracts a * b + c into a fused multiply-add by default, and the
// __fmul_rn / __fadd_rn intrinsics of this toolchain are plain `*` and `+` that
// the contraction still sees after inlining, so normalizePrio's expression
// lives in prio_norm / prio_min_div under `#pragma clang fp contract(off)`
// (honoured under the default -ffp-contract=fast-honor-pragmas).  Division is
// `/`, which hipcc compiles correctly rounded unless asked otherwise, and
// nothing here is built with fast-math.
#include <algorithm>

#include "segsort.h"
#include "prio_args.h"

namespace syz {

constexpr uint32_t kPrThreads = 256;
constexpr uint32_t kPrGroup = 16;  // the lanes that walk one posting's program (programs have some tens of calls)
constexpr uint32_t kPrCapSmall = 4096, kPrCapLarge = SYZSIG_PRIO_MAX_CALLS;  // cells of the LDS row
constexpr uint32_t kPrClamp = 1u << 24;
constexpr int kPrBadOff = kCntError, kPrBadId = kCntAux, kPrHuge = kCntAux2, kPrPairs = kCntCandidates,
              kPrWhole = kCntTouched, kPrSplit = kCntChanged, kPrSlices = kCntDistinct, kPrBadRow = kCntDefer;
static_assert(kPrCapLarge * 4 <= 64 * 1024, "the row of counters is static LDS");
static_assert(kPrThreads % kPrGroup == 0 && 64 % kPrGroup == 0, "whole groups per wave");

// ---- the inverted index ----

__global__ __launch_bounds__(kPrThreads) void k_prio_prep(const uint64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ id, uint64_t nprog,
                                                          uint64_t total, uint32_t N, uint32_t* hist,
                                                          unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t bad = 0, huge = 0, pairs = 0, bad_id = 0;
	for (uint64_t p = t; p < nprog; p += T) {
		const uint64_t a = off[p], b = off[p + 1];
		if (a > b || b > total || (p == 0 && a != 0) || (p == nprog - 1 && b != total)) {
			bad++;
			continue;
		}
		const uint64_t len = b - a;
		if (len >= 1ull << 16)
			huge++;  // (its square alone is 2^32 or more)
		else
			pairs += len * len;  // (below 2^32 each, fewer than 2^32 programs)
	}
	for (uint64_t i = t; i < total; i += T) {  // (d_call_id has `total` entries whatever the offsets say)
		const uint32_t x = id[i];
		if (x >= N)
			bad_id++;
		else
			atomicAdd(&hist[x], 1u);
	}
	block_count(&cnt[kPrBadOff], bad);
	block_count(&cnt[kPrBadId], bad_id);
	block_count(&cnt[kPrHuge], huge);
	block_count(&cnt[kPrPairs], pairs);
}

// one workgroup: the slices of every row
__global__ __launch_bounds__(kPrThreads) void k_prio_plan(const uint32_t* __restrict__ hist, uint32_t N, uint64_t split,
                                                          uint32_t* nsl, unsigned long long* cnt)
{
	uint64_t whole = 0, cut = 0, slices = 0;
	for (uint32_t a = threadIdx.x; a < N; a += kPrThreads) {
		const uint64_t s = prio_row_slices(hist[a], split);
		nsl[a] = (uint32_t)s;
		whole += s == 0;
		cut += s != 0;
		slices += s;
	}
	block_count(&cnt[kPrWhole], whole);
	block_count(&cnt[kPrSplit], cut);
	block_count(&cnt[kPrSlices], slices);
}

// cur[x] starts at the first posting of id x
__global__ __launch_bounds__(kPrThreads) void k_prio_fill(const uint64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ id, uint64_t nprog,
                                                          uint64_t total, uint32_t N, unsigned long long* cur,
                                                          uint32_t* post)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += T) {
		const uint32_t x = id[i];
		// the program of call i: the first p with off[p + 1] > i (empty programs are stepped over)
		const uint64_t p = su_search<uint64_t>(0, nprog, [&](uint64_t mid) { return off[mid + 1] <= i; });
		if (x >= N || p >= nprog)
			continue;  // (ruled out by k_prio_prep)
		const uint64_t at = atomicAdd(&cur[x], 1ull);
		if (at < total)
			post[at] = (uint32_t)p;
	}
}

// ---- a row ----

// postings [p0, p1): every call of each one's program adds 1 to its cell of the LDS row
__device__ __forceinline__ void prio_count(uint32_t* row, const uint32_t* __restrict__ post, uint64_t p0, uint64_t p1,
                                           const uint64_t* __restrict__ off, const uint32_t* __restrict__ id,
                                           uint32_t N)
{
	const uint32_t g = threadIdx.x / kPrGroup, l = threadIdx.x % kPrGroup;
	for (uint64_t k = p0 + g; k < p1; k += kPrThreads / kPrGroup) {
		const uint32_t p = post[k];
		const uint64_t a = off[p], b = off[p + 1];
		for (uint64_t i = a + l; i < b; i += kPrGroup) {
			const uint32_t x = id[i];
			if (x < N)
				atomicAdd(&row[x], 1u);
		}
	}
}

// normalizePrio's `min /= 2 * float32(nzero)` (prio.go:170), each operation rounded
__device__ __forceinline__ float prio_min_div(float mn, uint32_t nzero)
{
#pragma clang fp contract(off)
	const float d = 2.0f * (float)nzero;
	return mn / d;
}

// normalizePrio's loop body (prio.go:173-184) for one cell, each operation
// rounded on its own, times the static factor (prio.go:32)
__device__ __forceinline__ float prio_norm(float p, float mn, float mx, float factor)
{
#pragma clang fp contract(off)
	if (mx == 0)
		return 1.0f * factor;
	if (p == 0)
		p = mn;
	const float num = p - mn;
	const float den = mx - mn;
	const float q = num / den;
	const float m = q * 0.9f;
	float r = m + 0.1f;
	if (r > 1)
		r = 1;
	return r * factor;
}

struct PrioRed {
	float mx, mn;
	uint32_t nz;
};

// the reduction of normalizePrio's first loop (prio.go:155-168) over the floats
// in the LDS row; every comparison is Go's, so NaN cells take no part and the
// result does not depend on the order
__device__ __forceinline__ PrioRed prio_reduce(const float* row, uint32_t N, float (*s_f)[kPrThreads / 64],
                                               uint32_t* s_u)
{
	float mx = 0.0f, mn = 1e10f;
	uint32_t nz = 0;
	for (uint32_t i = threadIdx.x; i < N; i += kPrThreads) {
		const float p = row[i];
		if (mx < p)
			mx = p;
		if (p != 0 && mn > p)
			mn = p;
		nz += p == 0;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const float omx = __shfl_xor(mx, o, 64), omn = __shfl_xor(mn, o, 64);
		nz += __shfl_xor(nz, o, 64);
		if (mx < omx)
			mx = omx;
		if (mn > omn)
			mn = omn;
	}
	const uint32_t w = threadIdx.x >> 6;
	__syncthreads();  // (the scratch may still be read from the pass before)
	if (lane_id() == 0) {
		s_f[0][w] = mx;
		s_f[1][w] = mn;
		s_u[w] = nz;
	}
	__syncthreads();
	PrioRed r{0.0f, 1e10f, 0};
#pragma unroll
	for (uint32_t k = 0; k < kPrThreads / 64; k++) {
		if (r.mx < s_f[0][k])
			r.mx = s_f[0][k];
		if (r.mn > s_f[1][k])
			r.mn = s_f[1][k];
		r.nz += s_u[k];
	}
	return r;
}

// one slice of a split row: its partial counts to the workspace
template <uint32_t kCap>
__global__ __launch_bounds__(kPrThreads) void k_prio_slice(const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ id,
                                                           const uint32_t* __restrict__ post,
                                                           const uint64_t* __restrict__ post_off,
                                                           const uint64_t* __restrict__ sl_off, uint32_t N,
                                                           uint64_t split, uint64_t nslices, uint32_t* part)
{
	__shared__ uint32_t row[kCap];
	for (uint64_t s = blockIdx.x; s < nslices; s += gridDim.x) {
		// the row of slice s: the first a with sl_off[a + 1] > s
		const uint32_t a = su_search<uint32_t>(0, N, [&](uint32_t mid) { return sl_off[mid + 1] <= s; });
		if (a >= N)
			return;  // (sl_off[N] = nslices: cannot happen)
		for (uint32_t i = threadIdx.x; i < N; i += kPrThreads)
			row[i] = 0;
		__syncthreads();
		const uint64_t p0 = post_off[a] + (s - sl_off[a]) * split, pe = post_off[a + 1];
		prio_count(row, post, p0, std::min(p0 + split, pe), off, id, N);
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < N; i += kPrThreads)
			part[s * N + i] = row[i];
		__syncthreads();
	}
}

// kCount: row blockIdx.x of the dynamic matrix from the postings (or its
// slices), times stat's row if given, to out.  !kCount: the static tail on row
// blockIdx.x of `out`, in place.
template <uint32_t kCap, bool kCount>
__global__ __launch_bounds__(kPrThreads) void k_prio_row(const uint64_t* __restrict__ off,
                                                         const uint32_t* __restrict__ id,
                                                         const uint32_t* __restrict__ post,
                                                         const uint64_t* __restrict__ post_off,
                                                         const uint32_t* __restrict__ nsl,
                                                         const uint64_t* __restrict__ sl_off,
                                                         const uint32_t* __restrict__ part, uint32_t N,
                                                         const float* __restrict__ stat, float* out)
{
	__shared__ uint32_t row[kCap];
	__shared__ float s_f[2][kPrThreads / 64];
	__shared__ uint32_t s_u[kPrThreads / 64];
	float* rowf = reinterpret_cast<float*>(row);
	const uint32_t a = blockIdx.x;  // (the grid is N workgroups)
	float* o = out + (uint64_t)a * N;
	if (kCount) {
		const uint32_t ns = nsl[a];
		if (ns == 0) {
			for (uint32_t i = threadIdx.x; i < N; i += kPrThreads)
				row[i] = 0;
			__syncthreads();
			prio_count(row, post, post_off[a], post_off[a + 1], off, id, N);
			__syncthreads();
			for (uint32_t i = threadIdx.x; i < N; i += kPrThreads)
				rowf[i] = (float)std::min(row[i], kPrClamp);
		} else {
			const uint32_t* pr = part + sl_off[a] * N;
			for (uint32_t i = threadIdx.x; i < N; i += kPrThreads) {
				uint32_t c = 0;
				for (uint32_t k = 0; k < ns; k++)
					c += pr[(uint64_t)k * N + i];  // (all of them together are below 2^32)
				rowf[i] = (float)std::min(c, kPrClamp);
			}
		}
	} else {
		for (uint32_t i = threadIdx.x; i < N; i += kPrThreads)
			rowf[i] = o[i];
		__syncthreads();
		const PrioRed d = prio_reduce(rowf, N, s_f, s_u);  // prio.go:120-127: the diagonal takes the row's max
		if (threadIdx.x == 0)
			rowf[a] = d.mx;
	}
	__syncthreads();
	const PrioRed r = prio_reduce(rowf, N, s_f, s_u);
	const float mn = r.nz ? prio_min_div(r.mn, r.nz) : r.mn;
	const float* st = kCount && stat ? stat + (uint64_t)a * N : nullptr;
	for (uint32_t i = threadIdx.x; i < N; i += kPrThreads) {
		if (st)
			o[i] = prio_norm(rowf[i], mn, r.mx, st[i]);
		else
			o[i] = prio_norm(rowf[i], mn, r.mx, 1.0f);
	}
}

// ---- the choice table ----

// Row blockIdx.x of BuildChoiceTable.  !kWrite: only the weights checked -- a
// bad one counts in cnt[kCntError] and its row goes into cnt[kPrBadRow] as
// N - row (the maximum is the first row).
template <bool kWrite>
__global__ __launch_bounds__(kPrThreads) void k_choice_row(const float* __restrict__ prios,
                                                           const uint8_t* __restrict__ en, uint32_t N, float limit,
                                                           int32_t* run, unsigned long long* cnt)
{
	__shared__ uint32_t s_w[kPrThreads / 64];
	const uint32_t a = blockIdx.x, w = threadIdx.x >> 6;
	const bool row_on = !en || en[a];
	if (!row_on) {
		if (kWrite)
			for (uint32_t j = threadIdx.x; j < N; j += kPrThreads)
				run[(uint64_t)a * N + j] = 0;
		return;
	}
	const float* pr = prios ? prios + (uint64_t)a * N : nullptr;
	uint32_t sum = 0, bad = 0;
	for (uint32_t base = 0; base < N; base += kPrThreads) {
		const uint32_t j = base + threadIdx.x;
		uint32_t x = 0;
		if (j < N && (!en || en[j])) {
			x = 1;
			if (pr) {
				const float f = pr[j] * 1000.0f;  // (one operation: nothing to contract)
				if (!(f >= 0.0f) || f >= limit) {
					bad++;
					x = 0;
				} else {
					x = (uint32_t)(int32_t)f;  // Go's int(): truncation
				}
			}
		}
		if (!kWrite)
			continue;
		const uint32_t incl = wave_incl_scan(x);
		if (lane_id() == 63)
			s_w[w] = incl;
		__syncthreads();
		uint32_t wb = 0, tot = 0;
#pragma unroll
		for (uint32_t k = 0; k < kPrThreads / 64; k++) {
			wb += k < w ? s_w[k] : 0;
			tot += s_w[k];
		}
		if (j < N)
			run[(uint64_t)a * N + j] = (int32_t)(sum + wb + incl);  // (N weights below 2^31 / N each)
		sum += tot;
		__syncthreads();
	}
	if (!kWrite && bad) {
		atomicAdd(&cnt[kCntError], (unsigned long long)bad);
		atomicMax(&cnt[kPrBadRow], (unsigned long long)(N - a));
	}
}

// one lane per query
template <bool kWrite>
__global__ __launch_bounds__(kPrThreads) void k_choice_lookup(const int32_t* __restrict__ run, uint32_t N,
                                                              const int32_t* __restrict__ call,
                                                              const int32_t* __restrict__ xs, uint64_t n, int32_t* out,
                                                              unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad = 0;
	for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += T) {
		const int32_t c = call[q], x = xs[q];
		int32_t r = (int32_t)N;  // call < 0, or a nil row: uniform over enabledCalls
		if (c >= (int32_t)N) {
			bad++;
			continue;
		}
		if (c >= 0) {
			const int32_t* row = run + (uint64_t)c * N;
			const int32_t total = row[N - 1];
			if (total > 0) {
				if (x < 1 || x > total) {
					bad++;
					continue;
				}
				r = (int32_t)su_search<uint32_t>(0, N, [&](uint32_t mid) { return row[mid] < x; });
			}
		}
		if (kWrite)
			out[q] = r;
	}
	if (!kWrite)
		block_count(&cnt[kCntError], bad);
}

static int prio_fail(const PrioStatus& a) { return fail(a.code, a.msg); }

#define SYZ_PARGS(expr)                                                            \
	do {                                                                           \
		const syz::PrioStatus a__ = (expr);                                        \
		if (a__.code != SYZSIG_OK)                                                 \
			return syz::prio_fail(a__);                                            \
	} while (0)

// the workspace of one calc_prios call
struct PrioMeta {
	uint32_t *hist, *nsl;
	uint64_t *post_off, *cur, *sl_off;
};

static int prio_meta(syzsig_ctx* ctx, uint64_t N, PrioMeta* m)
{
	const size_t a32 = align256(N * 4), a64 = align256((N + 1) * 8);
	char* p;
	SYZ_TRY(ws_get(ctx, kWsPqMeta, 2 * a32 + 3 * a64, (void**)&p));
	m->hist = (uint32_t*)p;
	m->nsl = (uint32_t*)(p + a32);
	m->post_off = (uint64_t*)(p + 2 * a32);
	m->cur = (uint64_t*)(p + 2 * a32 + a64);
	m->sl_off = (uint64_t*)(p + 2 * a32 + 2 * a64);
	return SYZSIG_OK;
}

template <uint32_t kCap>
static int prio_rows(syzsig_ctx* ctx, const uint64_t* d_off, const uint32_t* d_id, const uint32_t* post,
                     const PrioMeta& m, uint32_t N, uint64_t split, uint64_t nslices, const float* d_static,
                     float* d_prios)
{
	const hipStream_t s = ctx->stream;
	uint32_t* part = nullptr;
	if (nslices) {
		SYZ_TRY(ws_get(ctx, kWsPqPart, nslices * N * 4, (void**)&part));
		k_prio_slice<kCap><<<grid_cap(nslices), kPrThreads, 0, s>>>(d_off, d_id, post, m.post_off, m.sl_off, N, split,
		                                                           nslices, part);
	}
	k_prio_row<kCap, true><<<N, kPrThreads, 0, s>>>(d_off, d_id, post, m.post_off, m.nsl, m.sl_off, part, N, d_static,
	                                               d_prios);
	SYZ_HIP(hipGetLastError());
	return SYZSIG_OK;
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_calc_prios_dev(syzsig_ctx* ctx, const uint64_t* d_prog_off, const uint32_t* d_call_id,
                                     uint64_t nprog, uint64_t total, uint64_t N, uint64_t split, const float* d_static,
                                     float* d_prios)
{
	SYZ_LOCK(ctx);
	SYZ_PARGS(calc_prios_args(ctx, d_prog_off, d_call_id, nprog, total, N, d_prios));
	std::fill(ctx->pq_stats, ctx->pq_stats + 4, 0);
	const hipStream_t s = ctx->stream;
	const uint32_t n = (uint32_t)N;
	const uint64_t sp = prio_split(split, total, N);
	PrioMeta m;
	SYZ_TRY(prio_meta(ctx, N, &m));
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	SYZ_HIP(hipMemsetAsync(m.hist, 0, N * 4, s));
	k_prio_prep<<<grid_for(std::max(nprog, total), kPrThreads), kPrThreads, 0, s>>>(d_prog_off, d_call_id, nprog, total,
	                                                                               n, m.hist, ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(m.hist, N, m.post_off);
	k_prio_plan<<<1, kPrThreads, 0, s>>>(m.hist, n, sp, m.nsl, ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(m.nsl, N, m.sl_off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	const unsigned long long* h = ctx->h_cnt;
	SYZ_PARGS(calc_prios_corpus_status(h[kPrBadOff], h[kPrBadId], h[kPrHuge], h[kPrPairs]));
	const uint64_t nslices = h[kPrSlices], whole = h[kPrWhole], cut = h[kPrSplit], pairs = h[kPrPairs];
	uint32_t* post = nullptr;
	if (total) {
		SYZ_TRY(ws_get(ctx, kWsPqPost, total * 4, (void**)&post));
		SYZ_HIP(hipMemcpyAsync(m.cur, m.post_off, (N + 1) * 8, hipMemcpyDeviceToDevice, s));
		k_prio_fill<<<grid_for(total, kPrThreads), kPrThreads, 0, s>>>(d_prog_off, d_call_id, nprog, total, n,
		                                                              (unsigned long long*)m.cur, post);
	}
	if (N <= kPrCapSmall)
		SYZ_TRY(prio_rows<kPrCapSmall>(ctx, d_prog_off, d_call_id, post, m, n, sp, nslices, d_static, d_prios));
	else
		SYZ_TRY(prio_rows<kPrCapLarge>(ctx, d_prog_off, d_call_id, post, m, n, sp, nslices, d_static, d_prios));
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	ctx->pq_stats[0] = whole;
	ctx->pq_stats[1] = cut;
	ctx->pq_stats[2] = nslices;
	ctx->pq_stats[3] = pairs;
	return SYZSIG_OK;
}

extern "C" int syzsig_prio_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::pq_stats, out, "prio_stats");
}

extern "C" int syzsig_static_prio_finish_dev(syzsig_ctx* ctx, float* d_prios, uint64_t N)
{
	SYZ_LOCK(ctx);
	SYZ_PARGS(static_finish_args(ctx, d_prios, N));
	const hipStream_t s = ctx->stream;
	SYZ_TRY(su_time_begin(ctx));
	if (N <= kPrCapSmall)
		k_prio_row<kPrCapSmall, false><<<(uint32_t)N, kPrThreads, 0, s>>>(nullptr, nullptr, nullptr, nullptr, nullptr,
		                                                                 nullptr, nullptr, (uint32_t)N, nullptr, d_prios);
	else
		k_prio_row<kPrCapLarge, false><<<(uint32_t)N, kPrThreads, 0, s>>>(nullptr, nullptr, nullptr, nullptr, nullptr,
		                                                                 nullptr, nullptr, (uint32_t)N, nullptr, d_prios);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

extern "C" int syzsig_choice_table_dev(syzsig_ctx* ctx, const float* d_prios, const uint8_t* d_enabled, uint64_t N,
                                       int32_t* d_run)
{
	SYZ_LOCK(ctx);
	SYZ_PARGS(choice_table_args(ctx, N, d_run));
	const hipStream_t s = ctx->stream;
	const uint32_t n = (uint32_t)N;
	const float limit = choice_weight_limit(N);
	SYZ_TRY(su_time_begin(ctx));
	if (d_prios) {  // (weights of 1 cannot be bad)
		SYZ_TRY(counters_reset(ctx));
		k_choice_row<false><<<n, kPrThreads, 0, s>>>(d_prios, d_enabled, n, limit, nullptr, ctx->d_cnt);
		SYZ_HIP(hipGetLastError());
		SYZ_TRY(counters_fetch(ctx));
		if (ctx->h_cnt[kCntError])
			return fail(SYZSIG_EINVAL, "choice_table: row " + std::to_string(N - ctx->h_cnt[kPrBadRow]) +
			                               " has a weight that is NaN, negative or 2^31 / N or more (" +
			                               std::to_string(ctx->h_cnt[kCntError]) + " such weights in all)");
	}
	k_choice_row<true><<<n, kPrThreads, 0, s>>>(d_prios, d_enabled, n, limit, d_run, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

extern "C" int syzsig_choice_lookup_dev(syzsig_ctx* ctx, const int32_t* d_run, uint64_t N, const int32_t* d_call,
                                        const int32_t* d_x, uint64_t n, int32_t* d_out)
{
	SYZ_LOCK(ctx);
	SYZ_PARGS(choice_lookup_args(ctx, d_run, N, d_call, d_x, n, d_out));
	if (n == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_choice_lookup<false><<<grid_for(n, kPrThreads), kPrThreads, 0, s>>>(d_run, (uint32_t)N, d_call, d_x, n, nullptr,
	                                                                     ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "choice_lookup: " + std::to_string(ctx->h_cnt[kCntError]) +
		                               " queries with a call >= N or an x outside [1, total]");
	k_choice_lookup<true><<<grid_for(n, kPrThreads), kPrThreads, 0, s>>>(d_run, (uint32_t)N, d_call, d_x, n, d_out,
	                                                                    ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}
