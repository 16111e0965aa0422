// calls.hip -- the calls of a batch of programs from their text: the head of
// every line, and nothing else of it (syzsig_prog_calls_dev), and the call-name
// table it looks names up in (syzsig_calltab).
//
// References:
//   prog/encoding.go:153-180   Deserialize's loop head: skip, Ident, '=', Ident,
//       the SyscallMap lookup, Parse('(')
//   prog/encoding.go:734-828   the parser: bufio.Scanner with a 1 MiB buffer, Ident, Char, Parse
//   prog/encoding.go:836-869   CallSet
//   syz-manager/manager.go:209-240, :888-896   the two per-program host loops this replaces
// The rules of a line and of a head are calls_core.h's; this file is where the
// bytes come from and where the results go.
//
// Kernels, T = SYZSIG_PROGTEXT_TILE bytes per workgroup (16 per lane, one
// coalesced load each), W = SYZSIG_PROGTEXT_WINDOW bytes staged behind them:
//   k_pc_prep       the offsets checked against each other and nbytes
//   k_pc_tiles<0>   per tile: the text into LDS, the starts of the programs in
//                   the tile as bits in LDS (a binary search for the first, then
//                   the offsets in order), the line starts -- a program's start,
//                   or the byte behind a '\n' -- as one 16-bit mask per lane, and
//                   their number
//   k_su_scan       the tiles' counts -> every line's ordinal in the batch
//   k_pc_tiles<1>   the same again, then: each program's first line ordinal
//                   (the rank of its offset among the tile's line starts), and
//                   one lane per line start parses the head from LDS and looks
//                   the name up; the line's start and its record go to the
//                   line's ordinal.  A head that does not end within the W bytes
//                   from its line's start (all staged, wherever in the tile the
//                   line starts) is listed.
//   k_pc_long       the list, one lane per head, the same scanner over global
//                   memory in 16-byte loads, bounded by the line's end, which the
//                   next line's start gives; a line of 2^20 bytes is not scanned
//   k_pc_reduce     a wave per program over its lines' records: the first error
//                   and its line number, the calls' number, the flags.  The
//                   too-long check is here, from the starts of neighbouring lines.
//   k_su_scan, k_pc_write   the counts -> offsets -> the ids in line order
//   CallSet mode: k_pc_write into a staging buffer, segsort.h's sort-unique per
//                   program, k_su_scan, k_su_gather.
// Order comes from the line ordinals alone; the only atomics whose order varies
// fill the long list, whose entries name their lines.  Every loop is bounded by
// a line's end, the window, a program's lines or the number of programs.
//
// The name table stays in global memory (L2): with a few thousand names its
// slots and bytes are some hundred KiB, more than a workgroup's LDS beside the
// tile, and a probe is one 16-byte slot and the name's bytes.
#include <algorithm>
#include <vector>

#include "segsort.h"
// (after segsort.h: the two below take syzsig.h's codes from their includer)
#include "calls_args.h"

struct syzsig_calltab {
	syzsig_ctx* ctx = nullptr;
	syz::CallSlot* slots = nullptr;
	uint8_t* names = nullptr;
	uint64_t* name_off = nullptr;
	uint64_t mask = 0, n = 0;
};

namespace syz {

constexpr uint32_t kPcTile = SYZSIG_PROGTEXT_TILE, kPcWin = SYZSIG_PROGTEXT_WINDOW, kPcThreads = 256;
constexpr uint32_t kPcStage = kPcTile + kPcWin, kPcChunks = kPcStage / 16, kPcSortTile = SYZSIG_PROGTEXT_SORT_TILE;
static_assert(kPcTile == kPcThreads * 16 && kPcWin % 32 == 0 && kPcWin <= kPcThreads * 16, "a lane loads one 16-byte chunk");
constexpr int kPcSkip = kCntInserted, kPcInWin = kCntOverflow, kPcLong = kCntAggOvf, kPcPending = kCntSpill;

using PcSortTile = SuU32Tile<kPcSortTile>;

struct PcText {
	const uint8_t* data;
	uint64_t nbytes;
	const uint64_t* off;
	uint64_t nprog;
};

// 16 bytes from position a (a multiple of 16) on; zeros past nbytes
__device__ __forceinline__ uint4 pc_load16(const uint8_t* __restrict__ data, uint64_t nbytes, uint64_t a)
{
	if (a + 16 <= nbytes)
		return *reinterpret_cast<const uint4*>(data + a);
	uint32_t w[4] = {0, 0, 0, 0};
	for (uint32_t k = 0; k < 16 && a + k < nbytes; k++)
		w[k >> 2] |= (uint32_t)data[a + k] << (8 * (k & 3));
	return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit k = byte k of the word is '\n'
__device__ __forceinline__ uint32_t pc_nl4(uint32_t w)
{
	uint32_t m = 0;
#pragma unroll
	for (int k = 0; k < 4; k++)
		m |= (uint32_t)(((w >> (8 * k)) & 0xff) == '\n') << k;
	return m;
}

__global__ __launch_bounds__(256) void k_pc_prep(PcText X, unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < X.nprog; i += T) {
		const uint64_t a = X.off[i], b = X.off[i + 1];
		bad += a > b || b > X.nbytes;
	}
	block_count(&cnt[kCntError], bad);
}

// a line's surroundings in the staged tile, positions relative to the tile
struct PcLdsSrc {
	const uint8_t* text;
	const uint32_t* ps;
	uint64_t p0, end, lim;
	__device__ __forceinline__ int byte(uint64_t q) const { return text[q]; }
	__device__ __forceinline__ bool ends_before(uint64_t q) const
	{
		return q >= end || (q > p0 && ((ps[q >> 5] >> (q & 31)) & 1));
	}
};

// a line's surroundings in global memory: [.., end) is the line, 16 bytes cached
struct PcGlobSrc {
	const uint8_t* data;
	uint64_t nbytes, end, lim;
	mutable uint64_t cur, lo, hi;
	__device__ __forceinline__ int byte(uint64_t q) const
	{
		if ((q >> 4) != cur) {
			cur = q >> 4;
			const uint4 v = pc_load16(data, nbytes, cur << 4);
			lo = v.x | (uint64_t)v.y << 32;
			hi = v.z | (uint64_t)v.w << 32;
		}
		return (int)((((q & 8) ? hi : lo) >> ((q & 7) * 8)) & 0xff);
	}
	__device__ __forceinline__ bool ends_before(uint64_t q) const { return q >= end; }
};

struct PcTileOut {
	const uint64_t* tile_base;  // kParse
	uint64_t* first_line;       // [nprog + 1]
	uint64_t* pos;              // [nlines + 1]
	uint32_t* rec;
	uint64_t nlines;
	uint64_t* list;
	uint64_t list_cap;
	uint32_t* tile_cnt;  // !kParse
};

template <bool kParse>
__global__ __launch_bounds__(kPcThreads) void k_pc_tiles(PcText X, uint32_t mode, CallTabView tab, PcTileOut O,
                                                         unsigned long long* cnt)
{
	__shared__ uint4 s_text[kPcChunks];
	__shared__ uint32_t s_ps[kPcStage / 32];
	__shared__ uint32_t s_ls[kPcThreads], s_pre[kPcThreads], s_w[kPcThreads / 64];
	__shared__ uint64_t s_i0;
	const uint32_t tid = threadIdx.x;
	const uint64_t t0 = (uint64_t)blockIdx.x * kPcTile;
	const uint64_t off0 = X.off[0], E = X.off[X.nprog];
	const uint4 mine = pc_load16(X.data, X.nbytes, t0 + tid * 16);
	s_text[tid] = mine;
	if (tid < kPcWin / 16)
		s_text[kPcThreads + tid] = pc_load16(X.data, X.nbytes, t0 + kPcTile + tid * 16);
	if (tid < kPcStage / 32)
		s_ps[tid] = 0;
	if (tid == 0)
		s_i0 = su_search<uint64_t>(0, X.nprog, [&](uint64_t mid) { return X.off[mid] < t0; });
	__syncthreads();
	const uint64_t i0 = s_i0;
	// the programs that start in [t0, t0 + kPcStage): their starts as bits (an empty one starts no line)
	for (uint64_t b = i0;; b += kPcThreads) {
		const uint64_t i = b + tid;
		bool in = false;
		if (i < X.nprog) {
			const uint64_t a = X.off[i];
			in = a < t0 + kPcStage;
			if (in && a >= t0 && X.off[i + 1] > a)
				atomicOr(&s_ps[(a - t0) >> 5], 1u << ((a - t0) & 31));
		}
		if (!__syncthreads_or(tid == kPcThreads - 1 && in))
			break;
	}
	__syncthreads();
	// the line starts of this lane's 16 bytes
	const uint32_t nl = pc_nl4(mine.x) | pc_nl4(mine.y) << 4 | pc_nl4(mine.z) << 8 | pc_nl4(mine.w) << 12;
	const uint64_t a0 = t0 + tid * 16;
	bool prev = false;
	if (tid)
		prev = reinterpret_cast<const uint8_t*>(s_text)[tid * 16 - 1] == '\n';
	else if (t0 && t0 <= X.nbytes)
		prev = X.data[t0 - 1] == '\n';
	const uint32_t ps16 = (s_ps[tid >> 1] >> ((tid & 1) * 16)) & 0xffff;
	uint32_t valid = 0;
	if (a0 + 16 > off0 && a0 < E) {
		valid = 0xffff;
		if (a0 < off0)
			valid &= 0xffffu << (off0 - a0);
		if (E - a0 < 16)
			valid &= (1u << (E - a0)) - 1;
	}
	const uint32_t ls = ((((nl << 1) | (uint32_t)prev) & 0xffff) | ps16) & valid;
	const uint32_t c = __popc(ls);
	const uint32_t incl = wave_incl_scan(c);
	if (lane_id() == 63)
		s_w[tid >> 6] = incl;
	__syncthreads();
	uint32_t wb = 0, total = 0;
#pragma unroll
	for (uint32_t k = 0; k < kPcThreads / 64; k++) {
		wb += k < (tid >> 6) ? s_w[k] : 0;
		total += s_w[k];
	}
	if (!kParse) {
		if (tid == 0)
			O.tile_cnt[blockIdx.x] = total;
		return;
	}
	const uint64_t base = O.tile_base[blockIdx.x];
	s_ls[tid] = ls;
	s_pre[tid] = wb + incl - c;
	if (blockIdx.x == 0 && tid == 0)
		O.pos[O.nlines] = E;
	__syncthreads();
	// every offset in [t0, t0 + kPcTile), the last one included: the line starts before it
	for (uint64_t b = i0;; b += kPcThreads) {
		const uint64_t i = b + tid;
		bool in = false;
		if (i <= X.nprog) {
			const uint64_t a = X.off[i];
			in = a < t0 + kPcTile;
			if (in && a >= t0) {
				const uint32_t r = (uint32_t)(a - t0);
				O.first_line[i] = base + s_pre[r >> 4] + __popc(s_ls[r >> 4] & ((1u << (r & 15)) - 1));
			}
		}
		if (!__syncthreads_or(tid == kPcThreads - 1 && in))
			break;
	}
	// one lane per line start
	uint64_t nskip = 0, nwin = 0;
	uint64_t g = base + wb + incl - c;
	for (uint32_t m = ls; m; m &= m - 1, g++) {
		const uint32_t p = tid * 16 + (__ffs(m) - 1);
		const PcLdsSrc S{reinterpret_cast<const uint8_t*>(s_text), s_ps, p, E - t0, p + kPcWin};  // (p + kPcWin <= kPcStage)
		const uint32_t r = line_record(S, p, mode, tab);
		if (g >= O.nlines)  // (the count pass saw the same bytes: cannot happen)
			break;
		O.pos[g] = t0 + p;
		O.rec[g] = r;
		if (r == kRecPending) {
			const uint64_t x = atomicAdd(&cnt[kPcLong], 1ull);
			if (x < O.list_cap)  // (a listed line has kPcWin - 1 bytes at the least: cannot fail)
				O.list[x] = g;
		} else {
			nwin += r != kRecSkip;
			nskip += r == kRecSkip;
		}
	}
	block_count(&cnt[kPcSkip], nskip);
	block_count(&cnt[kPcInWin], nwin);
}

__global__ __launch_bounds__(64) void k_pc_long(PcText X, uint32_t mode, CallTabView tab, const uint64_t* __restrict__ pos,
                                                uint32_t* rec, const uint64_t* __restrict__ list, uint64_t list_cap,
                                                unsigned long long* cnt)
{
	const uint64_t n = std::min<uint64_t>(cnt[kPcLong], list_cap), T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t nskip = 0;
	for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += T) {
		const uint64_t g = list[x], a = pos[g], b = pos[g + 1];
		if (a >= b || b > X.nbytes)
			continue;  // (line starts ascend inside the text: cannot happen; the record stays pending)
		const uint64_t end = b - (X.data[b - 1] == '\n');
		if (end - a >= kPtMaxLine)
			continue;  // k_pc_reduce fails the program without the head
		const PcGlobSrc S{X.data, X.nbytes, end, ~0ull, ~0ull, 0, 0};
		const uint32_t r = line_record(S, a, mode, tab);
		rec[g] = r;
		nskip += r == kRecSkip;
	}
	nskip = wave_sum_u64(nskip);
	if (threadIdx.x == 0 && nskip)
		atomicAdd(&cnt[kPcSkip], (unsigned long long)nskip);
}

struct PcProgOut {
	uint8_t* status;
	uint32_t* err_line;
	uint8_t* flag;
	uint32_t* seg_len;
};

// line g's record with the too-long rule applied (the line's length before its '\n', the '\r' counted)
__device__ __forceinline__ uint32_t pc_record(const PcText& X, const uint64_t* __restrict__ pos,
                                              const uint32_t* __restrict__ rec, uint64_t g)
{
	const uint64_t a = pos[g], b = pos[g + 1];
	if (a >= b || b > X.nbytes)
		return kRecPending;  // (cannot happen: reported as an internal error)
	if (b - a >= kPtMaxLine && b - a - (X.data[b - 1] == '\n') >= kPtMaxLine)
		return kRecErr | SYZSIG_PT_LINE_TOO_LONG;
	return rec[g];
}

// a wave per program
__global__ __launch_bounds__(256) void k_pc_reduce(PcText X, uint32_t mode, const uint8_t* __restrict__ enabled,
                                                   const uint64_t* __restrict__ first_line,
                                                   const uint64_t* __restrict__ pos, const uint32_t* __restrict__ rec,
                                                   uint64_t nlines, PcProgOut O, unsigned long long* cnt)
{
	const uint32_t lane = lane_id();
	const uint64_t W = (uint64_t)gridDim.x * 4;
	for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < X.nprog; i += W) {
		const uint64_t b = std::min(first_line[i + 1], nlines), a = std::min(first_line[i], b);
		uint64_t ncall = 0, nunk = 0, err_at = 0;
		uint32_t status = SYZSIG_PT_OK;
		bool dis = false, pending = false;
		for (uint64_t k = a; k < b && status == SYZSIG_PT_OK; k += 64) {
			const uint64_t g = k + lane;
			const uint32_t r = g < b ? pc_record(X, pos, rec, g) : kRecSkip;
			const uint32_t kind = r & kRecKindMask;
			const uint64_t em = __ballot(kind == kRecErr || kind == kRecPending);
			const uint64_t before = em ? (1ull << (__ffsll((unsigned long long)em) - 1)) - 1 : ~0ull;
			if (em) {
				const int src = __ffsll((unsigned long long)em) - 1;
				const uint32_t r0 = __shfl(r, src, 64);
				pending = (r0 & kRecKindMask) == kRecPending;
				status = pending ? SYZSIG_PT_BAD_HEAD : (r0 & kRecValMask);
				err_at = k + src - a + 1;
			}
			ncall += __popcll(__ballot(kind == kRecCall) & before);
			nunk += __popcll(__ballot(kind == kRecUnknown) & before);
			const bool off_call = kind == kRecCall && enabled && !enabled[r & kRecValMask];
			dis = dis || (__ballot(off_call) & before) != 0;
		}
		if (lane)
			continue;
		if (pending)
			atomicAdd(&cnt[kPcPending], 1ull);
		uint32_t len = 0, flag = 0;
		if (status == SYZSIG_PT_OK) {
			if (mode == SYZSIG_PROGTEXT_CALLSET) {
				if (ncall + nunk == 0)
					status = SYZSIG_PT_NO_CALLS;
				else
					flag = (uint32_t)(!nunk && !dis) | (nunk ? 2u : 0u);
			} else {
				flag = dis;
			}
		}
		if (status == SYZSIG_PT_OK)
			len = (uint32_t)std::min<uint64_t>(ncall, 0xffffffffull);
		O.status[i] = (uint8_t)status;
		O.err_line[i] = (uint32_t)std::min<uint64_t>(err_at, 0xffffffffull);
		O.flag[i] = (uint8_t)flag;
		O.seg_len[i] = len;
	}
}

// the OK programs' known ids in line order, program i's from out[woff[i]] on
__global__ __launch_bounds__(256) void k_pc_write(uint64_t nprog, const uint64_t* __restrict__ first_line,
                                                  const uint32_t* __restrict__ rec, const uint32_t* __restrict__ seg_len,
                                                  const uint64_t* __restrict__ woff, uint64_t nlines, uint32_t* out,
                                                  uint64_t cap)
{
	const uint32_t lane = lane_id();
	const uint64_t W = (uint64_t)gridDim.x * 4;
	for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nprog; i += W) {
		const uint64_t b = std::min(first_line[i + 1], nlines), a = std::min(first_line[i], b), n = seg_len[i], o = woff[i];
		uint64_t done = 0;
		for (uint64_t k = a; k < b && done < n; k += 64) {
			const uint32_t r = k + lane < b ? rec[k + lane] : kRecSkip;
			const bool call = (r & kRecKindMask) == kRecCall;
			const uint64_t m = __ballot(call);
			const uint64_t at = done + lane_rank(m);
			if (call && at < n && o + at < cap)  // (the counts are k_pc_reduce's over the same records)
				out[o + at] = r & kRecValMask;
			done += __popcll(m);
		}
	}
}

__global__ __launch_bounds__(256) void k_pc_seglens(const uint32_t* __restrict__ len, uint64_t nseg, unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t nl = 0, nt = 0, nk = 0;
	for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += T)
		su_count_large<PcSortTile::kTile, PcSortTile::kAlign>(len[s], nl, nt, nk, cnt);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
}

static int pc_arg_fail(const ArgStatus& a) { return fail(a.code, a.msg); }

#define SYZ_PC_ARGS(expr)                                                          \
	do {                                                                           \
		const syz::ArgStatus a__ = (expr);                                         \
		if (a__.code != SYZSIG_OK)                                                 \
			return syz::pc_arg_fail(a__);                                          \
	} while (0)

}  // namespace syz

using namespace syz;

extern "C" int syzsig_calltab_make(syzsig_ctx* ctx, const uint8_t* names, const uint64_t* name_off, uint64_t n,
                                   syzsig_calltab** out)
{
	SYZ_LOCK(ctx);
	SYZ_PC_ARGS(calltab_args(ctx, names, name_off, n, out));
	std::vector<CallSlot> slots;
	SYZ_PC_ARGS(calltab_build(names, name_off, n, slots));
	syzsig_calltab* t = new syzsig_calltab();
	t->ctx = ctx;
	t->n = n;
	t->mask = slots.size() - 1;
	const hipStream_t s = ctx->stream;
	hipError_t e = hipMalloc((void**)&t->slots, slots.size() * sizeof(CallSlot));
	if (e == hipSuccess)
		e = hipMalloc((void**)&t->names, name_off[n]);
	if (e == hipSuccess)
		e = hipMalloc((void**)&t->name_off, (n + 1) * 8);
	if (e == hipSuccess)
		e = hipMemcpyAsync(t->slots, slots.data(), slots.size() * sizeof(CallSlot), hipMemcpyHostToDevice, s);
	if (e == hipSuccess)
		e = hipMemcpyAsync(t->names, names, name_off[n], hipMemcpyHostToDevice, s);
	if (e == hipSuccess)
		e = hipMemcpyAsync(t->name_off, name_off, (n + 1) * 8, hipMemcpyHostToDevice, s);
	if (e == hipSuccess)
		e = hipStreamSynchronize(s);
	if (e != hipSuccess) {
		(void)hipFree(t->slots);
		(void)hipFree(t->names);
		(void)hipFree(t->name_off);
		delete t;
		return hip_fail(e, "calltab_make", __FILE__, __LINE__);
	}
	*out = t;
	return SYZSIG_OK;
}

extern "C" void syzsig_calltab_free(syzsig_calltab* t)
{
	if (!t)
		return;
	{
		SYZ_LOCK(t->ctx);
		(void)hipStreamSynchronize(t->ctx->stream);
		(void)hipFree(t->slots);
		(void)hipFree(t->names);
		(void)hipFree(t->name_off);
	}
	delete t;
}

extern "C" uint64_t syzsig_calltab_len(const syzsig_calltab* t) { return t ? t->n : 0; }

extern "C" int syzsig_prog_calls_dev(syzsig_ctx* ctx, const syzsig_calltab* tab, const uint8_t* d_data, uint64_t nbytes,
                                     const uint64_t* d_off, uint64_t nprog, uint32_t mode, const uint8_t* d_enabled,
                                     uint64_t* d_call_off, uint32_t* d_call_id, uint64_t cap, uint8_t* d_status,
                                     uint32_t* d_err_line, uint8_t* d_flag, uint64_t* total)
{
	SYZ_LOCK(ctx);
	if (total)
		*total = 0;
	SYZ_PC_ARGS(prog_calls_args(ctx, tab, d_data, nbytes, d_off, nprog, mode, d_call_off, d_call_id, cap, d_status,
	                            d_err_line, d_flag, total));
	std::fill(ctx->pc_stats, ctx->pc_stats + 4, 0);
	const hipStream_t s = ctx->stream;
	if (nprog == 0) {
		SYZ_HIP(hipMemsetAsync(d_call_off, 0, 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	const bool callset = mode == SYZSIG_PROGTEXT_CALLSET;
	const PcText X{d_data, nbytes, d_off, nprog};
	const CallTabView T{tab->slots, tab->mask, tab->names, tab->name_off, (uint32_t)tab->n};
	const uint64_t ntiles = nbytes / kPcTile + 1;  // (position nbytes has a tile: the last offset may be there)
	// tile_cnt, tile_base; first_line; the outputs held back: status, err_line, flag, call_off; seg_len, roff, ucnt
	char* m;
	const size_t o_tb = align256(ntiles * 4), o_fl = o_tb + align256((ntiles + 1) * 8),
	             o_st = o_fl + align256((nprog + 1) * 8), o_el = o_st + align256(nprog),
	             o_fg = o_el + align256(nprog * 4), o_co = o_fg + align256(nprog),
	             o_sl = o_co + align256((nprog + 1) * 8), o_ro = o_sl + align256(nprog * 4),
	             o_uc = o_ro + align256((nprog + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsPcMeta, o_uc + align256(nprog * 4), (void**)&m));
	uint32_t *tile_cnt = (uint32_t*)m, *err_line = (uint32_t*)(m + o_el), *seg_len = (uint32_t*)(m + o_sl),
	         *ucnt = (uint32_t*)(m + o_uc);
	uint64_t *tile_base = (uint64_t*)(m + o_tb), *first_line = (uint64_t*)(m + o_fl), *coff = (uint64_t*)(m + o_co),
	         *roff = (uint64_t*)(m + o_ro);
	uint8_t *status = (uint8_t*)(m + o_st), *flag = (uint8_t*)(m + o_fg);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_pc_prep<<<grid_for(nprog, 256), 256, 0, s>>>(X, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	SYZ_PC_ARGS(prog_calls_offsets_status(ctx->h_cnt[kCntError]));
	PcTileOut O{};
	O.tile_cnt = tile_cnt;
	k_pc_tiles<false><<<(unsigned)ntiles, kPcThreads, 0, s>>>(X, mode, T, O, ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(tile_cnt, ntiles, tile_base);
	SYZ_HIP(hipGetLastError());
	uint64_t nlines = 0;
	SYZ_HIP(hipMemcpyAsync(&nlines, tile_base + ntiles, 8, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipStreamSynchronize(s));
	char* lines;
	uint64_t* list;
	const size_t o_rec = align256((nlines + 1) * 8);
	const uint64_t list_cap = prog_calls_long_cap(nbytes);
	SYZ_TRY(ws_get(ctx, kWsPcLines, o_rec + align256(nlines * 4) + 256, (void**)&lines));
	SYZ_TRY(ws_get(ctx, kWsPcList, list_cap * 8, (void**)&list));
	uint64_t* pos = (uint64_t*)lines;
	uint32_t* rec = (uint32_t*)(lines + o_rec);
	O = PcTileOut{tile_base, first_line, pos, rec, nlines, list, list_cap, nullptr};
	k_pc_tiles<true><<<(unsigned)ntiles, kPcThreads, 0, s>>>(X, mode, T, O, ctx->d_cnt);
	k_pc_long<<<(unsigned)std::min<uint64_t>((list_cap + 63) / 64, 1024), 64, 0, s>>>(X, mode, T, pos, rec, list, list_cap,
	                                                                                 ctx->d_cnt);
	const unsigned pgrid = (unsigned)std::min<uint64_t>((nprog + 3) / 4, 1u << 16);
	k_pc_reduce<<<pgrid, 256, 0, s>>>(X, mode, d_enabled, first_line, pos, rec, nlines, PcProgOut{status, err_line, flag, seg_len},
	                                  ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(seg_len, nprog, callset ? roff : coff);
	if (callset)
		k_pc_seglens<<<grid_for(nprog, 256), 256, 0, s>>>(seg_len, nprog, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	uint64_t raw = 0, need = 0;
	SYZ_HIP(hipMemcpyAsync(&raw, (callset ? roff : coff) + nprog, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kPcPending])
		return fail(SYZSIG_EIO, "prog_calls: internal: a listed head was left undecided");
	ctx->pc_stats[0] = nlines;
	ctx->pc_stats[1] = ctx->h_cnt[kPcSkip];
	ctx->pc_stats[2] = ctx->h_cnt[kPcInWin];
	ctx->pc_stats[3] = ctx->h_cnt[kPcLong];
	const bool sizing = d_call_id == nullptr;
	if (!callset) {
		need = raw;
		*total = need;
		SYZ_PC_ARGS(prog_calls_room(need, cap, sizing));
		if (!sizing && need)
			k_pc_write<<<pgrid, 256, 0, s>>>(nprog, first_line, rec, seg_len, coff, nlines, d_call_id, cap);
	} else {
		SYZ_PC_ARGS(prog_calls_room(raw, ~0ull, true));
		uint32_t *stage, *stage2;
		SYZ_TRY(ws_get(ctx, kWsPcStage, raw * 4 + 256, (void**)&stage));
		SYZ_TRY(ws_get(ctx, kWsPcStage2, raw * 4 + 256, (void**)&stage2));
		if (raw)
			k_pc_write<<<pgrid, 256, 0, s>>>(nprog, first_line, rec, seg_len, roff, nlines, stage, raw);
		const SuSegs S{stage, 1, roff, seg_len, 1, seg_len, nprog};
		const SuOutKeys<SuU32> pol{stage2, roff, 1, ucnt};
		SYZ_TRY((su_sort_unique<PcSortTile, SuOutKeys<SuU32>>(ctx, S, pol)));
		k_su_scan<<<1, kSuThreads, 0, s>>>(ucnt, nprog, coff);
		SYZ_HIP(hipGetLastError());
		SYZ_HIP(hipMemcpyAsync(&need, coff + nprog, 8, hipMemcpyDeviceToHost, s));
		SYZ_TRY(counters_fetch(ctx));
		if (ctx->h_cnt[kCntError])
			return fail(SYZSIG_EIO, "prog_calls: internal: a long program did not fit its workspace");
		*total = need;
		SYZ_PC_ARGS(prog_calls_room(need, cap, sizing));
		if (!sizing && need)
			k_su_gather<uint32_t><<<grid_cap(nprog, 1u << 16), kSuThreads, 0, s>>>(stage2, roff, 1, 1, coff, nprog, d_call_id,
			                                                                       nullptr);
	}
	SYZ_HIP(hipGetLastError());
	// nothing can fail from here on but the device itself: the outputs are written
	SYZ_HIP(hipMemcpyAsync(d_call_off, coff, (nprog + 1) * 8, hipMemcpyDeviceToDevice, s));
	SYZ_HIP(hipMemcpyAsync(d_status, status, nprog, hipMemcpyDeviceToDevice, s));
	SYZ_HIP(hipMemcpyAsync(d_err_line, err_line, nprog * 4, hipMemcpyDeviceToDevice, s));
	SYZ_HIP(hipMemcpyAsync(d_flag, flag, nprog, hipMemcpyDeviceToDevice, s));
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

extern "C" int syzsig_prog_calls_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::pc_stats, out, "prog_calls_stats");
}
