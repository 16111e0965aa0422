// report.hip -- the corpus-wide loops behind the manager's coverage pages, on
// device: the numeric part of syz-manager/html.go and syz-manager/cover.go.
//
// References:
//   syz-manager/html.go:135-149   collectSyscallInfo: per call, count++ and
//                                 cov.Merge(inp.Cover) over the whole corpus
//   syz-manager/html.go:202-212   httpCover: the union of one input's, one
//                                 call's or every input's cover
//   syz-manager/html.go:319-331   httpRawCover: RestorePC, previousInstructionPC,
//                                 sort.Slice
//   syz-manager/cover.go:99-104   generateCoverHTML: the same map, unsorted
//   syz-manager/cover.go:254-304  uncoveredPcsInFuncs
//   syz-manager/cover.go:394-411  previousInstructionPC
//   pkg/cover/cover.go:28-30      RestorePC
//
// syzsig_call_cover_dev: a union of covers grouped by call is a segmented
// sort-unique once the PCs stand in call order:
//   k_rc_prep      offsets and call ids checked (nothing else runs when one is
//                  bad); per call the selected inputs and their PCs (histogram)
//   k_rc_seglens   the calls past a tile, their tiles and keys (segsort.h's plan)
//   k_su_scan      histogram -> the calls' ranges
//   k_rc_scatter   one wave per selected input: its PCs to its call's range (one
//                  atomic per input; the order inside a call is whatever the
//                  atomics give, the sort that follows does not depend on it)
//   su_sort_unique over ncalls segments with cover.hip's u32 tile, then
//   k_su_scan / k_su_gather: the calls' unions as CSR.
// The union over all selected inputs is the sort-unique of that CSR as one
// more segment (each PC at most once per call instead of once per input).
//
// syzsig_report_pcs_dev: the map is one kernel.  The sorted list keeps
// repeats, so its sort keys are (value, index) pairs -- two words, all
// distinct -- through the same sort-unique, and the output policy writes the
// first word.  It is not the map of a sorted input: with base == 0 a PC below
// the subtrahend wraps and sorts last, and arm's mask folds neighbours.
//
// syzsig_uncovered_pcs_dev.  The reference loop depends on the order of pcs in
// three ways; each is reproduced by an order-independent min / max:
//   1. the search is sort.Search over `pc < symbols[i].end`, whose ends are not
//      monotone when symbols nest: k_un_search runs the same probe sequence
//      (su_search halves as Go does), then the same start / end test;
//   2. handledFuncs is keyed by start, the range added uses the end of the
//      alias that the first PC's search found: per distinct start (equal
//      starts are contiguous; the slot is the start's lower bound) the minimum
//      of pos << 32 | idx;
//   3. a function's sites are added once, at the position of its first PC,
//      before that position's delete: k_un_add takes the max of pos + 1 into
//      add[site] over the handled functions whose range holds the site,
//      k_un_search the max of pos + 1 into del[site] over the accepted
//      occurrences of the site in pcs, and a site is in the result iff
//      add != 0 && add > del.
// A function's range is walked by the wave that owns its slot, or, past
// kReportWaveSites sites, by a workgroup (k_un_add_block) from a list.
//   k_un_count / k_su_scan / k_un_write   the survivors compacted in order.
//
// syzsig_file_set_dev: fileSet (cover.go:162-193) and the line walk's Coverage
// count (cover.go:129-148) over frames whose File and Func are dense ids.
//   k_fs_pass<covered>      funcs[Func] = true as one bit per function id, the
//                           ids checked, per file the frames (histogram)
//   k_fs_pass<uncovered>    the same for the frames whose function has its bit
//                           (a separate launch: every covered frame came first)
//   k_rc_seglens, k_su_scan segsort.h's plan; the files' ranges
//   k_fs_pass<.., scatter>  every counted frame's key to its file's range.  Frames
//                           of neighbouring PCs share a file: one atomic per run
//                           of equal neighbours in a wave (fs_run_add)
//   su_sort_unique          over nfiles segments with the plain one-word tile.
//                           Key = file_set_key: the line in signed order, then
//                           covered before uncovered.  The key type calls two
//                           keys equal when their lines are: what survives the
//                           sort-unique is each line's first key -- its covered
//                           entry if it has one -- so `true` is never overwritten
//                           and a line is listed once, without a pass of its own
//   k_su_scan               the lists' lengths -> the CSR offsets, the total
//                           (cap is checked against it; nothing is written before)
//   k_fs_emit / _block      per file, by a wave or (past kFileSetWaveEntries) a
//                           workgroup from a list: keys -> (line, covered), and
//                           the walk in closed form -- the head's sign, an upper
//                           bound of nlines, a sum over the flags before it.
#include <algorithm>

#include "cover_tile.h"
#include "report_args.h"

namespace syz {

constexpr uint32_t kRcThreads = 256;
constexpr uint32_t kRcPcsTile = 2048;  // (value, index) keys of report_pcs in LDS: 32 KB
constexpr uint32_t kUnChunk = 2048;    // sites per workgroup of the compaction
constexpr int kRcBadOff = kCntError, kRcBadCall = kCntInserted, kRcSelected = kSuTotal;
constexpr int kUnBadCover = kCntError, kUnBadSym = kCntInserted, kUnHandled = kCntAux, kUnLong = kCntAux2;
static_assert(kUnChunk % kRcThreads == 0, "whole sweeps per chunk");

using RcPcsTile = SuWordsTile<2, kRcPcsTile>;

// ---- per-call cover ----

__global__ __launch_bounds__(kRcThreads) void k_rc_prep(const uint64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ call,
                                                        const uint8_t* __restrict__ select, uint64_t ninputs,
                                                        uint64_t total, uint32_t ncalls, uint32_t* hist,
                                                        uint32_t* count, unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad_off = 0, bad_call = 0, sel = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ninputs; i += T) {
		const uint64_t a = off[i], b = off[i + 1];
		const uint32_t c = call[i];
		const bool bo = a > b || b > total || (i == 0 && a != 0) || (i == ninputs - 1 && b != total);
		bad_off += bo;
		bad_call += c >= ncalls;
		if (bo || c >= ncalls || (select && !select[i]))
			continue;
		atomicAdd(&count[c], 1u);
		if (b > a)
			atomicAdd(&hist[c], (uint32_t)(b - a));  // (total < 2^31)
		sel += b - a;
	}
	block_count(&cnt[kRcBadOff], bad_off);
	block_count(&cnt[kRcBadCall], bad_call);
	block_count(&cnt[kRcSelected], sel);
}

template <uint32_t kTile, uint32_t kAlign>
__global__ __launch_bounds__(kRcThreads) void k_rc_seglens(const uint32_t* __restrict__ len, uint64_t nseg,
                                                           unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t nl = 0, nt = 0, nk = 0;
	for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += T)
		su_count_large<kTile, kAlign>(len[s], nl, nt, nk, cnt);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
}

// one segment of *len_src keys (len_src == nullptr: len_val) from key 0 on: its length, its start, segsort.h's plan
template <uint32_t kTile, uint32_t kAlign>
__global__ void k_rc_one_seg(const uint64_t* __restrict__ len_src, uint64_t len_val, uint32_t* seg_len,
                             uint64_t* seg_start, unsigned long long* cnt)
{
	if (threadIdx.x || blockIdx.x)
		return;
	const uint32_t len = (uint32_t)(len_src ? *len_src : len_val);
	uint64_t nl = 0, nt = 0, nk = 0;
	*seg_len = len;
	*seg_start = 0;
	su_count_large<kTile, kAlign>(len, nl, nt, nk, cnt);
	cnt[kSuLarge] = nl;
	cnt[kSuTiles] = nt;
	cnt[kSuKeys] = nk;
}

// cur[c] starts at the first PC of call c
__global__ __launch_bounds__(kRcThreads) void k_rc_scatter(const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ cov,
                                                           const uint32_t* __restrict__ call,
                                                           const uint8_t* __restrict__ select, uint64_t ninputs,
                                                           uint32_t ncalls, uint64_t cap, unsigned long long* cur,
                                                           uint32_t* stage)
{
	const uint64_t W = (uint64_t)gridDim.x * (kRcThreads / 64);
	const uint32_t lane = lane_id();
	for (uint64_t i = (uint64_t)blockIdx.x * (kRcThreads / 64) + (threadIdx.x >> 6); i < ninputs; i += W) {
		const uint64_t a = off[i], b = off[i + 1];
		const uint32_t c = call[i];
		if (c >= ncalls || b <= a || (select && !select[i]))
			continue;  // (bad ones are ruled out by k_rc_prep)
		const uint64_t len = b - a;
		uint64_t at = 0;
		if (lane == 0)
			at = atomicAdd(&cur[c], (unsigned long long)len);
		at = __shfl(at, 0, 64);
		if (at + len > cap)
			continue;  // (the ranges are the histogram's: cannot happen)
		for (uint64_t x = lane; x < len; x += 64)
			stage[at + x] = cov[a + x];
	}
}

// ---- report PCs ----

__global__ __launch_bounds__(kRcThreads) void k_rp_map(const uint32_t* __restrict__ pcs, uint64_t n, uint32_t base,
                                                       ReportArch arch, uint64_t* out_order, uint64_t* keys)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
		const uint64_t v = report_prev_pc(arch, base, pcs[i]);
		out_order[i] = v;
		keys[2 * i] = v;
		keys[2 * i + 1] = i;
	}
}

// output policy: the first word of every surviving (value, index) key
struct RpOutValue {
	uint64_t* out;
	uint32_t* out_cnt;
	__device__ __forceinline__ uint64_t weight(uint64_t, const SuWords<2>&) const { return 1; }
	__device__ __forceinline__ void put(uint64_t, uint64_t pos, const SuWords<2>& k, uint64_t) const { out[pos] = k.w[0]; }
	__device__ __forceinline__ void finish(uint64_t seg, uint64_t total) const { out_cnt[seg] = (uint32_t)total; }
};

// ---- uncovered PCs ----

__global__ __launch_bounds__(kRcThreads) void k_un_check(const uint64_t* __restrict__ all, uint64_t nall,
                                                         const uint64_t* __restrict__ sym_start, uint64_t nsym,
                                                         unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t bad_cover = 0, bad_sym = 0;
	for (uint64_t i = t + 1; i < nall; i += T)
		bad_cover += all[i - 1] >= all[i];
	for (uint64_t i = t + 1; i < nsym; i += T)
		bad_sym += sym_start[i - 1] > sym_start[i];
	block_count(&cnt[kUnBadCover], bad_cover);
	block_count(&cnt[kUnBadSym], bad_sym);
}

// the first index of the ascending a[0 .. n) with a[i] >= x (kUpper: > x)
template <bool kUpper>
__device__ __forceinline__ uint64_t un_bound(const uint64_t* __restrict__ a, uint64_t n, uint64_t x)
{
	return su_search<uint64_t>(0, n, [&](uint64_t mid) { return kUpper ? a[mid] <= x : a[mid] < x; });
}

// cover.go:274-284 and :297 per position: the search, the acceptance, the
// function's first (position, alias), the site's last delete
__global__ __launch_bounds__(kRcThreads) void k_un_search(const uint64_t* __restrict__ pcs, uint64_t npc,
                                                          const uint64_t* __restrict__ sym_start,
                                                          const uint64_t* __restrict__ sym_end, uint64_t nsym,
                                                          const uint64_t* __restrict__ all, uint64_t nall,
                                                          unsigned long long* first, uint32_t* del)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npc; p += T) {
		const uint64_t pc = pcs[p];
		// sort.Search(len(symbols), func(i) { return pc < symbols[i].end }): h = (i + j) >> 1, !f(h) -> i = h + 1
		const uint64_t idx = su_search<uint64_t>(0, nsym, [&](uint64_t h) { return !(pc < sym_end[h]); });
		if (idx == nsym)
			continue;
		const uint64_t st = sym_start[idx];
		if (pc < st || pc > sym_end[idx])
			continue;
		atomicMin(&first[un_bound<false>(sym_start, nsym, st)], (unsigned long long)(p << 32 | idx));
		const uint64_t i = un_bound<false>(all, nall, pc);
		if (i < nall && all[i] == pc)
			atomicMax(&del[i], (uint32_t)p + 1);
	}
}

// the sites of the function handled at slot s: cover.go:287-292 with the first PC's alias
__device__ __forceinline__ bool un_range(const unsigned long long* __restrict__ first, uint64_t s,
                                         const uint64_t* __restrict__ sym_start, const uint64_t* __restrict__ sym_end,
                                         uint64_t nsym, const uint64_t* __restrict__ all, uint64_t nall, uint64_t& lo,
                                         uint64_t& hi, uint32_t& mark)
{
	const unsigned long long f = first[s];
	if (f == ~0ull)
		return false;
	const uint64_t idx = (uint32_t)f;
	if (idx >= nsym)
		return false;  // (an index k_un_search wrote: cannot happen)
	mark = (uint32_t)(f >> 32) + 1;
	lo = un_bound<false>(all, nall, sym_start[idx]);
	hi = std::max(lo, un_bound<true>(all, nall, sym_end[idx]));
	return true;
}

// one wave per slot
__global__ __launch_bounds__(kRcThreads) void k_un_add(const unsigned long long* __restrict__ first,
                                                       const uint64_t* __restrict__ sym_start,
                                                       const uint64_t* __restrict__ sym_end, uint64_t nsym,
                                                       const uint64_t* __restrict__ all, uint64_t nall, uint32_t* add,
                                                       uint32_t* longs, unsigned long long* cnt)
{
	const uint64_t W = (uint64_t)gridDim.x * (kRcThreads / 64);
	const uint32_t lane = lane_id();
	uint64_t handled = 0;
	for (uint64_t s = (uint64_t)blockIdx.x * (kRcThreads / 64) + (threadIdx.x >> 6); s < nsym; s += W) {
		uint64_t lo, hi;
		uint32_t mark;
		if (!un_range(first, s, sym_start, sym_end, nsym, all, nall, lo, hi, mark))
			continue;
		handled += lane == 0;
		if (report_block_path(hi - lo)) {
			if (lane == 0) {
				const uint64_t k = atomicAdd(&cnt[kUnLong], 1ull);
				if (k < nsym)
					longs[k] = (uint32_t)s;
			}
			continue;
		}
		for (uint64_t i = lo + lane; i < hi; i += 64)
			atomicMax(&add[i], mark);
	}
	block_count(&cnt[kUnHandled], handled);
}

// one workgroup per listed slot
__global__ __launch_bounds__(kRcThreads) void k_un_add_block(const unsigned long long* __restrict__ first,
                                                             const uint64_t* __restrict__ sym_start,
                                                             const uint64_t* __restrict__ sym_end, uint64_t nsym,
                                                             const uint64_t* __restrict__ all, uint64_t nall,
                                                             uint32_t* add, const uint32_t* __restrict__ longs,
                                                             const unsigned long long* cnt)
{
	const uint64_t n = std::min<uint64_t>(cnt[kUnLong], nsym);
	for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
		uint64_t lo, hi;
		uint32_t mark;
		if (!un_range(first, longs[k], sym_start, sym_end, nsym, all, nall, lo, hi, mark))
			continue;
		for (uint64_t i = lo + threadIdx.x; i < hi; i += kRcThreads)
			atomicMax(&add[i], mark);
	}
}

__device__ __forceinline__ bool un_keep(uint32_t add, uint32_t del) { return add != 0 && add > del; }

__global__ __launch_bounds__(kRcThreads) void k_un_count(const uint32_t* __restrict__ add,
                                                         const uint32_t* __restrict__ del, uint64_t nall,
                                                         uint32_t* blk)
{
	__shared__ uint32_t s_n;
	if (threadIdx.x == 0)
		s_n = 0;
	__syncthreads();
	const uint64_t b0 = (uint64_t)blockIdx.x * kUnChunk;
	uint32_t c = 0;
	for (uint32_t x = threadIdx.x; x < kUnChunk && b0 + x < nall; x += kRcThreads)
		c += un_keep(add[b0 + x], del[b0 + x]);
	if (c)
		atomicAdd(&s_n, c);
	__syncthreads();
	if (threadIdx.x == 0)
		blk[blockIdx.x] = s_n;
}

// the survivors of chunk blockIdx.x, in order, from blk_off[blockIdx.x] on
__global__ __launch_bounds__(kRcThreads) void k_un_write(const uint64_t* __restrict__ all,
                                                         const uint32_t* __restrict__ add,
                                                         const uint32_t* __restrict__ del, uint64_t nall,
                                                         const uint64_t* __restrict__ blk_off, uint64_t* out)
{
	__shared__ uint32_t s_w[2][kRcThreads / 64];
	const uint64_t b0 = (uint64_t)blockIdx.x * kUnChunk;
	const uint32_t w = threadIdx.x >> 6;
	uint64_t run = blk_off[blockIdx.x];
	uint32_t it = 0;
	for (uint32_t base = 0; base < kUnChunk; base += kRcThreads, it ^= 1) {
		const uint64_t i = b0 + base + threadIdx.x;
		const uint32_t f = i < nall && un_keep(add[i], del[i]);
		const uint32_t incl = wave_incl_scan(f);
		if (lane_id() == 63)
			s_w[it][w] = incl;
		__syncthreads();  // (s_w[it] is rewritten two sweeps on, past the next sweep's barrier)
		uint32_t wb = 0, tot = 0;
#pragma unroll
		for (uint32_t x = 0; x < kRcThreads / 64; x++) {
			wb += x < w ? s_w[it][x] : 0;
			tot += s_w[it][x];
		}
		if (f)
			out[run + wb + incl - 1] = all[i];
		run += tot;
	}
}

// ---- fileSet and the line walk ----

constexpr uint32_t kFsTile = SYZSIG_FILESET_TILE;
constexpr int kFsBadFile = kCntError, kFsBadFunc = kCntInserted, kFsKept = kSuTotal, kFsLong = kCntSpill;

// file_set_key as a sort key: ordered as the word it is, equal when the lines are
struct FsKey : SuU64<1> {
	static __device__ __forceinline__ bool eq(const T& a, const T& b) { return (a.w[0] >> 1) == (b.w[0] >> 1); }
};

// the plain one-word tile, its survivors chosen by FsKey::eq
struct FsTile : SuWordsTile<1, kFsTile> {
	using Key = FsKey;
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

struct FsFrames {
	const uint32_t* file;
	const int32_t* line;
	const uint32_t* func;
	uint64_t n;
};

// ctr[id] += 1 for every lane that is `on`, with one atomic per run of
// neighbouring lanes that are on and hold the same id; returns this lane's
// place: the count before its run plus its rank in the run.  The whole wave
// calls it.
__device__ __forceinline__ uint32_t fs_run_add(uint32_t* ctr, uint32_t id, bool on)
{
	const uint32_t lane = lane_id();
	const uint32_t key = on ? id : 0xffffffffu;  // (an id that is on is below 2^32 - 1)
	const uint32_t prev = __shfl_up(key, 1, 64);
	const bool head = on && (lane == 0 || prev != key);
	const uint64_t heads = __ballot(head), stops = heads | ~__ballot(on);
	// an on lane has a head at or below it: lane 0, or the first on lane after an off one
	const uint32_t hl = on ? 63 - (uint32_t)__clzll((long long)(heads & (~0ull >> (63 - lane)))) : lane;
	const uint64_t after = hl == 63 ? 0 : stops & (~0ull << (hl + 1));
	const uint32_t end = after ? (uint32_t)__ffsll((long long)after) - 1 : 64;
	uint32_t at = 0;
	if (head)
		at = atomicAdd(&ctr[id], end - lane);
	at = __shfl(at, hl, 64);
	return at + (lane - hl);
}

// One pass over one list of frames.  kCovered: cover.go:165-171, funcs[Func] =
// true as a bit; else cover.go:172-175, a frame whose function has no bit is
// skipped.  !kScatter: the ids checked, per_file = the files' histogram, the
// kept frames counted.  kScatter: per_file = the files' cursors (from 0), every
// frame the histogram counted puts its key into its file's range of `stage`.
template <bool kCovered, bool kScatter>
__global__ __launch_bounds__(kRcThreads) void k_fs_pass(FsFrames F, uint32_t nfiles, uint32_t nfuncs, uint32_t* funcs,
                                                        uint32_t* per_file, const uint64_t* __restrict__ seg_off,
                                                        uint64_t cap, uint64_t* stage, unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad_file = 0, bad_func = 0, kept = 0;
	for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < F.n; i0 += T) {  // (uniform per workgroup)
		const uint64_t i = i0 + threadIdx.x;
		uint32_t file = 0, func = 0;
		bool on = false;
		if (i < F.n) {
			file = F.file[i];
			func = F.func[i];
			bad_file += file >= nfiles;
			bad_func += func >= nfuncs;
			on = file < nfiles && func < nfuncs;
		}
		if (on && !(kCovered && kScatter)) {
			// neighbouring frames share a function: most lanes find the bit set and issue no atomic
			const uint32_t bit = 1u << (func & 31), have = __atomic_load_n(&funcs[func >> 5], __ATOMIC_RELAXED) & bit;
			if (!kCovered)
				on = have != 0;
			else if (!kScatter && !have)
				atomicOr(&funcs[func >> 5], bit);
		}
		kept += on;
		const uint32_t at = fs_run_add(per_file, file, on);
		if (kScatter && on) {
			const uint64_t p = seg_off[file] + at;
			if (p < cap)  // (the ranges are the histogram's: cannot fail)
				stage[p] = file_set_key(F.line[i], kCovered);
		}
	}
	if (!kScatter) {
		block_count(&cnt[kFsBadFile], bad_file);
		block_count(&cnt[kFsBadFunc], bad_func);
		if (!kCovered)
			block_count(&cnt[kFsKept], kept);
	}
}

// A file's sorted keys src[0 .. n) to entries dst .. of the outputs; this
// thread takes first, first + stride, ...  With `walk`, shown = the entries the
// walk of cover.go:131-143 consumes, and the return value is this thread's
// share of the covered ones among them.
__device__ __forceinline__ uint32_t fs_emit_file(const uint64_t* __restrict__ src, uint32_t n, uint64_t dst, bool walk,
                                                 uint32_t nlines, uint32_t first, uint32_t stride, int32_t* line,
                                                 uint8_t* covered, uint32_t& shown)
{
	shown = 0;
	if (walk && n && file_set_key_line(src[0]) >= 1)  // a head below line 1 is never consumed and blocks the rest
		shown = su_search<uint32_t>(
			0, n, [&](uint32_t mid) { return file_set_line_within(file_set_key_line(src[mid]), nlines); });
	uint32_t c = 0;
	for (uint32_t i = first; i < n; i += stride) {
		const uint64_t k = src[i];
		const bool cv = file_set_key_covered(k);
		line[dst + i] = file_set_key_line(k);
		covered[dst + i] = cv;
		c += cv && i < shown;
	}
	return c;
}

// one wave per file; the long ones listed for k_fs_emit_block
__global__ __launch_bounds__(kRcThreads) void k_fs_emit(const uint64_t* __restrict__ stage,
                                                        const uint64_t* __restrict__ seg_off,
                                                        const uint32_t* __restrict__ len,
                                                        const uint64_t* __restrict__ off, uint64_t nfiles,
                                                        const uint32_t* __restrict__ nlines, uint64_t* d_off,
                                                        int32_t* d_line, uint8_t* d_covered, uint32_t* d_shown,
                                                        uint32_t* d_coverage, uint32_t* longs, unsigned long long* cnt)
{
	const uint64_t W = (uint64_t)gridDim.x * (kRcThreads / 64);
	const uint32_t lane = lane_id();
	for (uint64_t f = (uint64_t)blockIdx.x * (kRcThreads / 64) + (threadIdx.x >> 6); f < nfiles; f += W) {
		const uint32_t n = len[f];
		if (lane == 0)
			d_off[f] = off[f];
		if (file_set_block_path(n)) {
			if (lane == 0) {
				const uint64_t k = atomicAdd(&cnt[kFsLong], 1ull);
				if (k < nfiles)
					longs[k] = (uint32_t)f;
			}
			continue;
		}
		uint32_t shown;
		const uint32_t c = (uint32_t)wave_sum_u64(fs_emit_file(stage + seg_off[f], n, off[f], nlines != nullptr,
		                                                       nlines ? nlines[f] : 0, lane, 64, d_line, d_covered, shown));
		if (nlines && lane == 0) {
			d_shown[f] = shown;
			d_coverage[f] = c;
		}
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
		d_off[nfiles] = off[nfiles];
}

// one workgroup per listed file
__global__ __launch_bounds__(kRcThreads) void k_fs_emit_block(const uint64_t* __restrict__ stage,
                                                              const uint64_t* __restrict__ seg_off,
                                                              const uint32_t* __restrict__ len,
                                                              const uint64_t* __restrict__ off, uint64_t nfiles,
                                                              const uint32_t* __restrict__ nlines, int32_t* d_line,
                                                              uint8_t* d_covered, uint32_t* d_shown, uint32_t* d_coverage,
                                                              const uint32_t* __restrict__ longs,
                                                              const unsigned long long* cnt)
{
	__shared__ uint32_t s_c[kRcThreads / 64];
	const uint64_t nl = std::min<uint64_t>(cnt[kFsLong], nfiles);
	for (uint64_t k = blockIdx.x; k < nl; k += gridDim.x) {
		const uint64_t f = longs[k];
		if (f >= nfiles)
			continue;  // (an index k_fs_emit wrote: cannot happen)
		uint32_t shown;
		const uint32_t c = (uint32_t)wave_sum_u64(fs_emit_file(stage + seg_off[f], len[f], off[f], nlines != nullptr,
		                                                       nlines ? nlines[f] : 0, threadIdx.x, kRcThreads, d_line,
		                                                       d_covered, shown));
		if (lane_id() == 0)
			s_c[threadIdx.x >> 6] = c;
		__syncthreads();
		if (nlines && threadIdx.x == 0) {
			uint32_t sum = 0;
			for (uint32_t x = 0; x < kRcThreads / 64; x++)
				sum += s_c[x];
			d_shown[f] = shown;
			d_coverage[f] = sum;
		}
		__syncthreads();  // s_c is rewritten for the next file
	}
}

static int report_fail(const ReportStatus& a) { return fail(a.code, a.msg); }

#define SYZ_RARGS(expr)                                                            \
	do {                                                                           \
		const syz::ReportStatus a__ = (expr);                                      \
		if (a__.code != SYZSIG_OK)                                                 \
			return syz::report_fail(a__);                                          \
	} while (0)

}  // namespace syz

using namespace syz;

extern "C" int syzsig_call_cover_dev(syzsig_ctx* ctx, const uint64_t* d_cov_off, const uint32_t* d_cov,
                                     uint64_t ninputs, uint64_t total, const uint32_t* d_call, const uint8_t* d_select,
                                     uint64_t ncalls, uint32_t* d_count, uint32_t* d_cover_len,
                                     uint64_t* d_call_cov_off, uint32_t* d_call_cov, uint64_t cover_cap,
                                     uint32_t* d_all_cov, uint64_t* n_all)
{
	SYZ_LOCK(ctx);
	SYZ_RARGS(call_cover_args(ctx, d_cov_off, d_cov, ninputs, total, d_call, ncalls, d_count, d_cover_len,
	                          d_call_cov_off, d_call_cov, cover_cap, d_all_cov, n_all));
	std::fill(ctx->rc_stats, ctx->rc_stats + 4, 0);
	const hipStream_t s = ctx->stream;
	const uint32_t nc = (uint32_t)ncalls;
	// hist, count, cnt [ncalls]; seg_off, cur, off [ncalls + 1]; the union's one segment: len, cnt, start
	char* m;
	const size_t a32 = align256(ncalls * 4), a64 = align256((ncalls + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsRcMeta, 3 * a32 + 3 * a64 + 3 * 256, (void**)&m));
	uint32_t *hist = (uint32_t*)m, *count = (uint32_t*)(m + a32), *cnt = (uint32_t*)(m + 2 * a32);
	uint64_t *seg_off = (uint64_t*)(m + 3 * a32), *cur = (uint64_t*)(m + 3 * a32 + a64),
	         *off = (uint64_t*)(m + 3 * a32 + 2 * a64);
	char* one = m + 3 * a32 + 3 * a64;
	uint32_t *one_len = (uint32_t*)one, *one_cnt = (uint32_t*)(one + 256);
	uint64_t* one_start = (uint64_t*)(one + 512);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	if (ncalls)
		SYZ_HIP(hipMemsetAsync(m, 0, 3 * a32, s));
	if (ninputs)
		k_rc_prep<<<grid_for(ninputs, kRcThreads), kRcThreads, 0, s>>>(d_cov_off, d_call, d_select, ninputs, total, nc,
		                                                              hist, count, ctx->d_cnt);
	k_rc_seglens<kCvTile, kCvAlign><<<grid_for(ncalls, kRcThreads), kRcThreads, 0, s>>>(hist, ncalls, ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(hist, ncalls, seg_off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	const unsigned long long* h = ctx->h_cnt;
	SYZ_RARGS(call_cover_corpus_status(h[kRcBadOff], h[kRcBadCall], h[kRcSelected], cover_cap));
	const uint64_t selected = h[kRcSelected], nlarge = h[kSuLarge], maxlen = h[kSuMaxLen];
	uint32_t *stage, *stage2;
	SYZ_TRY(ws_get(ctx, kWsRcStage, selected * 4 + 256, (void**)&stage));
	SYZ_TRY(ws_get(ctx, kWsRcStage2, selected * 4 + 256, (void**)&stage2));
	if (selected) {
		SYZ_HIP(hipMemcpyAsync(cur, seg_off, (ncalls + 1) * 8, hipMemcpyDeviceToDevice, s));
		k_rc_scatter<<<grid_for(ninputs, kRcThreads / 64, 1 << 16), kRcThreads, 0, s>>>(
			d_cov_off, d_cov, d_call, d_select, ninputs, nc, selected, (unsigned long long*)cur, stage);
	}
	if (ncalls) {
		const SuSegs S{stage, 1, seg_off, hist, 1, hist, ncalls};
		const CvOut pol{stage2, seg_off, 1, cnt};
		SYZ_TRY((su_sort_unique<CvTile<false>, CvOut>(ctx, S, pol)));
	}
	k_su_scan<<<1, kSuThreads, 0, s>>>(cnt, ncalls, off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "call_cover: internal: a long segment did not fit its workspace");
	// nothing can fail from here on but the device itself: the outputs are written
	k_su_gather<<<grid_cap(ncalls), kSuThreads, 0, s>>>((const uint32_t*)stage2, seg_off, 1, 1, off, ncalls, d_call_cov,
	                                                    d_call_cov_off);
	if (ncalls) {
		SYZ_HIP(hipMemcpyAsync(d_count, count, ncalls * 4, hipMemcpyDeviceToDevice, s));
		SYZ_HIP(hipMemcpyAsync(d_cover_len, cnt, ncalls * 4, hipMemcpyDeviceToDevice, s));
	}
	SYZ_HIP(hipGetLastError());
	if (d_all_cov) {
		SYZ_TRY(counters_reset(ctx));
		k_rc_one_seg<kCvTile, kCvAlign><<<1, 64, 0, s>>>(off + ncalls, 0, one_len, one_start, ctx->d_cnt);
		SYZ_HIP(hipGetLastError());
		SYZ_TRY(counters_fetch(ctx));
		const SuSegs S{d_call_cov, 1, one_start, one_len, 1, one_len, 1};
		const CvOut pol{d_all_cov, one_start, 1, one_cnt};
		SYZ_TRY((su_sort_unique<CvTile<false>, CvOut>(ctx, S, pol)));
		uint32_t nall = 0;
		SYZ_HIP(hipMemcpyAsync(&nall, one_cnt, 4, hipMemcpyDeviceToHost, s));
		SYZ_TRY(counters_fetch(ctx));
		if (ctx->h_cnt[kCntError])
			return fail(SYZSIG_EIO, "call_cover: internal: the whole union did not fit its workspace");
		*n_all = nall;
	}
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	ctx->rc_stats[0] = nlarge;
	ctx->rc_stats[1] = report_merge_passes(maxlen, kCvTile);
	return SYZSIG_OK;
}

extern "C" int syzsig_report_pcs_dev(syzsig_ctx* ctx, const uint32_t* d_pcs, uint64_t n, uint32_t base, uint32_t arch,
                                     uint64_t* d_out_order, uint64_t* d_out_sorted)
{
	SYZ_LOCK(ctx);
	SYZ_RARGS(report_pcs_args(ctx, d_pcs, n, arch, d_out_order, d_out_sorted));
	std::fill(ctx->rc_stats, ctx->rc_stats + 4, 0);
	if (n == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	char* m;
	uint64_t* keys;
	SYZ_TRY(ws_get(ctx, kWsRcMeta, 3 * 256, (void**)&m));
	SYZ_TRY(ws_get(ctx, kWsRcStage, n * 16 + 256, (void**)&keys));
	uint32_t *one_len = (uint32_t*)m, *one_cnt = (uint32_t*)(m + 256);
	uint64_t* one_start = (uint64_t*)(m + 512);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_rp_map<<<grid_for(n, kRcThreads), kRcThreads, 0, s>>>(d_pcs, n, base, report_arch(arch), d_out_order, keys);
	k_rc_one_seg<RcPcsTile::kTile, RcPcsTile::kAlign><<<1, 64, 0, s>>>(nullptr, n, one_len, one_start, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	const SuSegs S{keys, 2, one_start, one_len, 1, one_len, 1};
	const RpOutValue pol{d_out_sorted, one_cnt};
	SYZ_TRY((su_sort_unique<RcPcsTile, RpOutValue>(ctx, S, pol)));
	SYZ_TRY(su_time_end(ctx));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "report_pcs: internal: the keys did not fit their workspace");
	return SYZSIG_OK;
}

extern "C" int syzsig_uncovered_pcs_dev(syzsig_ctx* ctx, const uint64_t* d_sym_start, const uint64_t* d_sym_end,
                                        uint64_t nsym, const uint64_t* d_all_cover, uint64_t nall,
                                        const uint64_t* d_pcs, uint64_t npc, uint64_t* d_out, uint64_t* n_out)
{
	SYZ_LOCK(ctx);
	SYZ_RARGS(uncovered_args(ctx, d_sym_start, d_sym_end, nsym, d_all_cover, nall, d_pcs, npc, d_out, n_out));
	std::fill(ctx->rc_stats, ctx->rc_stats + 4, 0);
	if (nall == 0) {  // cover.go:268-270
		*n_out = 0;
		return SYZSIG_OK;
	}
	const hipStream_t s = ctx->stream;
	const uint64_t nblk = (nall + kUnChunk - 1) / kUnChunk;
	char *m, *w, *b;
	const size_t a_first = align256(nsym * 8 + 8), a_site = align256(nall * 4), a_blk = align256(nblk * 4);
	SYZ_TRY(ws_get(ctx, kWsRcMeta, a_first + align256(nsym * 4 + 4), (void**)&m));
	SYZ_TRY(ws_get(ctx, kWsRcStage, 2 * a_site, (void**)&w));
	SYZ_TRY(ws_get(ctx, kWsRcStage2, a_blk + align256((nblk + 1) * 8), (void**)&b));
	unsigned long long* first = (unsigned long long*)m;
	uint32_t *longs = (uint32_t*)(m + a_first), *add = (uint32_t*)w, *del = (uint32_t*)(w + a_site), *blk = (uint32_t*)b;
	uint64_t* blk_off = (uint64_t*)(b + a_blk);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_un_check<<<grid_for(std::max(nall, nsym), kRcThreads), kRcThreads, 0, s>>>(d_all_cover, nall, d_sym_start, nsym,
	                                                                            ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	SYZ_RARGS(uncovered_tables_status(ctx->h_cnt[kUnBadCover], ctx->h_cnt[kUnBadSym]));
	SYZ_HIP(hipMemsetAsync(first, 0xff, a_first, s));
	SYZ_HIP(hipMemsetAsync(w, 0, 2 * a_site, s));
	if (npc && nsym) {
		k_un_search<<<grid_for(npc, kRcThreads), kRcThreads, 0, s>>>(d_pcs, npc, d_sym_start, d_sym_end, nsym,
		                                                            d_all_cover, nall, first, del);
		k_un_add<<<grid_for(nsym, kRcThreads / 64, 1 << 16), kRcThreads, 0, s>>>(first, d_sym_start, d_sym_end, nsym,
		                                                                        d_all_cover, nall, add, longs,
		                                                                        ctx->d_cnt);
		k_un_add_block<<<grid_for(std::min(nsym, npc), 1, 1024), kRcThreads, 0, s>>>(first, d_sym_start, d_sym_end, nsym,
		                                                                           d_all_cover, nall, add, longs,
		                                                                           ctx->d_cnt);
	}
	k_un_count<<<(uint32_t)nblk, kRcThreads, 0, s>>>(add, del, nall, blk);
	k_su_scan<<<1, kSuThreads, 0, s>>>(blk, nblk, blk_off);
	k_un_write<<<(uint32_t)nblk, kRcThreads, 0, s>>>(d_all_cover, add, del, nall, blk_off, d_out);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, blk_off + nblk, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(su_time_end(ctx));
	SYZ_TRY(counters_fetch(ctx));
	*n_out = total;
	ctx->rc_stats[2] = ctx->h_cnt[kUnHandled];
	ctx->rc_stats[3] = ctx->h_cnt[kUnLong];
	return SYZSIG_OK;
}

extern "C" int syzsig_report_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::rc_stats, out, "report_stats");
}

extern "C" int syzsig_file_set_dev(syzsig_ctx* ctx, const uint32_t* d_cov_file, const int32_t* d_cov_line,
                                   const uint32_t* d_cov_func, uint64_t ncov, const uint32_t* d_unc_file,
                                   const int32_t* d_unc_line, const uint32_t* d_unc_func, uint64_t nunc, uint64_t nfiles,
                                   uint64_t nfuncs, const uint32_t* d_nlines, uint64_t* d_off, int32_t* d_line,
                                   uint8_t* d_covered, uint64_t cap, uint32_t* d_shown, uint32_t* d_coverage)
{
	SYZ_LOCK(ctx);
	SYZ_RARGS(file_set_args(ctx, d_cov_file, d_cov_line, d_cov_func, ncov, d_unc_file, d_unc_line, d_unc_func, nunc, nfiles,
	                        nfuncs, d_nlines, d_off, d_line, d_covered, cap, d_shown, d_coverage));
	std::fill(ctx->fs_stats, ctx->fs_stats + 4, 0);
	const hipStream_t s = ctx->stream;
	const uint32_t nf = (uint32_t)nfiles, nfn = (uint32_t)nfuncs;
	// hist, cur [nfiles], the funcs bitmap (zeroed); cnt, longs [nfiles]; seg_off, off [nfiles + 1]
	char* m;
	const size_t a32 = align256(nfiles * 4), abm = align256((nfuncs + 31) / 32 * 4), a64 = align256((nfiles + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsRcMeta, 4 * a32 + abm + 2 * a64, (void**)&m));
	uint32_t *hist = (uint32_t*)m, *cur = (uint32_t*)(m + a32), *funcs = (uint32_t*)(m + 2 * a32),
	         *cnt = (uint32_t*)(m + 2 * a32 + abm), *longs = (uint32_t*)(m + 3 * a32 + abm);
	uint64_t *seg_off = (uint64_t*)(m + 4 * a32 + abm), *off = (uint64_t*)(m + 4 * a32 + abm + a64);
	const FsFrames C{d_cov_file, d_cov_line, d_cov_func, ncov}, U{d_unc_file, d_unc_line, d_unc_func, nunc};
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	if (2 * a32 + abm)
		SYZ_HIP(hipMemsetAsync(m, 0, 2 * a32 + abm, s));
	if (ncov)
		k_fs_pass<true, false><<<grid_for(ncov, kRcThreads), kRcThreads, 0, s>>>(C, nf, nfn, funcs, hist, nullptr, 0,
		                                                                        nullptr, ctx->d_cnt);
	if (nunc)
		k_fs_pass<false, false><<<grid_for(nunc, kRcThreads), kRcThreads, 0, s>>>(U, nf, nfn, funcs, hist, nullptr, 0,
		                                                                         nullptr, ctx->d_cnt);
	k_rc_seglens<FsTile::kTile, FsTile::kAlign><<<grid_for(nfiles, kRcThreads), kRcThreads, 0, s>>>(hist, nfiles,
	                                                                                               ctx->d_cnt);
	k_su_scan<<<1, kSuThreads, 0, s>>>(hist, nfiles, seg_off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	const unsigned long long* h = ctx->h_cnt;
	SYZ_RARGS(file_set_frames_status(h[kFsBadFile], h[kFsBadFunc]));
	const uint64_t kept = h[kFsKept], nlarge = h[kSuLarge], maxlen = h[kSuMaxLen], nkeys = ncov + kept;
	uint64_t *stage, *stage2;
	SYZ_TRY(ws_get(ctx, kWsRcStage, nkeys * 8 + 256, (void**)&stage));
	SYZ_TRY(ws_get(ctx, kWsRcStage2, nkeys * 8 + 256, (void**)&stage2));
	if (ncov)
		k_fs_pass<true, true><<<grid_for(ncov, kRcThreads), kRcThreads, 0, s>>>(C, nf, nfn, funcs, cur, seg_off, nkeys,
		                                                                       stage, ctx->d_cnt);
	if (kept)
		k_fs_pass<false, true><<<grid_for(nunc, kRcThreads), kRcThreads, 0, s>>>(U, nf, nfn, funcs, cur, seg_off, nkeys,
		                                                                        stage, ctx->d_cnt);
	if (nfiles) {
		const SuSegs S{stage, 1, seg_off, hist, 1, hist, nfiles};
		const SuOutKeys<FsKey> pol{stage2, seg_off, 1, cnt};
		SYZ_TRY((su_sort_unique<FsTile, SuOutKeys<FsKey>>(ctx, S, pol)));
	}
	k_su_scan<<<1, kSuThreads, 0, s>>>(cnt, nfiles, off);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, off + nfiles, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "file_set: internal: a long file did not fit its workspace");
	SYZ_RARGS(file_set_cap_status(total, cap));
	// nothing can fail from here on but the device itself: the outputs are written
	k_fs_emit<<<grid_for(nfiles, kRcThreads / 64, 1 << 16), kRcThreads, 0, s>>>(
		stage2, seg_off, cnt, off, nfiles, d_nlines, d_off, d_line, d_covered, d_shown, d_coverage, longs, ctx->d_cnt);
	if (file_set_block_path(total))
		k_fs_emit_block<<<grid_for(total / (kFileSetWaveEntries + 1), 1, 1024), kRcThreads, 0, s>>>(
			stage2, seg_off, cnt, off, nfiles, d_nlines, d_line, d_covered, d_shown, d_coverage, longs, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	ctx->fs_stats[0] = kept;
	ctx->fs_stats[1] = nlarge;
	ctx->fs_stats[2] = report_merge_passes(maxlen, kFsTile);
	ctx->fs_stats[3] = total;
	return SYZSIG_OK;
}

extern "C" int syzsig_file_set_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::fs_stats, out, "file_set_stats");
}
