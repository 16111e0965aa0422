// cover.hip -- the executor's cover output and triageInput's inputCover, on
// device: a segmented sort-unique of u32 keys.
//
// References:
//   executor/executor.h:514-527   write_coverage_signal's second half: with
//       flag_collect_cover the call's PCs go out as u32, after std::sort +
//       std::unique over the u64 PCs with flag_dedup_cover
//       (syzsig_edge_cover_dev);
//   syz-fuzzer/proc.go:139, :173  inputCover.Merge(inf.Cover) over the re-runs
//       and Cover: inputCover.Serialize() (syzsig_triage_cover_dev).
// Both are the same operation per segment (a call's trace; the concatenated
// cover lists of an item's merged runs): sort ascending, drop equal
// neighbours, write the survivors densely and their count.
//
// The keys, per KCOV target (syzsig.h SYZSIG_TARGET_*; std::sort + std::unique
// run on cover_t, the truncation of executor.h:525-526 comes after):
//   SYZSIG_TARGET_CHECK_X86 -- the low words of the u64 PCs.  Exactness of
//     sorting the low words holds for this target and for it alone: every PC of
//     a completed call passed cover_check (executor_linux.cc:196-204), so it
//     lies in [0xffffffff80000000, 0xffffffffff000000): its upper word is
//     0xffffffff.  u64 order and equality of such PCs are those of their low
//     words, so sort + unique on the low words, which is what leaves here, is
//     the reference's sort + unique on u64 followed by the truncation.
//   SYZSIG_TARGET_PC32 -- the u32 PCs themselves (cover_t = uint32): the same
//     u32 sort, loaded 4 B per key.
//   0 (u64, no check) -- the full u64 PCs.  Upper words differ, so two PCs
//     with one low word both survive and the output follows the u64 order:
//     0x100000009, 0x200000003 leave as 9, 3.  Sorted as u64 keys (CvTile64:
//     segsort.h's plain one-word tile), the survivors truncated on the way out
//     (CvOutLow).
// A call that did not complete (the one holding the PC that failed
// cover_check, and every later call of its program) never reaches this: its
// segment length is forced to 0 from `completed` before any key is read
// (k_cover_prep_calls), as doexit(0) happens inside the signal loop before any
// cover is written.
//
// The segmented sort-unique is segsort.h's, over u32 keys with the tile
// routines of cover_tile.h (shared with report.hip; T = kCvTile keys,
// SYZSIG_COVER_TILE; 4 T bytes of LDS, 16 KB at T = 4096: several workgroups
// share a CU): 16-B global loads on a source's aligned body (cv_load), the
// quad sort described below (cv_sort), a quad per
// thread in the unique sweep (cv_unique_write), and key ranges of whole quads
// in the sort buffers, so that the tile stores and the sweep's loads are 16 B.
//   k_cover_prep_calls / _items   validate; per segment its length (and per
//                                 run of an item its merged length); count the
//                                 segments longer than T, their tiles and keys
//
// The LDS sort.  The compare-exchanges of strides 2 and 1 of every stage run
// in registers on the thread's own 16-B quad (no barrier between them, and
// the stages of size 2 and 4 need no LDS step at all); the strides >= 4 pair
// two aligned quads, read and written as 16-B LDS accesses.  At quad strides
// 1..8 the ds_read_b128 lane groups see a 2-way bank conflict (two rows of
// 256 B per 16 lanes), larger strides are conflict-free; the 16-B stores are
// bound by their register transfer, not by the array.
#include <algorithm>

#include "cover_tile.h"
#include "edge_args.h"

namespace syz {

// executor.h:514-527 per call: seg_len[c] = call_len[c] for a call with a
// cover record (c - prog_call[p] < completed[p]), else 0.  Validates every
// call of every program as syzsig_edge_derive_dev does.
__global__ __launch_bounds__(64) void k_cover_prep_calls(const uint64_t* __restrict__ call_start,
                                                         const uint32_t* __restrict__ call_len, uint64_t ncalls,
                                                         uint64_t npc, const uint32_t* __restrict__ prog_call,
                                                         uint64_t nprog, const uint32_t* __restrict__ completed,
                                                         uint32_t* seg_len, unsigned long long* cnt)
{
	uint64_t err = 0, nl = 0, nt = 0, nk = 0;
	for (uint64_t p = blockIdx.x; p < nprog; p += gridDim.x) {
		const uint64_t cb = prog_call[p], ce = prog_call[p + 1];
		if (edge_prog_bad(cb, ce, ncalls) || completed[p] > ce - cb) {
			err += threadIdx.x == 0;
			continue;
		}
		const uint64_t done = completed[p];
		for (uint64_t c = cb + threadIdx.x; c < ce; c += blockDim.x) {
			const uint64_t start = call_start[c];
			const uint32_t len = call_len[c];
			if (edge_call_bad(start, len, npc)) {
				err++;  // executor_linux.cc:186-187 fail("too much cover") / malformed input
				continue;
			}
			const uint32_t eff = c - cb < done ? len : 0;
			seg_len[c] = eff;
			su_count_large<kCvTile, kCvAlign>(eff, nl, nt, nk, cnt);
		}
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
}

// proc.go:119-139 per item: run r of a kept item is merged (:139) unless the
// loop skipped it (:122-123: not executed, no signal, or failed after a
// successful original); a dropped item took a `return` before :173.
__global__ __launch_bounds__(256) void k_cover_prep_items(
	uint64_t nitems, uint32_t R, const uint8_t* __restrict__ item_flags, const uint8_t* __restrict__ item_keep,
	const uint64_t* __restrict__ run_off, const int32_t* __restrict__ run_errno, const uint8_t* __restrict__ run_exec,
	uint64_t ncover, const uint64_t* __restrict__ run_cover_start, const uint32_t* __restrict__ run_cover_len,
	uint32_t* src_len, uint32_t* seg_len, unsigned long long* cnt)
{
	uint64_t err = 0, ovf = 0, nl = 0, nt = 0, nk = 0, tot = 0;
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < nitems) {
		const bool keep = item_keep[i] != 0, orig_ok = item_flags[i] & SYZSIG_TRIAGE_ORIG_OK;
		uint64_t total = 0;
		for (uint32_t r = 0; r < R; r++) {
			const uint64_t rr = i * R + r, s = run_cover_start[rr];
			const uint32_t l = run_cover_len[rr];
			if (s > ncover || l > ncover - s) {
				err++;
				src_len[rr] = 0;
				continue;
			}
			const bool merged = keep && run_exec[rr] && run_off[rr + 1] > run_off[rr] && !(orig_ok && run_errno[rr] != 0);
			src_len[rr] = merged ? l : 0;
			total += merged ? l : 0;
		}
		if (total > kCvMaxSeg) {
			ovf++;
			total = 0;
		}
		seg_len[i] = (uint32_t)total;
		tot = total;
		su_count_large<kCvTile, kCvAlign>((uint32_t)total, nl, nt, nk, cnt);
	}
	block_count(&cnt[kCntError], err);
	block_count(&cnt[kCntOverflow], ovf);
	block_count(&cnt[kSuLarge], nl);
	block_count(&cnt[kSuTiles], nt);
	block_count(&cnt[kSuKeys], nk);
	block_count(&cnt[kSuTotal], tot);
}

// executor.h:525-527 without flag_dedup_cover: the PCs truncated, in trace order
// (PC = cover_t; a copy for u32 PCs)
template <typename PC>
__global__ __launch_bounds__(kCvThreads) void k_cover_trunc(const PC* __restrict__ pcs, SuSegs S, CvOut pol)
{
	for (uint64_t seg = blockIdx.x; seg < S.nseg; seg += gridDim.x) {
		const uint32_t n = S.seg_len[seg];
		const uint64_t g = S.src_start[seg];
		uint32_t* o = pol.dst(seg);
		for (uint32_t i = threadIdx.x; i < n; i += kCvThreads)
			o[i] = (uint32_t)pcs[g + i];
		if (threadIdx.x == 0)
			pol.finish(seg, n);
	}
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_edge_cover_target_dev(syzsig_ctx* ctx, const void* d_pcs, uint64_t npc,
                                            const uint64_t* d_call_start, const uint32_t* d_call_len, uint64_t ncalls,
                                            const uint32_t* d_prog_call, uint64_t nprog, const uint32_t* d_completed,
                                            uint32_t flags, uint32_t target, uint32_t* d_cover, uint32_t* d_cover_cnt)
{
	SYZ_LOCK(ctx);
	const EdgeStatus a = edge_cover_args(ctx, d_pcs, npc, d_call_start, d_call_len, ncalls, d_prog_call, nprog,
	                                     d_completed, flags, target, d_cover, d_cover_cnt);
	if (a.code != SYZSIG_OK)
		return fail(a.code, a.msg);
	if (ncalls == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	void* seg_len;
	SYZ_TRY(ws_get(ctx, kWsSuMeta, ncalls * 4 + 256, &seg_len));
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	// a call outside every program has no record
	SYZ_HIP(hipMemsetAsync(seg_len, 0, ncalls * 4, s));
	if (nprog)
		k_cover_prep_calls<<<grid_cap(nprog), 64, 0, s>>>(d_call_start, d_call_len, ncalls, npc, d_prog_call, nprog,
		                                                  d_completed, (uint32_t*)seg_len, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "edge_cover: malformed program/call ranges, completed past a program's calls, or "
		                           "a call with >= 262144 PCs");
	const SuSegs S{d_pcs, 1, d_call_start, (const uint32_t*)seg_len, 1, (const uint32_t*)seg_len, ncalls};
	const CvOut pol{d_cover, d_call_start, 1, d_cover_cnt};
	const bool pc32 = target & SYZSIG_TARGET_PC32;
	if (flags & SYZSIG_COVER_DEDUP) {
		// (the keys per target: header of this file)
		if (pc32)
			SYZ_TRY((su_sort_unique<CvTile<false>, CvOut>(ctx, S, pol)));
		else if (target & SYZSIG_TARGET_CHECK_X86)
			SYZ_TRY((su_sort_unique<CvTile<true>, CvOut>(ctx, S, pol)));
		else
			SYZ_TRY((su_sort_unique<CvTile64, CvOutLow>(ctx, S, CvOutLow{d_cover, d_call_start, 1, d_cover_cnt})));
	} else {
		if (pc32)
			k_cover_trunc<<<grid_cap(ncalls), kCvThreads, 0, s>>>(static_cast<const uint32_t*>(d_pcs), S, pol);
		else
			k_cover_trunc<<<grid_cap(ncalls), kCvThreads, 0, s>>>(static_cast<const uint64_t*>(d_pcs), S, pol);
		SYZ_HIP(hipGetLastError());
	}
	SYZ_TRY(su_time_end(ctx));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "edge_cover: internal: a long segment did not fit its workspace");
	return SYZSIG_OK;
}

extern "C" int syzsig_edge_cover_dev(syzsig_ctx* ctx, const uint64_t* d_pcs, uint64_t npc,
                                     const uint64_t* d_call_start, const uint32_t* d_call_len, uint64_t ncalls,
                                     const uint32_t* d_prog_call, uint64_t nprog, const uint32_t* d_completed,
                                     uint32_t flags, uint32_t* d_cover, uint32_t* d_cover_cnt)
{
	return syzsig_edge_cover_target_dev(ctx, d_pcs, npc, d_call_start, d_call_len, ncalls, d_prog_call, nprog,
	                                    d_completed, flags, SYZSIG_TARGET_LINUX_AMD64, d_cover, d_cover_cnt);
}

extern "C" int syzsig_triage_cover_dev(syzsig_ctx* ctx, uint64_t nitems, uint32_t runs, const uint8_t* d_item_flags,
                                       const uint8_t* d_item_keep, const uint64_t* d_run_off,
                                       const int32_t* d_run_errno, const uint8_t* d_run_exec,
                                       const uint32_t* d_cover, uint64_t ncover, const uint64_t* d_run_cover_start,
                                       const uint32_t* d_run_cover_len, uint64_t* d_item_cover_off,
                                       uint32_t* d_item_cover, uint64_t cap, uint64_t* n_out)
{
	SYZ_LOCK(ctx);
	if (n_out)
		*n_out = 0;
	if (!ctx || !d_item_cover_off || !n_out || (nitems && (!d_item_flags || !d_item_keep)) ||
	    (nitems && runs && (!d_run_off || !d_run_errno || !d_run_exec || !d_run_cover_start || !d_run_cover_len)) ||
	    (ncover && !d_cover) || (cap && !d_item_cover))
		return fail(SYZSIG_EINVAL, "triage_cover: NULL argument");
	if (runs > kCvMaxRuns)
		return fail(SYZSIG_ERANGE, "triage_cover: at most 8 runs per item");
	const hipStream_t s = ctx->stream;
	if (nitems == 0 || runs == 0) {
		SYZ_HIP(hipMemsetAsync(d_item_cover_off, 0, (nitems + 1) * 8, s));
		SYZ_HIP(hipStreamSynchronize(s));
		return SYZSIG_OK;
	}
	const uint64_t nruns = nitems * runs;
	// src_len[nruns], seg_len[nitems], cnt[nitems], stage_off[nitems + 1], off[nitems + 1]
	char* d;
	const size_t o_seg = align256(nruns * 4), o_cnt = o_seg + align256(nitems * 4), o_soff = o_cnt + align256(nitems * 4),
	             o_off = o_soff + align256((nitems + 1) * 8);
	SYZ_TRY(ws_get(ctx, kWsSuMeta, o_off + align256((nitems + 1) * 8), (void**)&d));
	uint32_t *src_len = (uint32_t*)d, *seg_len = (uint32_t*)(d + o_seg), *cnt = (uint32_t*)(d + o_cnt);
	uint64_t *stage_off = (uint64_t*)(d + o_soff), *off = (uint64_t*)(d + o_off);
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_cover_prep_items<<<(int)((nitems + 255) / 256), 256, 0, s>>>(nitems, runs, d_item_flags, d_item_keep, d_run_off,
	                                                               d_run_errno, d_run_exec, ncover, d_run_cover_start,
	                                                               d_run_cover_len, src_len, seg_len, ctx->d_cnt);
	k_su_scan<<<1, kCvThreads, 0, s>>>(seg_len, nitems, stage_off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EINVAL, "triage_cover: a run's cover range lies outside the cover buffer");
	if (ctx->h_cnt[kCntOverflow])
		return fail(SYZSIG_ERANGE, "triage_cover: an item's runs hold 2^31 or more PCs");
	void* stage;
	SYZ_TRY(ws_get(ctx, kWsSuStage, ctx->h_cnt[kSuTotal] * 4 + 256, &stage));
	const SuSegs S{d_cover, 1, d_run_cover_start, src_len, runs, seg_len, nitems};
	const CvOut pol{(uint32_t*)stage, stage_off, 1, cnt};
	SYZ_TRY((su_sort_unique<CvTile<false>, CvOut>(ctx, S, pol)));
	k_su_scan<<<1, kCvThreads, 0, s>>>(cnt, nitems, off);
	SYZ_HIP(hipGetLastError());
	uint64_t total = 0;
	SYZ_HIP(hipMemcpyAsync(&total, off + nitems, 8, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntError])
		return fail(SYZSIG_EIO, "triage_cover: internal: a long segment did not fit its workspace");
	*n_out = total;
	if (total > cap)
		return fail(SYZSIG_ERANGE, "triage_cover: the items' cover needs more than the given capacity");
	k_su_gather<<<grid_cap(nitems), kCvThreads, 0, s>>>((const uint32_t*)stage, stage_off, 1, 1, off, nitems, d_item_cover,
	                                                    d_item_cover_off);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}
