// edge_args.h -- the host-side argument checks of edge.hip's and cover.hip's
// trace entry points (syzsig_edge_derive_target_dev, syzsig_edge_cover_target_dev
// and the two callers that fix the target): the KCOV target word, the NULL
// forms, the cover flags, and the per-program / per-call range predicates the
// kernels apply to the layout arrays (device memory, so the kernels call them).
// No HIP here, so that tests/edge_driver.cc runs every branch on the CPU under
// ASan + UBSan.  Whoever includes this has syzsig.h's codes and flags.
#pragma once

#include <cstdint>

#include "common.h"

namespace syz {

struct EdgeStatus {
	int code;  // SYZSIG_OK: go on
	const char* msg;
};

inline EdgeStatus edge_ok() { return EdgeStatus{SYZSIG_OK, nullptr}; }

// The three instantiations the reference has (executor.h:595-598 picks cover_t,
// the executor's own cover_check(cover_t) comes with it): u64 unchecked, u32
// (cover_check(uint32) is `return true` everywhere), u64 with the x86 range.
inline bool edge_target_valid(uint32_t target)
{
	return target == 0 || target == SYZSIG_TARGET_PC32 || target == SYZSIG_TARGET_CHECK_X86;
}

// a program's call range [cb, ce) of prog_call (u32 entries widened)
SYZ_HD bool edge_prog_bad(uint64_t cb, uint64_t ce, uint64_t ncalls) { return cb > ce || ce > ncalls; }

// a call's PCs [start, start + len) of a trace of npc PCs:
// executor_linux.cc:186-187 fail("too much cover") / malformed input
SYZ_HD bool edge_call_bad(uint64_t start, uint32_t len, uint64_t npc)
{
	return len >= kCoverSize || start > npc || len > npc - start;
}

// what both entry points take alike: the trace, its layout, the target
inline EdgeStatus edge_trace_args(const void* ctx, const void* d_pcs, uint64_t npc, const uint64_t* d_call_start,
                                  const uint32_t* d_call_len, uint64_t ncalls, const uint32_t* d_prog_call,
                                  uint64_t nprog, const uint32_t* d_completed, const uint32_t* d_out,
                                  const uint32_t* d_out_cnt, uint32_t target, const char* who_null,
                                  const char* who_target)
{
	if (!ctx || (nprog && (!d_prog_call || !d_completed)) || (ncalls && (!d_call_start || !d_call_len || !d_out_cnt)) ||
	    (npc && (!d_pcs || !d_out)))
		return EdgeStatus{SYZSIG_EINVAL, who_null};
	if (!edge_target_valid(target))
		return EdgeStatus{SYZSIG_EINVAL, who_target};
	return edge_ok();
}

inline EdgeStatus edge_derive_args(const void* ctx, const void* d_pcs, uint64_t npc, const uint64_t* d_call_start,
                                   const uint32_t* d_call_len, uint64_t ncalls, const uint32_t* d_prog_call,
                                   uint64_t nprog, uint32_t target, const uint32_t* d_sigs, const uint32_t* d_sig_cnt,
                                   const uint32_t* d_completed)
{
	return edge_trace_args(ctx, d_pcs, npc, d_call_start, d_call_len, ncalls, d_prog_call, nprog, d_completed, d_sigs,
	                       d_sig_cnt, target, "edge_derive: NULL argument",
	                       "edge_derive: target is not 0, SYZSIG_TARGET_PC32 or SYZSIG_TARGET_CHECK_X86");
}

inline EdgeStatus edge_cover_args(const void* ctx, const void* d_pcs, uint64_t npc, const uint64_t* d_call_start,
                                  const uint32_t* d_call_len, uint64_t ncalls, const uint32_t* d_prog_call,
                                  uint64_t nprog, const uint32_t* d_completed, uint32_t flags, uint32_t target,
                                  const uint32_t* d_cover, const uint32_t* d_cover_cnt)
{
	const EdgeStatus s = edge_trace_args(ctx, d_pcs, npc, d_call_start, d_call_len, ncalls, d_prog_call, nprog,
	                                     d_completed, d_cover, d_cover_cnt, target, "edge_cover: NULL argument",
	                                     "edge_cover: target is not 0, SYZSIG_TARGET_PC32 or SYZSIG_TARGET_CHECK_X86");
	if (s.code != SYZSIG_OK)
		return s;
	if (flags & ~(uint32_t)SYZSIG_COVER_DEDUP)
		return EdgeStatus{SYZSIG_EINVAL, "edge_cover: unknown flag"};
	return edge_ok();
}

}  // namespace syz
