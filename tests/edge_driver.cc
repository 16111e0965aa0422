// edge_driver.cc -- the host-compilable half of syzkaller_amd/csrc/edge.hip and
// cover.hip's trace entry point on the CPU, built under ASan + UBSan by
// tests/test_target_ref_cpu.py: every branch of csrc/edge_args.h -- the KCOV
// target word (every value 0..7 and a high bit), the NULL forms of
// syzsig_edge_derive_target_dev and syzsig_edge_cover_target_dev (what may be
// NULL when a count is 0), the cover flags, and the range predicates the
// kernels apply per program and per call (call_len < 262144, a range inside
// the trace, 64-bit sums that cannot wrap).
#include <cstdint>
#include <cstdio>

#include "../include/syzsig.h"
#include "../syzkaller_amd/csrc/edge_args.h"

using namespace syz;

static int g_fail = 0;
#define CHECK(c)                                                    \
	do {                                                            \
		if (!(c)) {                                                 \
			printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
			g_fail++;                                               \
		}                                                           \
	} while (0)

static void run_targets()
{
	// the reference has three executors: u64 unchecked, u32, u64 with the x86 range
	const bool valid[8] = {true, true, true, false, false, false, false, false};
	for (uint32_t t = 0; t < 8; t++)
		CHECK(edge_target_valid(t) == valid[t]);
	CHECK(!edge_target_valid(1u << 31) && !edge_target_valid(SYZSIG_TARGET_PC32 | 1u << 16) && !edge_target_valid(~0u));
	CHECK(SYZSIG_TARGET_LINUX_AMD64 == SYZSIG_TARGET_CHECK_X86 && edge_target_valid(SYZSIG_TARGET_LINUX_AMD64));
	CHECK(!edge_target_valid(SYZSIG_TARGET_PC32 | SYZSIG_TARGET_CHECK_X86));
}

static void run_derive_args()
{
	int ctx = 0;
	const uint64_t pcs[2] = {0, 0}, start[1] = {0};
	const uint32_t len[1] = {2}, prog[2] = {0, 1};
	uint32_t sigs[2], cnt[1], comp[1];
	for (uint32_t t = 0; t < 8; t++) {
		const EdgeStatus s = edge_derive_args(&ctx, pcs, 2, start, len, 1, prog, 1, t, sigs, cnt, comp);
		CHECK(s.code == (t <= 2 ? SYZSIG_OK : SYZSIG_EINVAL));
		CHECK((s.msg != nullptr) == (t > 2));
	}
	// every pointer in turn
	CHECK(edge_derive_args(nullptr, pcs, 2, start, len, 1, prog, 1, 0, sigs, cnt, comp).code == SYZSIG_EINVAL);
	CHECK(edge_derive_args(&ctx, nullptr, 2, start, len, 1, prog, 1, 0, sigs, cnt, comp).code == SYZSIG_EINVAL);
	CHECK(edge_derive_args(&ctx, pcs, 2, nullptr, len, 1, prog, 1, 0, sigs, cnt, comp).code == SYZSIG_EINVAL);
	CHECK(edge_derive_args(&ctx, pcs, 2, start, nullptr, 1, prog, 1, 0, sigs, cnt, comp).code == SYZSIG_EINVAL);
	CHECK(edge_derive_args(&ctx, pcs, 2, start, len, 1, nullptr, 1, 0, sigs, cnt, comp).code == SYZSIG_EINVAL);
	CHECK(edge_derive_args(&ctx, pcs, 2, start, len, 1, prog, 1, 0, nullptr, cnt, comp).code == SYZSIG_EINVAL);
	CHECK(edge_derive_args(&ctx, pcs, 2, start, len, 1, prog, 1, 0, sigs, nullptr, comp).code == SYZSIG_EINVAL);
	CHECK(edge_derive_args(&ctx, pcs, 2, start, len, 1, prog, 1, 0, sigs, cnt, nullptr).code == SYZSIG_EINVAL);
	// ... and what a zero count excuses: an empty trace, no calls, no programs
	CHECK(edge_derive_args(&ctx, nullptr, 0, start, len, 1, prog, 1, SYZSIG_TARGET_PC32, nullptr, cnt, comp).code ==
	      SYZSIG_OK);
	CHECK(edge_derive_args(&ctx, pcs, 2, nullptr, nullptr, 0, prog, 1, 0, sigs, nullptr, comp).code == SYZSIG_OK);
	CHECK(edge_derive_args(&ctx, pcs, 2, start, len, 1, nullptr, 0, 0, sigs, cnt, nullptr).code == SYZSIG_OK);
	CHECK(edge_derive_args(&ctx, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, SYZSIG_TARGET_CHECK_X86, nullptr, nullptr,
	                       nullptr)
	          .code == SYZSIG_OK);
	// a NULL argument is reported before the target, and a bad target with nothing to do is still rejected
	CHECK(edge_derive_args(nullptr, pcs, 2, start, len, 1, prog, 1, 3, sigs, cnt, comp).msg ==
	      edge_derive_args(nullptr, pcs, 2, start, len, 1, prog, 1, 0, sigs, cnt, comp).msg);
	CHECK(edge_derive_args(&ctx, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 4, nullptr, nullptr, nullptr).code ==
	      SYZSIG_EINVAL);
}

static void run_cover_args()
{
	int ctx = 0;
	const uint32_t pcs[2] = {0, 0};  // (a PC32 trace: the checks never look at the words)
	const uint64_t start[1] = {0};
	const uint32_t len[1] = {2}, prog[2] = {0, 1}, comp[1] = {1};
	uint32_t cover[2], cnt[1];
	for (uint32_t t = 0; t < 8; t++)
		for (uint32_t f = 0; f < 4; f++) {
			const EdgeStatus s = edge_cover_args(&ctx, pcs, 2, start, len, 1, prog, 1, comp, f, t, cover, cnt);
			CHECK(s.code == (t <= 2 && f <= SYZSIG_COVER_DEDUP ? SYZSIG_OK : SYZSIG_EINVAL));
			CHECK((s.msg != nullptr) == (s.code != SYZSIG_OK));
		}
	CHECK(edge_cover_args(&ctx, pcs, 2, start, len, 1, prog, 1, comp, 1u << 31, 0, cover, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(nullptr, pcs, 2, start, len, 1, prog, 1, comp, 0, 0, cover, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, nullptr, 2, start, len, 1, prog, 1, comp, 0, 0, cover, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, pcs, 2, nullptr, len, 1, prog, 1, comp, 0, 0, cover, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, pcs, 2, start, nullptr, 1, prog, 1, comp, 0, 0, cover, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, pcs, 2, start, len, 1, nullptr, 1, comp, 0, 0, cover, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, pcs, 2, start, len, 1, prog, 1, nullptr, 0, 0, cover, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, pcs, 2, start, len, 1, prog, 1, comp, 0, 0, nullptr, cnt).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, pcs, 2, start, len, 1, prog, 1, comp, 0, 0, cover, nullptr).code == SYZSIG_EINVAL);
	CHECK(edge_cover_args(&ctx, nullptr, 0, start, len, 1, prog, 1, comp, 1, 1, nullptr, cnt).code == SYZSIG_OK);
	CHECK(edge_cover_args(&ctx, pcs, 2, nullptr, nullptr, 0, prog, 1, comp, 1, 0, cover, nullptr).code == SYZSIG_OK);
	CHECK(edge_cover_args(&ctx, pcs, 2, start, len, 1, nullptr, 0, nullptr, 1, 2, cover, cnt).code == SYZSIG_OK);
}

static void run_ranges()
{
	// a program's calls [cb, ce) of ncalls
	CHECK(!edge_prog_bad(0, 0, 0) && !edge_prog_bad(0, 5, 5) && !edge_prog_bad(5, 5, 5));
	CHECK(edge_prog_bad(2, 1, 5) && edge_prog_bad(0, 6, 5) && edge_prog_bad(6, 6, 5));
	CHECK(!edge_prog_bad(0, 0xffffffffull, 0xffffffffull) && edge_prog_bad(0, 0xffffffffull, 0xfffffffeull));
	// a call's PCs [start, start + len) of npc: executor_linux.cc:186-187 n >= kCoverSize
	CHECK(kCoverSize == 262144);
	CHECK(!edge_call_bad(0, 262143, 262143) && edge_call_bad(0, 262144, 262144) && edge_call_bad(0, 262144, 1ull << 40));
	CHECK(edge_call_bad(0, 0xffffffffu, 1ull << 40));
	CHECK(!edge_call_bad(0, 0, 0) && !edge_call_bad(7, 0, 7) && edge_call_bad(8, 0, 7));
	CHECK(!edge_call_bad(3, 4, 7) && edge_call_bad(3, 5, 7) && edge_call_bad(4, 4, 7));
	// no wrap: a start near 2^64 with a short length, an npc near 2^64
	CHECK(edge_call_bad(~0ull, 1, 100) && edge_call_bad(~0ull - 1, 2, ~0ull - 1) && !edge_call_bad(~0ull - 2, 2, ~0ull));
	CHECK(edge_call_bad(~0ull, 1, ~0ull) && !edge_call_bad(~0ull, 0, ~0ull));
}

int main()
{
	run_targets();
	run_derive_args();
	run_cover_args();
	run_ranges();
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}
