// report_driver.cc -- the host-compilable half of syzkaller_amd/csrc/report.hip
// on the CPU, built under ASan + UBSan by tests/test_report_ref_cpu.py: every
// branch of csrc/report_args.h -- the argument checks of syzsig_call_cover_dev,
// syzsig_report_pcs_dev and syzsig_uncovered_pcs_dev (EINVAL, ERANGE, the NULL
// forms), how the device-side checks' counters become a status,
// previousInstructionPC per arch with its wrap, the wave / workgroup threshold
// of a function's site range and the merge-pass count.
#include <cstdint>
#include <cstdio>

#include "../include/syzsig.h"
#include "../syzkaller_amd/csrc/report_args.h"

using namespace syz;

static int g_fail = 0;
#define CHECK(c)                                                    \
	do {                                                            \
		if (!(c)) {                                                 \
			printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
			g_fail++;                                               \
		}                                                           \
	} while (0)

static void run_call_cover()
{
	int ctx = 0;
	const uint64_t off[2] = {0, 1};
	const uint32_t cov[1] = {7}, call[1] = {0};
	uint32_t count[1], len[1], out[1], all[1];
	uint64_t out_off[2], n_all;
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, count, len, out_off, out, 1, all, &n_all).code == SYZSIG_OK);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, count, len, out_off, out, 1, nullptr, nullptr).code == SYZSIG_OK);
	// the empty corpus, with and without calls; an input with an empty cover; no room asked for
	CHECK(call_cover_args(&ctx, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, out_off, nullptr, 0, nullptr, nullptr)
	          .code == SYZSIG_OK);
	CHECK(call_cover_args(&ctx, nullptr, nullptr, 0, 0, nullptr, 1, count, len, out_off, nullptr, 0, nullptr, nullptr).code ==
	      SYZSIG_OK);
	CHECK(call_cover_args(&ctx, off, nullptr, 1, 0, call, 1, count, len, out_off, nullptr, 0, nullptr, nullptr).code ==
	      SYZSIG_OK);
	CHECK(call_cover_args(nullptr, off, cov, 1, 1, call, 1, count, len, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, nullptr, cov, 1, 1, call, 1, count, len, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, nullptr, 1, 1, call, 1, count, len, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, nullptr, 1, count, len, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, nullptr, len, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, count, nullptr, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, count, len, nullptr, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, count, len, out_off, nullptr, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, count, len, out_off, out, 1, all, nullptr).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1, count, len, out_off, out, 1, nullptr, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 0, 1, call, 1, count, len, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 0, count, len, out_off, out, 1, all, &n_all).code == SYZSIG_EINVAL);
	CHECK(call_cover_args(&ctx, off, cov, 1ull << 32, 1, call, 1, count, len, out_off, out, 1, all, &n_all).code ==
	      SYZSIG_ERANGE);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1, call, 1ull << 32, count, len, out_off, out, 1, all, &n_all).code ==
	      SYZSIG_ERANGE);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1ull << 31, call, 1, count, len, out_off, out, 1, all, &n_all).code ==
	      SYZSIG_ERANGE);
	CHECK(call_cover_args(&ctx, off, cov, 1, (1ull << 31) - 1, call, 1, count, len, out_off, out, 1, all, &n_all).code ==
	      SYZSIG_OK);
	CHECK(call_cover_args(&ctx, off, cov, 1, 1ull << 31, call, 1, count, len, out_off, out, 1, all, &n_all).msg != nullptr);
	// (bad offsets, bad call ids, the selected inputs' PCs, cover_cap)
	CHECK(call_cover_corpus_status(0, 0, 0, 0).code == SYZSIG_OK);
	CHECK(call_cover_corpus_status(0, 0, 10, 10).code == SYZSIG_OK);
	CHECK(call_cover_corpus_status(0, 0, 10, 9).code == SYZSIG_ERANGE);
	CHECK(call_cover_corpus_status(1, 0, 0, 0).code == SYZSIG_EINVAL);
	CHECK(call_cover_corpus_status(0, 1, 0, 0).code == SYZSIG_EINVAL);
	CHECK(call_cover_corpus_status(1, 1, 10, 0).code == SYZSIG_EINVAL);  // bad offsets make the total meaningless
	CHECK(call_cover_corpus_status(0, 1, 10, 0).code == SYZSIG_EINVAL);
	CHECK(call_cover_corpus_status(1, 0, 0, 0).msg && call_cover_corpus_status(0, 0, 1, 0).msg);
}

static void run_report_pcs()
{
	int ctx = 0;
	const uint32_t pcs[1] = {0};
	uint64_t a[1], b[1];
	const uint32_t archs[] = {SYZSIG_ARCH_AMD64, SYZSIG_ARCH_386, SYZSIG_ARCH_ARM64, SYZSIG_ARCH_ARM, SYZSIG_ARCH_PPC64LE};
	for (uint32_t arch : archs)
		CHECK(report_pcs_args(&ctx, pcs, 1, arch, a, b).code == SYZSIG_OK);
	CHECK(report_pcs_args(&ctx, nullptr, 0, SYZSIG_ARCH_AMD64, nullptr, nullptr).code == SYZSIG_OK);
	CHECK(report_pcs_args(nullptr, pcs, 1, SYZSIG_ARCH_AMD64, a, b).code == SYZSIG_EINVAL);
	CHECK(report_pcs_args(&ctx, pcs, 1, 5, a, b).code == SYZSIG_EINVAL);  // Go: panic("unknown arch")
	CHECK(report_pcs_args(&ctx, pcs, 0, 0xffffffffu, a, b).code == SYZSIG_EINVAL);
	CHECK(report_pcs_args(&ctx, nullptr, 1, SYZSIG_ARCH_AMD64, a, b).code == SYZSIG_EINVAL);
	CHECK(report_pcs_args(&ctx, pcs, 1, SYZSIG_ARCH_AMD64, nullptr, b).code == SYZSIG_EINVAL);
	CHECK(report_pcs_args(&ctx, pcs, 1, SYZSIG_ARCH_AMD64, a, nullptr).code == SYZSIG_EINVAL);
	CHECK(report_pcs_args(&ctx, pcs, 1ull << 31, SYZSIG_ARCH_AMD64, a, b).code == SYZSIG_ERANGE);
	CHECK(report_pcs_args(&ctx, pcs, (1ull << 31) - 1, SYZSIG_ARCH_AMD64, a, b).code == SYZSIG_OK);
	// previousInstructionPC at hand-computed PCs (tests/report_cases.py has the same values)
	const uint64_t H = 0xffffffff00000000ull;
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_AMD64), 0xffffffffu, 0x81000005u) == H + 0x81000000u);
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_386), 0xffffffffu, 0x81000005u) == H + 0x81000004u);
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_ARM64), 0xffffffffu, 0x81000005u) == H + 0x81000001u);
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_ARM), 0xffffffffu, 0x81000005u) == H + 0x81000002u);
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_PPC64LE), 0xffffffffu, 0x81000005u) == H + 0x81000001u);
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_ARM), 0, 0x1005) == 0x1002 &&
	      report_prev_pc(report_arch(SYZSIG_ARCH_ARM), 0, 0x1006) == 0x1002);  // the pair that collides
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_AMD64), 0, 3) == ~0ull - 1);   // the u64 wrap
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_ARM), 0, 2) == ~0ull - 1);
	CHECK(report_prev_pc(report_arch(SYZSIG_ARCH_AMD64), 0xffffffffu, 0xffffffffu) == ~0ull - 5);
	CHECK(!report_arch(5).known && !report_arch(0xffffffffu).known);
}

static void run_uncovered()
{
	int ctx = 0;
	const uint64_t s[1] = {10}, e[1] = {20}, all[1] = {12}, pcs[1] = {12};
	uint64_t out[1], n;
	CHECK(uncovered_args(&ctx, s, e, 1, all, 1, pcs, 1, out, &n).code == SYZSIG_OK);
	CHECK(uncovered_args(&ctx, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, &n).code == SYZSIG_OK);
	CHECK(uncovered_args(&ctx, s, e, 1, nullptr, 0, pcs, 1, nullptr, &n).code == SYZSIG_OK);  // cover.go:268: no sites
	CHECK(uncovered_args(nullptr, s, e, 1, all, 1, pcs, 1, out, &n).code == SYZSIG_EINVAL);
	CHECK(uncovered_args(&ctx, nullptr, e, 1, all, 1, pcs, 1, out, &n).code == SYZSIG_EINVAL);
	CHECK(uncovered_args(&ctx, s, nullptr, 1, all, 1, pcs, 1, out, &n).code == SYZSIG_EINVAL);
	CHECK(uncovered_args(&ctx, s, e, 1, nullptr, 1, pcs, 1, out, &n).code == SYZSIG_EINVAL);
	CHECK(uncovered_args(&ctx, s, e, 1, all, 1, nullptr, 1, out, &n).code == SYZSIG_EINVAL);
	CHECK(uncovered_args(&ctx, s, e, 1, all, 1, pcs, 1, nullptr, &n).code == SYZSIG_EINVAL);
	CHECK(uncovered_args(&ctx, s, e, 1, all, 1, pcs, 1, out, nullptr).code == SYZSIG_EINVAL);
	CHECK(uncovered_args(&ctx, s, e, 1, all, 1, pcs, 1ull << 32, out, &n).code == SYZSIG_ERANGE);
	CHECK(uncovered_args(&ctx, s, e, 1ull << 32, all, 1, pcs, 1, out, &n).code == SYZSIG_ERANGE);
	CHECK(uncovered_args(&ctx, s, e, 1, all, 1ull << 32, pcs, 1, out, &n).code == SYZSIG_ERANGE);
	CHECK(uncovered_args(&ctx, s, e, (1ull << 32) - 1, all, (1ull << 32) - 1, pcs, (1ull << 32) - 1, out, &n).code ==
	      SYZSIG_OK);
	CHECK(uncovered_tables_status(0, 0).code == SYZSIG_OK);
	CHECK(uncovered_tables_status(1, 0).code == SYZSIG_EINVAL);
	CHECK(uncovered_tables_status(0, 1).code == SYZSIG_EINVAL);
	CHECK(uncovered_tables_status(1, 1).msg && uncovered_tables_status(0, 1).msg);
	CHECK(!report_block_path(0) && !report_block_path(kReportWaveSites) && report_block_path(kReportWaveSites + 1));
	// merge passes over tiles of 4096: none up to a tile, one up to two tiles, two up to four
	CHECK(report_merge_passes(0, 4096) == 0 && report_merge_passes(4096, 4096) == 0);
	CHECK(report_merge_passes(4097, 4096) == 1 && report_merge_passes(8192, 4096) == 1);
	CHECK(report_merge_passes(8193, 4096) == 2 && report_merge_passes(8195, 4096) == 2);
	CHECK(report_merge_passes((1ull << 31) - 1, 4096) == 19);
}

int main()
{
	run_call_cover();
	run_report_pcs();
	run_uncovered();
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}
