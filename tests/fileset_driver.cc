// fileset_driver.cc -- the host-compilable half of syzsig_file_set_dev
// (syzkaller_amd/csrc/report.hip) on the CPU, built under ASan + UBSan by
// tests/test_fileset_ref_cpu.py: every branch of its checks in
// csrc/report_args.h -- the argument checks (EINVAL, ERANGE, the NULL forms, the
// all-or-none rule of the walk's arrays), how the device-side counters become a
// status, the sort key's signed order and covered-before-uncovered rule, the
// 64-bit line / nlines compare and the wave / workgroup threshold.
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

static void run_args()
{
	int ctx = 0;
	const uint32_t cf[1] = {0}, cfn[1] = {0}, uf[1] = {0}, ufn[1] = {0}, nl[1] = {3};
	const int32_t cl[1] = {1}, ul[1] = {2};
	uint64_t off[2];
	int32_t line[2];
	uint8_t cov[2];
	uint32_t shown[1], coverage[1];
	const uint64_t M31 = 1ull << 31, M32 = 1ull << 32;
#define ARGS(...) file_set_args(__VA_ARGS__).code
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_OK);
	// the lists only; one list empty; no frames at all, with and without files; no room asked for
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nullptr, off, line, cov, 2, nullptr, nullptr) == SYZSIG_OK);
	CHECK(ARGS(&ctx, nullptr, nullptr, nullptr, 0, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_OK);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, nullptr, nullptr, nullptr, 0, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_OK);
	CHECK(ARGS(&ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, off, nullptr, nullptr, 0,
	           nullptr, nullptr) == SYZSIG_OK);
	CHECK(ARGS(&ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 1, 1, nl, off, nullptr, nullptr, 0, shown,
	           coverage) == SYZSIG_OK);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, nullptr, nullptr, 0, shown, coverage) ==
	      SYZSIG_OK);  // (cap 0 with entries is the device's ERANGE)
	// NULL forms
	CHECK(ARGS(nullptr, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, nullptr, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, nullptr, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, nullptr, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, nullptr, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, nullptr, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, nullptr, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, nullptr, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, nullptr, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, nullptr, 2, shown, coverage) == SYZSIG_EINVAL);
	// the walk's three arrays: all or none -- the six mixed forms
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, nullptr, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, nullptr) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, nullptr, nullptr) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nullptr, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nullptr, off, line, cov, 2, shown, nullptr) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nullptr, off, line, cov, 2, nullptr, coverage) == SYZSIG_EINVAL);
	// limits: files and functions below 2^32, frames of both lists together below 2^31
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, M32, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_ERANGE);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, M32, nl, off, line, cov, 2, shown, coverage) == SYZSIG_ERANGE);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, M32 - 1, M32 - 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_OK);
	CHECK(ARGS(&ctx, cf, cl, cfn, M31, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_ERANGE);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, M31, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_ERANGE);
	CHECK(ARGS(&ctx, cf, cl, cfn, M31 / 2, uf, ul, ufn, M31 / 2, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_ERANGE);
	CHECK(ARGS(&ctx, cf, cl, cfn, M31 / 2, uf, ul, ufn, M31 / 2 - 1, 1, 1, nl, off, line, cov, 2, shown, coverage) == SYZSIG_OK);
	CHECK(ARGS(&ctx, cf, cl, cfn, ~0ull, uf, ul, ufn, 2, 1, 1, nl, off, line, cov, 2, shown, coverage) ==
	      SYZSIG_ERANGE);  // (a sum that wraps)
	// frames need a file and a function to name
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 0, 1, nullptr, off, line, cov, 2, nullptr, nullptr) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, cf, cl, cfn, 1, nullptr, nullptr, nullptr, 0, 1, 0, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
	CHECK(ARGS(&ctx, nullptr, nullptr, nullptr, 0, uf, ul, ufn, 1, 1, 0, nl, off, line, cov, 2, shown, coverage) == SYZSIG_EINVAL);
#undef ARGS
	CHECK(file_set_args(nullptr, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage).msg != nullptr);
	CHECK(file_set_args(&ctx, cf, cl, cfn, 1, uf, ul, ufn, 1, 1, 1, nl, off, line, cov, 2, shown, coverage).msg == nullptr);
}

static void run_status()
{
	CHECK(file_set_frames_status(0, 0).code == SYZSIG_OK);
	CHECK(file_set_frames_status(1, 0).code == SYZSIG_EINVAL);
	CHECK(file_set_frames_status(0, 1).code == SYZSIG_EINVAL);
	CHECK(file_set_frames_status(3, 2).code == SYZSIG_EINVAL);
	CHECK(file_set_frames_status(1, 0).msg && file_set_frames_status(0, 1).msg);
	CHECK(file_set_cap_status(0, 0).code == SYZSIG_OK);
	CHECK(file_set_cap_status(10, 10).code == SYZSIG_OK);
	CHECK(file_set_cap_status(10, 11).code == SYZSIG_OK);
	CHECK(file_set_cap_status(10, 9).code == SYZSIG_ERANGE);
	CHECK(file_set_cap_status(1, 0).msg != nullptr);
}

static void run_key()
{
	const int32_t lo = INT32_MIN, hi = INT32_MAX;
	const int32_t lines[] = {lo, lo + 1, -1, 0, 1, 2, hi - 1, hi};
	const int n = sizeof(lines) / sizeof(lines[0]);
	for (int i = 0; i < n; i++) {
		const uint64_t c = file_set_key(lines[i], true), u = file_set_key(lines[i], false);
		CHECK(c + 1 == u);  // a line's covered entry directly before its uncovered one
		CHECK(c >> 1 == u >> 1);
		CHECK(file_set_key_line(c) == lines[i] && file_set_key_line(u) == lines[i]);
		CHECK(file_set_key_covered(c) && !file_set_key_covered(u));
		CHECK(u < (1ull << 33));  // below segsort.h's all-ones pad key
		if (i + 1 < n) {
			CHECK(u < file_set_key(lines[i + 1], true));  // signed order across lines
			CHECK(u >> 1 != file_set_key(lines[i + 1], true) >> 1);
		}
	}
	CHECK(file_set_key(lo, true) == 0 && file_set_key(hi, false) == (1ull << 33) - 1);
	// line <= nlines in 64 bits: i32 against u32
	CHECK(file_set_line_within(5, 5) && !file_set_line_within(6, 5) && file_set_line_within(4, 5));
	CHECK(!file_set_line_within(1, 0) && file_set_line_within(0, 0) && file_set_line_within(-1, 0));
	CHECK(file_set_line_within(hi, 0x80000000u) && file_set_line_within(hi, 0xffffffffu));
	CHECK(file_set_line_within(hi, (uint32_t)hi) && !file_set_line_within(hi, (uint32_t)hi - 1));
	CHECK(file_set_line_within(lo, 0) && file_set_line_within(lo, 0xffffffffu));
	CHECK(!file_set_block_path(0) && !file_set_block_path(kFileSetWaveEntries) &&
	      file_set_block_path(kFileSetWaveEntries + 1));
	// merge passes over the file-set tile: none up to a tile, one up to two tiles, two up to four
	const uint64_t T = SYZSIG_FILESET_TILE;
	CHECK(report_merge_passes(T, T) == 0 && report_merge_passes(T + 1, T) == 1 && report_merge_passes(2 * T, T) == 1);
	CHECK(report_merge_passes(2 * T + 1, T) == 2 && report_merge_passes(4 * T + 6, T) == 3);
}

int main()
{
	run_args();
	run_status();
	run_key();
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}
