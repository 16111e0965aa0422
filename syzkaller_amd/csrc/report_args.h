// report_args.h -- the host-side argument checks of report.hip's entry points:
// what is rejected before any device work, how the counters of the device-side
// checks become a status, previousInstructionPC's subtrahend per arch, and
// fileSet's sort key.  No HIP here, so that tests/report_driver.cc and
// tests/fileset_driver.cc run every branch on the CPU under ASan + UBSan.
// Whoever includes this has syzsig.h's codes and limits.
#pragma once

#include <cstdint>

#include "common.h"

namespace syz {

constexpr uint64_t kReportMaxPcs = 1ull << 31;    // PCs of one call (one sort segment)
constexpr uint64_t kReportMaxCount = 1ull << 32;  // inputs, calls, symbols, report PCs

struct ReportStatus {
	int code;  // SYZSIG_OK: go on
	const char* msg;
};

inline ReportStatus report_ok() { return ReportStatus{SYZSIG_OK, nullptr}; }

// syzsig_call_cover_dev before the corpus is looked at (it is device memory)
inline ReportStatus call_cover_args(const void* ctx, const uint64_t* d_cov_off, const uint32_t* d_cov, uint64_t ninputs,
                                    uint64_t total, const uint32_t* d_call, uint64_t ncalls, const uint32_t* d_count,
                                    const uint32_t* d_cover_len, const uint64_t* d_call_cov_off,
                                    const uint32_t* d_call_cov, uint64_t cover_cap, const uint32_t* d_all_cov,
                                    const uint64_t* n_all)
{
	if (!ctx)
		return ReportStatus{SYZSIG_EINVAL, "call_cover: NULL context"};
	if (!d_call_cov_off || (ncalls && (!d_count || !d_cover_len)) || (ninputs && (!d_cov_off || !d_call)) ||
	    (total && !d_cov) || (cover_cap && !d_call_cov))
		return ReportStatus{SYZSIG_EINVAL, "call_cover: NULL argument"};
	if ((d_all_cov != nullptr) != (n_all != nullptr))
		return ReportStatus{SYZSIG_EINVAL, "call_cover: the whole union needs both d_all_cov and n_all"};
	if (total && !ninputs)
		return ReportStatus{SYZSIG_EINVAL, "call_cover: PCs without inputs"};
	if (ninputs && !ncalls)
		return ReportStatus{SYZSIG_EINVAL, "call_cover: inputs without calls"};
	if (ninputs >= kReportMaxCount || ncalls >= kReportMaxCount)
		return ReportStatus{SYZSIG_ERANGE, "call_cover: 2^32 or more inputs or calls"};
	if (total >= kReportMaxPcs)
		return ReportStatus{SYZSIG_ERANGE, "call_cover: 2^31 or more PCs"};
	return report_ok();
}

// ... and after: `bad_off` offsets that decrease or do not run from 0 to total,
// `bad_call` call ids >= ncalls, `selected` = the selected inputs' PCs
inline ReportStatus call_cover_corpus_status(uint64_t bad_off, uint64_t bad_call, uint64_t selected, uint64_t cover_cap)
{
	if (bad_off)
		return ReportStatus{SYZSIG_EINVAL, "call_cover: the offsets decrease or do not run from 0 to total"};
	if (bad_call)
		return ReportStatus{SYZSIG_EINVAL, "call_cover: a call id is not below ncalls"};
	if (cover_cap < selected)
		return ReportStatus{SYZSIG_ERANGE, "call_cover: cover_cap is below the selected inputs' PCs"};
	return report_ok();
}

// previousInstructionPC (syz-manager/cover.go:394-411): pc - sub, then & mask.
// An unknown arch is Go's panic("unknown arch").
struct ReportArch {
	bool known;
	uint64_t sub, mask;
};

SYZ_HD ReportArch report_arch(uint32_t arch)
{
	switch (arch) {
	case SYZSIG_ARCH_AMD64:
		return ReportArch{true, 5, ~0ull};
	case SYZSIG_ARCH_386:
		return ReportArch{true, 1, ~0ull};
	case SYZSIG_ARCH_ARM64:
		return ReportArch{true, 4, ~0ull};
	case SYZSIG_ARCH_ARM:
		return ReportArch{true, 3, ~1ull};
	case SYZSIG_ARCH_PPC64LE:
		return ReportArch{true, 4, ~0ull};
	}
	return ReportArch{false, 0, 0};
}

// cover.RestorePC (pkg/cover/cover.go:28-30), then previousInstructionPC: u64 arithmetic, wrapping as Go's
SYZ_HD uint64_t report_prev_pc(const ReportArch& a, uint32_t base, uint32_t pc)
{
	return ((((uint64_t)base << 32) + pc) - a.sub) & a.mask;
}

inline ReportStatus report_pcs_args(const void* ctx, const uint32_t* d_pcs, uint64_t n, uint32_t arch,
                                    const uint64_t* d_out_order, const uint64_t* d_out_sorted)
{
	if (!ctx)
		return ReportStatus{SYZSIG_EINVAL, "report_pcs: NULL context"};
	if (!report_arch(arch).known)
		return ReportStatus{SYZSIG_EINVAL, "report_pcs: unknown arch"};
	if (n && (!d_pcs || !d_out_order || !d_out_sorted))
		return ReportStatus{SYZSIG_EINVAL, "report_pcs: NULL argument"};
	if (n >= kReportMaxPcs)
		return ReportStatus{SYZSIG_ERANGE, "report_pcs: 2^31 or more PCs"};
	return report_ok();
}

inline ReportStatus uncovered_args(const void* ctx, const uint64_t* d_sym_start, const uint64_t* d_sym_end,
                                   uint64_t nsym, const uint64_t* d_all_cover, uint64_t nall, const uint64_t* d_pcs,
                                   uint64_t npc, const uint64_t* d_out, const uint64_t* n_out)
{
	if (!ctx)
		return ReportStatus{SYZSIG_EINVAL, "uncovered_pcs: NULL context"};
	if (!n_out || (nsym && (!d_sym_start || !d_sym_end)) || (nall && (!d_all_cover || !d_out)) || (npc && !d_pcs))
		return ReportStatus{SYZSIG_EINVAL, "uncovered_pcs: NULL argument"};
	if (npc >= kReportMaxCount || nsym >= kReportMaxCount || nall >= kReportMaxCount)
		return ReportStatus{SYZSIG_ERANGE, "uncovered_pcs: 2^32 or more PCs, symbols or call sites"};
	return report_ok();
}

// ... and after: neighbours of d_all_cover that do not ascend strictly,
// neighbours of d_sym_start that descend
inline ReportStatus uncovered_tables_status(uint64_t bad_cover, uint64_t bad_sym)
{
	if (bad_cover)
		return ReportStatus{SYZSIG_EINVAL, "uncovered_pcs: d_all_cover repeats a PC or is not ascending"};
	if (bad_sym)
		return ReportStatus{SYZSIG_EINVAL, "uncovered_pcs: the symbols are not sorted by start"};
	return report_ok();
}

// syzsig_file_set_dev before the frames are looked at (they are device memory)
inline ReportStatus file_set_args(const void* ctx, const uint32_t* d_cov_file, const int32_t* d_cov_line,
                                  const uint32_t* d_cov_func, uint64_t ncov, const uint32_t* d_unc_file,
                                  const int32_t* d_unc_line, const uint32_t* d_unc_func, uint64_t nunc, uint64_t nfiles,
                                  uint64_t nfuncs, const uint32_t* d_nlines, const uint64_t* d_off, const int32_t* d_line,
                                  const uint8_t* d_covered, uint64_t cap, const uint32_t* d_shown,
                                  const uint32_t* d_coverage)
{
	if (!ctx)
		return ReportStatus{SYZSIG_EINVAL, "file_set: NULL context"};
	if (!d_off || (ncov && (!d_cov_file || !d_cov_line || !d_cov_func)) ||
	    (nunc && (!d_unc_file || !d_unc_line || !d_unc_func)) || (cap && (!d_line || !d_covered)))
		return ReportStatus{SYZSIG_EINVAL, "file_set: NULL argument"};
	if ((d_shown != nullptr) != (d_nlines != nullptr) || (d_coverage != nullptr) != (d_nlines != nullptr))
		return ReportStatus{SYZSIG_EINVAL, "file_set: the walk needs d_nlines, d_shown and d_coverage, all or none"};
	if (nfiles >= kReportMaxCount || nfuncs >= kReportMaxCount)
		return ReportStatus{SYZSIG_ERANGE, "file_set: 2^32 or more files or functions"};
	if (ncov >= kReportMaxPcs || nunc >= kReportMaxPcs || ncov + nunc >= kReportMaxPcs)
		return ReportStatus{SYZSIG_ERANGE, "file_set: 2^31 or more frames"};
	if ((ncov || nunc) && (!nfiles || !nfuncs))
		return ReportStatus{SYZSIG_EINVAL, "file_set: frames without files or functions"};
	return report_ok();
}

// ... after the frames' ids were checked: `bad_file` file ids >= nfiles, `bad_func` function ids >= nfuncs
inline ReportStatus file_set_frames_status(uint64_t bad_file, uint64_t bad_func)
{
	if (bad_file)
		return ReportStatus{SYZSIG_EINVAL, "file_set: a file id is not below nfiles"};
	if (bad_func)
		return ReportStatus{SYZSIG_EINVAL, "file_set: a function id is not below nfuncs"};
	return report_ok();
}

// ... and once the lists are known, before any is written: `entries` (file, line) pairs in all
inline ReportStatus file_set_cap_status(uint64_t entries, uint64_t cap)
{
	if (cap < entries)
		return ReportStatus{SYZSIG_ERANGE, "file_set: cap is below the entries of the files' lists"};
	return report_ok();
}

// fileSet's sort key of a (line, covered) pair inside its file: lines in signed
// order (Go's int), a line's covered entry directly before its uncovered one.
// 33 bits; two keys are entries of one line iff they agree above bit 0.
SYZ_HD uint64_t file_set_key(int32_t line, bool covered)
{
	return (uint64_t)((uint32_t)line ^ 0x80000000u) << 1 | (covered ? 0u : 1u);
}
SYZ_HD int32_t file_set_key_line(uint64_t key) { return (int32_t)((uint32_t)(key >> 1) ^ 0x80000000u); }
SYZ_HD bool file_set_key_covered(uint64_t key) { return !(key & 1); }

// the walk of cover.go:131-143 consumes an entry only at `line == i + 1` with
// i < nlines: an entry can be shown iff 1 <= line <= nlines (i32 against u32: in 64 bits)
SYZ_HD bool file_set_line_within(int32_t line, uint32_t nlines) { return (int64_t)line <= (int64_t)nlines; }

// A file whose list holds more entries than this is written and walked by a
// workgroup, a shorter one by a wave.
constexpr uint32_t kFileSetWaveEntries = 256;
SYZ_HD bool file_set_block_path(uint64_t entries) { return entries > kFileSetWaveEntries; }

// A handled function whose call sites number more than this is walked by a
// workgroup, a shorter range by the wave that found it.
constexpr uint32_t kReportWaveSites = 256;
SYZ_HD bool report_block_path(uint64_t nsites) { return nsites > kReportWaveSites; }

// merge passes of segsort.h over a longest segment of `maxlen` keys with tiles of `tile`
inline uint64_t report_merge_passes(uint64_t maxlen, uint64_t tile)
{
	uint64_t p = 0;
	for (uint64_t w = tile; w < maxlen; w <<= 1)
		p++;
	return p;
}

}  // namespace syz
