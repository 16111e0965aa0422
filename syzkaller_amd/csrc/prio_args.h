// prio_args.h -- the host-side argument checks of prio.hip's entry points: what
// is rejected before any device work, how the counters of the corpus check
// become a status, and the slicing plan's arithmetic.  No HIP here, so that
// tests/prio_driver.cc runs every branch on the CPU under ASan + UBSan.  Whoever
// includes this has syzsig.h's codes and limits.
#pragma once

#include <cstdint>

#include "common.h"

namespace syz {

constexpr uint64_t kPrioMaxCalls = SYZSIG_PRIO_MAX_CALLS;
constexpr uint64_t kPrioSplitDefault = SYZSIG_PRIO_SPLIT;
constexpr uint64_t kPrioPartialBytes = 1ull << 30;  // the slices' partial rows in the workspace, at most
constexpr uint64_t kPrioMaxQueries = 1ull << 32;

struct PrioStatus {
	int code;  // SYZSIG_OK: go on
	const char* msg;
};

inline PrioStatus prio_ok() { return PrioStatus{SYZSIG_OK, nullptr}; }

// the matrix side N of every entry point
inline PrioStatus prio_ncalls(const void* ctx, uint64_t N, const char* who_null, const char* who_zero,
                              const char* who_range)
{
	if (!ctx)
		return PrioStatus{SYZSIG_EINVAL, who_null};
	if (N == 0)
		return PrioStatus{SYZSIG_EINVAL, who_zero};
	if (N > kPrioMaxCalls)
		return PrioStatus{SYZSIG_ERANGE, who_range};
	return prio_ok();
}

// syzsig_calc_prios_dev before the corpus is looked at (it is device memory)
inline PrioStatus calc_prios_args(const void* ctx, const uint64_t* d_prog_off, const uint32_t* d_call_id,
                                  uint64_t nprog, uint64_t total, uint64_t N, const float* d_prios)
{
	const PrioStatus n = prio_ncalls(ctx, N, "calc_prios: NULL context", "calc_prios: N is 0",
	                                 "calc_prios: N is above SYZSIG_PRIO_MAX_CALLS");
	if (n.code != SYZSIG_OK)
		return n;
	if (!d_prios || (nprog && !d_prog_off) || (total && !d_call_id))
		return PrioStatus{SYZSIG_EINVAL, "calc_prios: NULL argument"};
	if (total && !nprog)
		return PrioStatus{SYZSIG_EINVAL, "calc_prios: calls without programs"};
	// a program of len calls adds len^2 >= len pairs: 2^32 calls are 2^32 pairs at the least
	if (total >= 1ull << 32 || nprog >= 1ull << 32)
		return PrioStatus{SYZSIG_ERANGE, "calc_prios: 2^32 or more pair increments"};
	return prio_ok();
}

// ... and after: `bad_off` offsets that decrease or do not end at total, `bad_id`
// ids >= N, `pairs` = sum of len^2 with `huge` programs of 2^16 calls or more
// left out (their squares alone reach 2^32)
inline PrioStatus calc_prios_corpus_status(uint64_t bad_off, uint64_t bad_id, uint64_t huge, uint64_t pairs)
{
	if (bad_off)
		return PrioStatus{SYZSIG_EINVAL, "calc_prios: the offsets decrease or do not end at total"};
	if (bad_id)
		return PrioStatus{SYZSIG_EINVAL, "calc_prios: a call id is not below N"};
	if (huge || pairs >= 1ull << 32)
		return PrioStatus{SYZSIG_ERANGE, "calc_prios: 2^32 or more pair increments"};
	return prio_ok();
}

// The postings of one slice.  split = 0 is the default; a row of more than
// `split` postings is cut into slices of `split`.  A slice costs N u32 of
// workspace and there are at most total / split + N of them, so the threshold is
// raised until those fit kPrioPartialBytes: the result does not depend on it.
inline uint64_t prio_split(uint64_t split, uint64_t total, uint64_t N)
{
	uint64_t s = split ? split : kPrioSplitDefault;
	const uint64_t rows = kPrioPartialBytes / (4 * N);  // >= 2^14 for N <= 2^14
	const uint64_t room = rows > N ? rows - N : 1;
	const uint64_t need = (total + room - 1) / room;    // total / s <= room
	return s < need ? need : s;
}

// slices of a row of `cnt` postings (0: the row is counted whole by its own workgroup)
SYZ_HD uint64_t prio_row_slices(uint64_t cnt, uint64_t split) { return cnt > split ? (cnt + split - 1) / split : 0; }

inline PrioStatus static_finish_args(const void* ctx, const float* d_prios, uint64_t N)
{
	const PrioStatus n = prio_ncalls(ctx, N, "static_prio_finish: NULL context", "static_prio_finish: N is 0",
	                                 "static_prio_finish: N is above SYZSIG_PRIO_MAX_CALLS");
	if (n.code != SYZSIG_OK)
		return n;
	if (!d_prios)
		return PrioStatus{SYZSIG_EINVAL, "static_prio_finish: NULL argument"};
	return prio_ok();
}

inline PrioStatus choice_table_args(const void* ctx, uint64_t N, const int32_t* d_run)
{
	const PrioStatus n = prio_ncalls(ctx, N, "choice_table: NULL context", "choice_table: N is 0",
	                                 "choice_table: N is above SYZSIG_PRIO_MAX_CALLS");
	if (n.code != SYZSIG_OK)
		return n;
	if (!d_run)
		return PrioStatus{SYZSIG_EINVAL, "choice_table: NULL argument"};
	return prio_ok();
}

inline PrioStatus choice_lookup_args(const void* ctx, const int32_t* d_run, uint64_t N, const int32_t* d_call,
                                     const int32_t* d_x, uint64_t n, const int32_t* d_out)
{
	const PrioStatus s = prio_ncalls(ctx, N, "choice_lookup: NULL context", "choice_lookup: N is 0",
	                                 "choice_lookup: N is above SYZSIG_PRIO_MAX_CALLS");
	if (s.code != SYZSIG_OK)
		return s;
	if (n >= kPrioMaxQueries)
		return PrioStatus{SYZSIG_ERANGE, "choice_lookup: 2^32 or more queries"};
	if (!d_run || (n && (!d_call || !d_x || !d_out)))
		return PrioStatus{SYZSIG_EINVAL, "choice_lookup: NULL argument"};
	return prio_ok();
}

// the weight int(p * 1000) of BuildChoiceTable must stay below this for N of
// them to sum inside an int32: 2^31 / N, in float as the kernel compares it
inline float choice_weight_limit(uint64_t N) { return 2147483648.0f / (float)N; }

}  // namespace syz
