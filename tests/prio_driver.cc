// prio_driver.cc -- the host-compilable half of syzkaller_amd/csrc/prio.hip on
// the CPU, built under ASan + UBSan by tests/test_prio_ref_cpu.py: every branch
// of csrc/prio_args.h -- the argument checks of syzsig_calc_prios_dev,
// syzsig_static_prio_finish_dev, syzsig_choice_table_dev and
// syzsig_choice_lookup_dev (EINVAL, ERANGE, the NULL forms), how the corpus
// check's counters become a status, and the slicing plan's arithmetic (the
// threshold's default and its raise, the slices of a row at and past it, the
// bound on the partial rows' workspace).
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../include/syzsig.h"
#include "../syzkaller_amd/csrc/prio_args.h"

using namespace syz;

static int g_fail = 0;
#define CHECK(c)                                                    \
	do {                                                            \
		if (!(c)) {                                                 \
			printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
			g_fail++;                                               \
		}                                                           \
	} while (0)

static void run_calc_args()
{
	int ctx = 0;
	const uint64_t off[2] = {0, 1};
	const uint32_t id[1] = {0};
	float prios[1];
	CHECK(calc_prios_args(&ctx, off, id, 1, 1, 1, prios).code == SYZSIG_OK);
	CHECK(calc_prios_args(&ctx, nullptr, nullptr, 0, 0, 1, prios).code == SYZSIG_OK);  // the empty corpus
	CHECK(calc_prios_args(&ctx, off, nullptr, 1, 0, 1, prios).code == SYZSIG_OK);      // one empty program
	CHECK(calc_prios_args(nullptr, off, id, 1, 1, 1, prios).code == SYZSIG_EINVAL);
	CHECK(calc_prios_args(&ctx, nullptr, id, 1, 1, 1, prios).code == SYZSIG_EINVAL);
	CHECK(calc_prios_args(&ctx, off, nullptr, 1, 1, 1, prios).code == SYZSIG_EINVAL);
	CHECK(calc_prios_args(&ctx, off, id, 1, 1, 1, nullptr).code == SYZSIG_EINVAL);
	CHECK(calc_prios_args(&ctx, off, id, 0, 1, 1, prios).code == SYZSIG_EINVAL);  // calls without programs
	CHECK(calc_prios_args(&ctx, off, id, 1, 1, 0, prios).code == SYZSIG_EINVAL);
	CHECK(calc_prios_args(&ctx, off, id, 1, 1, SYZSIG_PRIO_MAX_CALLS, prios).code == SYZSIG_OK);
	CHECK(calc_prios_args(&ctx, off, id, 1, 1, SYZSIG_PRIO_MAX_CALLS + 1, prios).code == SYZSIG_ERANGE);
	CHECK(calc_prios_args(&ctx, off, id, 1, 1ull << 32, 1, prios).code == SYZSIG_ERANGE);
	CHECK(calc_prios_args(&ctx, off, id, 1, (1ull << 32) - 1, 1, prios).code == SYZSIG_OK);
	CHECK(calc_prios_args(&ctx, off, id, 1ull << 32, 1, 1, prios).code == SYZSIG_ERANGE);
	CHECK(calc_prios_args(&ctx, off, id, 1, 1, SYZSIG_PRIO_MAX_CALLS + 1, prios).msg != nullptr);
	// the corpus check's counters: (bad offsets, bad ids, programs of 2^16 calls or more, sum of len^2)
	CHECK(calc_prios_corpus_status(0, 0, 0, 0).code == SYZSIG_OK);
	CHECK(calc_prios_corpus_status(0, 0, 0, (1ull << 32) - 1).code == SYZSIG_OK);
	CHECK(calc_prios_corpus_status(0, 0, 0, 1ull << 32).code == SYZSIG_ERANGE);
	CHECK(calc_prios_corpus_status(0, 0, 1, 0).code == SYZSIG_ERANGE);
	CHECK(calc_prios_corpus_status(1, 0, 0, 0).code == SYZSIG_EINVAL);
	CHECK(calc_prios_corpus_status(0, 1, 0, 0).code == SYZSIG_EINVAL);
	CHECK(calc_prios_corpus_status(1, 1, 1, 1ull << 40).code == SYZSIG_EINVAL);  // bad offsets make the lengths meaningless
	CHECK(calc_prios_corpus_status(0, 1, 1, 0).code == SYZSIG_EINVAL);           // Go panics on the index first
	CHECK(calc_prios_corpus_status(1, 0, 0, 0).msg && calc_prios_corpus_status(0, 0, 1, 0).msg);
}

static void run_split()
{
	CHECK(prio_split(0, 1000, 100) == SYZSIG_PRIO_SPLIT);
	CHECK(prio_split(1, 1000, 100) == 1 && prio_split(7, 1000, 100) == 7);
	CHECK(prio_row_slices(0, 4) == 0 && prio_row_slices(4, 4) == 0);  // at the threshold: whole
	CHECK(prio_row_slices(5, 4) == 2 && prio_row_slices(8, 4) == 2 && prio_row_slices(9, 4) == 3);
	CHECK(prio_row_slices(2, 1) == 2 && prio_row_slices(1, 1) == 0);
	// the partial rows fit the workspace whatever was asked: at most total / s + N slices of 4 N bytes
	const uint64_t totals[] = {0, 1, 4096, 3000000, (1ull << 32) - 1};
	const uint64_t ns[] = {1, 2, 257, 3500, 4096, 4097, SYZSIG_PRIO_MAX_CALLS};
	for (uint64_t total : totals)
		for (uint64_t N : ns)
			for (uint64_t ask : {0ull, 1ull, 7ull, 4096ull, 1ull << 40}) {
				const uint64_t s = prio_split(ask, total, N);
				CHECK(s >= (ask ? ask : (uint64_t)SYZSIG_PRIO_SPLIT));
				// a row is split only past s postings, so there are fewer than total / s split rows
				const uint64_t most = total / s + (total / s < N ? total / s : N);
				CHECK(most * N * 4 <= kPrioPartialBytes || total <= s);
			}
	CHECK(prio_split(1, (1ull << 32) - 1, SYZSIG_PRIO_MAX_CALLS) >= (1ull << 32) - 1);  // no room: never split
}

static void run_table_args()
{
	int ctx = 0;
	float m[1];
	int32_t run[1], call[1] = {0}, x[1] = {1}, out[1];
	CHECK(static_finish_args(&ctx, m, 1).code == SYZSIG_OK);
	CHECK(static_finish_args(nullptr, m, 1).code == SYZSIG_EINVAL);
	CHECK(static_finish_args(&ctx, nullptr, 1).code == SYZSIG_EINVAL);
	CHECK(static_finish_args(&ctx, m, 0).code == SYZSIG_EINVAL);
	CHECK(static_finish_args(&ctx, m, SYZSIG_PRIO_MAX_CALLS + 1).code == SYZSIG_ERANGE);
	CHECK(choice_table_args(&ctx, 1, run).code == SYZSIG_OK);
	CHECK(choice_table_args(nullptr, 1, run).code == SYZSIG_EINVAL);
	CHECK(choice_table_args(&ctx, 1, nullptr).code == SYZSIG_EINVAL);
	CHECK(choice_table_args(&ctx, 0, run).code == SYZSIG_EINVAL);
	CHECK(choice_table_args(&ctx, SYZSIG_PRIO_MAX_CALLS + 1, run).code == SYZSIG_ERANGE);
	CHECK(choice_lookup_args(&ctx, run, 1, call, x, 1, out).code == SYZSIG_OK);
	CHECK(choice_lookup_args(&ctx, run, 1, nullptr, nullptr, 0, nullptr).code == SYZSIG_OK);  // no queries
	CHECK(choice_lookup_args(nullptr, run, 1, call, x, 1, out).code == SYZSIG_EINVAL);
	CHECK(choice_lookup_args(&ctx, nullptr, 1, call, x, 1, out).code == SYZSIG_EINVAL);
	CHECK(choice_lookup_args(&ctx, run, 1, nullptr, x, 1, out).code == SYZSIG_EINVAL);
	CHECK(choice_lookup_args(&ctx, run, 1, call, nullptr, 1, out).code == SYZSIG_EINVAL);
	CHECK(choice_lookup_args(&ctx, run, 1, call, x, 1, nullptr).code == SYZSIG_EINVAL);
	CHECK(choice_lookup_args(&ctx, run, 0, call, x, 1, out).code == SYZSIG_EINVAL);
	CHECK(choice_lookup_args(&ctx, run, SYZSIG_PRIO_MAX_CALLS + 1, call, x, 1, out).code == SYZSIG_ERANGE);
	CHECK(choice_lookup_args(&ctx, run, 1, call, x, 1ull << 32, out).code == SYZSIG_ERANGE);
	// N weights below the limit sum inside an int32
	CHECK(choice_weight_limit(1) == 2147483648.0f && choice_weight_limit(4) == 536870912.0f);
	for (uint64_t N : {1ull, 3ull, 1000ull, (unsigned long long)SYZSIG_PRIO_MAX_CALLS}) {
		const float lim = choice_weight_limit(N);
		// the largest weight that passes: the float below the limit, truncated
		float below = lim;
		uint32_t bits;
		static_assert(sizeof(bits) == sizeof(below), "float is 32 bits");
		__builtin_memcpy(&bits, &below, 4);
		bits--;
		__builtin_memcpy(&below, &bits, 4);
		CHECK(below < lim && (uint64_t)below * N < (1ull << 31));
	}
}

int main()
{
	run_calc_args();
	run_split();
	run_table_args();
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}
