// dbw_driver.cc -- the host-compilable halves of pkg/db's write side in
// syzkaller_amd/csrc on the CPU, built under ASan + UBSan by
// tests/test_dbw_ref_cpu.py:
//   dbw_driver args          every branch of csrc/db_args.h's checks for
//                            syzsig_deflate_dev, syzsig_deflate_host (with its
//                            sizing and ERANGE convention), syzsig_db_records_dev
//                            and syzsig_db_apply_dev
//   dbw_driver deflate FILE  csrc/deflate_core.h over the values of FILE: u32
//                            count, then per value u32 length and the bytes.
//                            The value and the stream live in heap blocks of
//                            exactly their sizes, so one byte read past the
//                            value -- the bytes a hash or a match would want
//                            behind its end -- or written past the counted
//                            length is an ASan report.  Each stream is inflated
//                            back with csrc/inflate_core.h and compared; a
//                            capacity one byte short must report it and stay
//                            inside; prints the stream's size per value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/syzsig.h"
#include "../syzkaller_amd/csrc/db_args.h"
#include "../syzkaller_amd/csrc/deflate_core.h"
#include "../syzkaller_amd/csrc/inflate_core.h"

using namespace syz;

static int g_fail = 0;
#define CHECK(c)                                                    \
	do {                                                            \
		if (!(c)) {                                                 \
			printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
			g_fail++;                                               \
		}                                                           \
	} while (0)

static int run_args()
{
	int ctx = 0;
	const uint8_t byte = 0;
	uint8_t out = 0;
	const uint64_t off[2] = {0, 0}, seq = 0;
	const uint32_t len = 0;
	uint64_t ooff[2], total = 0, a = 0, b = 0;
	uint8_t sig[20] = {0};
	// syzsig_deflate_dev
	CHECK(deflate_args(&ctx, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, ooff, &total).code == SYZSIG_OK);
	CHECK(deflate_args(nullptr, &byte, 1, off, &len, 1, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(deflate_args(&ctx, &byte, 1, off, &len, 1, &out, 1, ooff, &total).code == SYZSIG_OK);
	CHECK(deflate_args(&ctx, nullptr, 1, off, &len, 1, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(deflate_args(&ctx, nullptr, 0, off, &len, 1, &out, 1, ooff, &total).code == SYZSIG_OK);
	CHECK(deflate_args(&ctx, &byte, 1, nullptr, &len, 1, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(deflate_args(&ctx, &byte, 1, off, nullptr, 1, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(deflate_args(&ctx, &byte, 1, off, &len, 1, &out, 1, nullptr, &total).code == SYZSIG_EINVAL);
	CHECK(deflate_args(&ctx, &byte, 1, off, &len, 1, &out, 1, ooff, nullptr).code == SYZSIG_EINVAL);
	CHECK(deflate_args(&ctx, &byte, 1, off, &len, 1, nullptr, 0, ooff, &total).code == SYZSIG_OK);  // sizing
	CHECK(deflate_args(&ctx, &byte, 1, off, &len, 1, nullptr, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(deflate_args(&ctx, &byte, 1, off, &len, kInflateMaxBatch, &out, 1, ooff, &total).code == SYZSIG_OK);
	CHECK(deflate_args(&ctx, &byte, 1, off, &len, kInflateMaxBatch + 1, &out, 1, ooff, &total).code == SYZSIG_ERANGE);
	CHECK(deflate_ranges_status(0, 0).code == SYZSIG_OK && deflate_ranges_status(2, 0).code == SYZSIG_EINVAL);
	CHECK(deflate_ranges_status(0, 1).code == SYZSIG_ERANGE && deflate_ranges_status(1, 1).code == SYZSIG_EINVAL);
	CHECK(write_room(10, 10, false, "x").code == SYZSIG_OK && write_room(10, 9, false, "x").code == SYZSIG_ERANGE);
	CHECK(write_room(10, 0, true, "x").code == SYZSIG_OK && write_room(0, 0, false, "x").code == SYZSIG_OK);
	// syzsig_deflate_host
	CHECK(deflate_host_args(&byte, 1, &out, 1, &total, 8).code == SYZSIG_OK);
	CHECK(deflate_host_args(nullptr, 0, nullptr, 0, &total, 8).code == SYZSIG_OK);  // the empty value, sizing
	CHECK(deflate_host_args(nullptr, 1, &out, 1, &total, 8).code == SYZSIG_EINVAL);
	CHECK(deflate_host_args(&byte, 1, nullptr, 1, &total, 8).code == SYZSIG_EINVAL);
	CHECK(deflate_host_args(&byte, 1, &out, 1, nullptr, 8).code == SYZSIG_EINVAL);
	CHECK(deflate_host_args(&byte, 8, &out, 1, &total, 8).code == SYZSIG_OK);
	CHECK(deflate_host_args(&byte, 9, &out, 1, &total, 8).code == SYZSIG_ERANGE);
	// syzsig_db_records_dev
	CHECK(db_records_args(&ctx, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, ooff, &total).code == SYZSIG_OK);
	CHECK(db_records_args(&ctx, sig, &seq, 1, &byte, 1, off, &out, 1, ooff, &total).code == SYZSIG_OK);
	CHECK(db_records_args(nullptr, sig, &seq, 1, &byte, 1, off, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, nullptr, &seq, 1, &byte, 1, off, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, sig, nullptr, 1, &byte, 1, off, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, sig, &seq, 1, nullptr, 1, off, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, sig, &seq, 1, nullptr, 0, off, &out, 1, ooff, &total).code == SYZSIG_OK);
	CHECK(db_records_args(&ctx, sig, &seq, 1, &byte, 1, nullptr, &out, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, sig, &seq, 1, &byte, 1, off, nullptr, 1, ooff, &total).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, sig, &seq, 1, &byte, 1, off, nullptr, 0, ooff, &total).code == SYZSIG_OK);  // sizing
	CHECK(db_records_args(&ctx, sig, &seq, 1, &byte, 1, off, &out, 1, nullptr, &total).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, sig, &seq, 1, &byte, 1, off, &out, 1, ooff, nullptr).code == SYZSIG_EINVAL);
	CHECK(db_records_args(&ctx, sig, &seq, kSigsMaxBatch + 1, &byte, 1, off, &out, 1, ooff, &total).code == SYZSIG_ERANGE);
	CHECK(db_records_status(0, 0, 0).code == SYZSIG_OK && db_records_status(1, 1, 1).code == SYZSIG_EINVAL);
	CHECK(db_records_status(0, 1, 1).code == SYZSIG_EINVAL && db_records_status(0, 0, 1).code == SYZSIG_ERANGE);
	// syzsig_db_apply_dev
	CHECK(db_apply_args(&ctx, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr,
	                    nullptr, nullptr, &total, &a, &b).code == SYZSIG_OK);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, &out, &total, &a, &b).code ==
	      SYZSIG_OK);
	CHECK(db_apply_args(nullptr, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, &out, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, nullptr, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, &out, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, nullptr, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, &out, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, nullptr, 0, off, sig, &seq, 1, nullptr, 0, off, &out, &out, &out, &total, &a,
	                    &b).code == SYZSIG_OK);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, nullptr, 1, &byte, 1, off, &out, &out, &out, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, nullptr, &out, &out, &out, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, nullptr, &out, &out, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, nullptr, &out, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, nullptr, &total, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, &out, nullptr, &a,
	                    &b).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, 1, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, &out, &total, &a,
	                    nullptr).code == SYZSIG_EINVAL);
	CHECK(db_apply_args(&ctx, sig, &seq, kSigsMaxBatch, &byte, 1, off, sig, &seq, 1, &byte, 1, off, &out, &out, &out, &total,
	                    &a, &b).code == SYZSIG_ERANGE);
	CHECK(db_apply_args(&ctx, nullptr, nullptr, 0, nullptr, 0, nullptr, sig, &seq, kSigsMaxBatch, &byte, 1, off, &out, nullptr,
	                    &out, &total, &a, &b).code == SYZSIG_OK);  // no live set: its arrays may be NULL
	CHECK(db_apply_status(0, 0, 0).code == SYZSIG_OK && db_apply_status(1, 0, 0).code == SYZSIG_EINVAL);
	CHECK(db_apply_status(0, 1, 0).code == SYZSIG_EINVAL && db_apply_status(0, 0, 1).code == SYZSIG_EINVAL);
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

// a heap block of exactly n bytes (n = 0: one byte that nobody may touch is still a valid pointer)
static uint8_t* exact(const uint8_t* from, uint64_t n)
{
	uint8_t* p = (uint8_t*)malloc(n ? n : 1);
	if (from && n)
		memcpy(p, from, n);
	return p;
}

static int run_deflate(const char* path)
{
	FILE* f = fopen(path, "rb");
	if (!f)
		return 2;
	std::vector<uint8_t> blob;
	uint8_t chunk[65536];
	for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;)
		blob.insert(blob.end(), chunk, chunk + k);
	fclose(f);
	uint32_t count;
	memcpy(&count, blob.data(), 4);
	size_t at = 4;
	DeflateTabArray* t = new DeflateTabArray;
	InflateTabArray* it = new InflateTabArray;
	for (uint32_t c = 0; c < count; c++) {
		uint32_t n;
		memcpy(&n, blob.data() + at, 4);
		at += 4;
		uint8_t* val = exact(blob.data() + at, n);
		at += n;
		memset(t->c, 0xEE, sizeof t->c);  // what another value left in the table must not matter
		const DeflateResult r0 = deflate_stream(val, n, nullptr, 0, 0, *t);
		CHECK((n == 0) == (r0.out_len == 0));
		CHECK(n == 0 || r0.out_len <= deflate_stored_len(n));
		uint8_t* out = exact(nullptr, r0.out_len);
		memset(t->c, 0x11, sizeof t->c);
		const DeflateResult r1 = deflate_stream(val, n, out, r0.out_len, r0.out_len, *t);
		CHECK(r1.out_len == r0.out_len && r1.fits && r1.stored == r0.stored);
		if (r0.out_len) {
			// one byte short: reported, and nothing outside the block
			uint8_t* tight = exact(nullptr, r0.out_len - 1);
			const DeflateResult r2 = deflate_stream(val, n, tight, r0.out_len - 1, 0, *t);
			CHECK(!r2.fits && r2.out_len == r0.out_len);
			CHECK(r0.out_len < 2 || memcmp(tight, out, r0.out_len - 1) == 0);
			free(tight);
			uint8_t* back = exact(nullptr, n);
			const InflateResult ir = inflate_stream(out, r0.out_len, back, n, SYZSIG_INFLATE_MAX_OUT, *it);
			CHECK(ir.status == kInfOk && ir.out_len == n && memcmp(back, val, n) == 0);
			CHECK(ir.stored + ir.fixed + ir.dynamic == (r0.stored ? (n + 65534) / 65535 : 1) && ir.dynamic == 0);
			free(back);
		}
		printf("%llu\n", (unsigned long long)r0.out_len);
		free(out);
		free(val);
	}
	delete t;
	delete it;
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

int main(int argc, char** argv)
{
	if (argc >= 2 && !strcmp(argv[1], "args"))
		return run_args();
	if (argc >= 3 && !strcmp(argv[1], "deflate"))
		return run_deflate(argv[2]);
	fprintf(stderr, "usage: dbw_driver args | deflate FILE\n");
	return 2;
}
