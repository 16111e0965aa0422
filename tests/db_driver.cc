// db_driver.cc -- the host-compilable halves of syzkaller_amd/csrc/db.hip on the
// CPU, built under ASan + UBSan by tests/test_db_ref_cpu.py:
//   db_driver args          every branch of csrc/db_args.h's argument checks:
//                           syzsig_db_scan, syzsig_inflate_dev, syzsig_db_live_dev
//   db_driver scan FILE     db_scan over every prefix of FILE, each from a heap
//                           block of exactly the prefix's size; prints, per
//                           prefix, "n ended version" for the test to hold against
//                           tests/db_ref.py; then hostile lengths patched into
//                           copies of the file
//   db_driver inflate FILE  csrc/inflate_core.h over the cases of FILE: u32
//                           ncases, u32 max_out, then per case u32 in_len, u32
//                           status, u32 out_len, the stream, the expected bytes.
//                           Stream and output live in heap blocks of exactly
//                           their sizes, so one byte read or written past
//                           either end is an ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/syzsig.h"
#include "../syzkaller_amd/csrc/db_args.h"
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
	uint8_t out = 0, status = 0;
	const uint64_t off = 0;
	const uint32_t len = 0;
	uint64_t ooff[2], total = 0, ver = 0, n = 0;
	uint32_t ended = 0;
	// syzsig_db_scan
	CHECK(db_scan_args(nullptr, 0, &ver, &n, &ended).code == SYZSIG_OK);  // the empty file needs no data
	CHECK(db_scan_args(nullptr, 1, &ver, &n, &ended).code == SYZSIG_EINVAL);
	CHECK(db_scan_args(&byte, 1, nullptr, &n, &ended).code == SYZSIG_EINVAL);
	CHECK(db_scan_args(&byte, 1, &ver, nullptr, &ended).code == SYZSIG_EINVAL);
	CHECK(db_scan_args(&byte, 1, &ver, &n, nullptr).code == SYZSIG_EINVAL);
	CHECK(db_scan_room(0, 0, false).code == SYZSIG_OK);
	CHECK(db_scan_room(3, 2, true).code == SYZSIG_ERANGE);
	CHECK(db_scan_room(3, 0, false).code == SYZSIG_ERANGE);  // the sizing call: the size comes first
	CHECK(db_scan_room(3, 3, false).code == SYZSIG_EINVAL);
	CHECK(db_scan_room(3, 3, true).code == SYZSIG_OK);
	// syzsig_inflate_dev
	CHECK(inflate_args(&ctx, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, ooff, nullptr, &total).code == SYZSIG_OK);
	CHECK(inflate_args(nullptr, &byte, 1, &off, &len, 1, &out, 1, ooff, &status, &total).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, 1, &out, 1, ooff, &status, &total).code == SYZSIG_OK);
	CHECK(inflate_args(&ctx, nullptr, 1, &off, &len, 1, &out, 1, ooff, &status, &total).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, nullptr, 0, &off, &len, 1, &out, 1, ooff, &status, &total).code == SYZSIG_OK);
	CHECK(inflate_args(&ctx, &byte, 1, nullptr, &len, 1, &out, 1, ooff, &status, &total).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, &byte, 1, &off, nullptr, 1, &out, 1, ooff, &status, &total).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, 1, &out, 1, nullptr, &status, &total).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, 1, &out, 1, ooff, nullptr, &total).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, 1, &out, 1, ooff, &status, nullptr).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, 1, nullptr, 0, ooff, &status, &total).code == SYZSIG_OK);  // sizing
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, 1, nullptr, 1, ooff, &status, &total).code == SYZSIG_EINVAL);
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, kInflateMaxBatch, &out, 1, ooff, &status, &total).code == SYZSIG_OK);
	CHECK(inflate_args(&ctx, &byte, 1, &off, &len, kInflateMaxBatch + 1, &out, 1, ooff, &status, &total).code ==
	      SYZSIG_ERANGE);
	CHECK(inflate_ranges_status(0).code == SYZSIG_OK && inflate_ranges_status(2).code == SYZSIG_EINVAL);
	CHECK(inflate_room(10, 10, false).code == SYZSIG_OK);
	CHECK(inflate_room(10, 9, false).code == SYZSIG_ERANGE);
	CHECK(inflate_room(10, 0, true).code == SYZSIG_OK);
	CHECK(inflate_room(0, 0, false).code == SYZSIG_OK);
	// syzsig_db_live_dev
	uint8_t sig[20] = {0};
	const uint64_t seq = 0;
	CHECK(db_live_args(&ctx, nullptr, nullptr, 0, 0, nullptr, &total, &n).code == SYZSIG_OK);
	CHECK(db_live_args(nullptr, sig, &seq, 1, 1, &out, &total, &n).code == SYZSIG_EINVAL);
	CHECK(db_live_args(&ctx, sig, &seq, 1, 1, &out, &total, &n).code == SYZSIG_OK);
	CHECK(db_live_args(&ctx, sig, &seq, 1, 0, &out, &total, &n).code == SYZSIG_OK);
	CHECK(db_live_args(&ctx, sig, &seq, 1, 2, &out, &total, &n).code == SYZSIG_EINVAL);
	CHECK(db_live_args(&ctx, nullptr, &seq, 1, 1, &out, &total, &n).code == SYZSIG_EINVAL);
	CHECK(db_live_args(&ctx, sig, nullptr, 1, 1, &out, &total, &n).code == SYZSIG_EINVAL);
	CHECK(db_live_args(&ctx, sig, &seq, 1, 1, nullptr, &total, &n).code == SYZSIG_EINVAL);
	CHECK(db_live_args(&ctx, sig, &seq, 1, 1, &out, nullptr, &n).code == SYZSIG_EINVAL);
	CHECK(db_live_args(&ctx, sig, &seq, 1, 1, &out, &total, nullptr).code == SYZSIG_EINVAL);
	CHECK(db_live_args(&ctx, sig, &seq, kSigsMaxBatch + 1, 1, &out, &total, &n).code == SYZSIG_ERANGE);
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

static bool read_file(const char* path, std::vector<uint8_t>& d)
{
	FILE* f = fopen(path, "rb");
	if (!f)
		return false;
	fseek(f, 0, SEEK_END);
	const long sz = ftell(f);
	fseek(f, 0, SEEK_SET);
	d.resize((size_t)sz);
	const bool ok = sz == 0 || fread(d.data(), 1, (size_t)sz, f) == (size_t)sz;
	fclose(f);
	return ok;
}

// db_scan of data[0 .. n) from a block of exactly n bytes: the counting walk, then the filling one into
// arrays of exactly the counted size; checks that both agree and every range lies inside the block
static DbScan scan_tight(const uint8_t* data, size_t n, bool check_ranges = true)
{
	uint8_t* tight = n ? (uint8_t*)malloc(n) : nullptr;
	if (n)
		memcpy(tight, data, n);
	const DbScan a = db_scan(tight, n, nullptr, nullptr, nullptr, nullptr, nullptr);
	std::vector<uint64_t> ko(a.n), sq(a.n), vo(a.n);
	std::vector<uint32_t> kl(a.n), vl(a.n);
	const DbScan b = db_scan(tight, n, a.n ? ko.data() : nullptr, kl.data(), sq.data(), vo.data(), vl.data());
	CHECK(a.n == b.n && a.ended == b.ended && a.version == b.version);
	for (uint64_t i = 0; check_ranges && i < a.n; i++) {
		CHECK(ko[i] <= n && kl[i] <= n - ko[i]);
		CHECK(vo[i] <= n && vl[i] <= n - vo[i]);
		CHECK(sq[i] != kDbSeqDeleted || (vo[i] == 0 && vl[i] == 0));
		CHECK(vl[i] != 0 || vo[i] == 0);
	}
	free(tight);
	return a;
}

static void put32(std::vector<uint8_t>& d, size_t at, uint32_t v)
{
	for (int i = 0; i < 4; i++)
		d[at + i] = (uint8_t)(v >> (8 * i));
}

static int run_scan(const char* path)
{
	std::vector<uint8_t> d;
	if (!read_file(path, d))
		return 2;
	for (size_t n = 0; n <= d.size(); n++) {
		const DbScan r = scan_tight(d.data(), n);
		printf("%llu %u %llu\n", (unsigned long long)r.n, r.ended, (unsigned long long)r.version);
	}
	// Hostile lengths.  The file is a version-2 header (16 bytes) and records whose first has its key
	// length at byte 20; the whole file scans clean.
	const DbScan whole = scan_tight(d.data(), d.size());
	CHECK(whole.ended == SYZSIG_DB_END_EOF && whole.n >= 2 && d.size() > 40);
	const uint32_t kl0 = db_u32(d.data(), 20);
	const size_t vl_at = 24 + (size_t)kl0 + 8;  // the first record's valLen
	for (const uint32_t hostile : {0xffffffffu, 0xfffffff0u, 0x80000000u, 0x7fffffffu, (uint32_t)d.size(),
	                               (uint32_t)d.size() - 23, (uint32_t)d.size() - 24}) {
		std::vector<uint8_t> x = d;
		put32(x, 20, hostile);  // key length: the key then runs past the end, or leaves no room for the seq
		const DbScan r = scan_tight(x.data(), x.size());
		CHECK(r.n == 0 && r.ended == SYZSIG_DB_END_TRUNCATED);
		x = d;
		put32(x, vl_at, hostile);  // valLen past the end
		const DbScan v = scan_tight(x.data(), x.size());
		CHECK(v.n == 0 && v.ended == SYZSIG_DB_END_TRUNCATED);
	}
	{  // a valLen that ends exactly at the file's end swallows the later records
		std::vector<uint8_t> x = d;
		put32(x, vl_at, (uint32_t)(d.size() - vl_at - 4));
		const DbScan r = scan_tight(x.data(), x.size());
		CHECK(r.n == 1 && r.ended == SYZSIG_DB_END_EOF);
		put32(x, vl_at, (uint32_t)(d.size() - vl_at - 3));
		CHECK(scan_tight(x.data(), x.size()).n == 0);
	}
	{  // a bad magic at the first record; bad headers
		std::vector<uint8_t> x = d;
		x[16] ^= 1;
		const DbScan r = scan_tight(x.data(), x.size());
		CHECK(r.n == 0 && r.ended == SYZSIG_DB_END_BAD_MAGIC && r.version == whole.version);
		x = d;
		x[0] ^= 1;
		CHECK(scan_tight(x.data(), x.size()).ended == SYZSIG_DB_END_BAD_HEADER);
		for (const uint32_t ver : {0u, 3u, 0xffffffffu}) {
			x = d;
			put32(x, 4, ver);
			const DbScan h = scan_tight(x.data(), x.size());
			CHECK(h.ended == SYZSIG_DB_END_BAD_HEADER && h.n == 0 && h.version == 0);
		}
	}
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

static int run_inflate(const char* path)
{
	std::vector<uint8_t> d;
	if (!read_file(path, d) || d.size() < 8)
		return 2;
	size_t at = 0;
	auto u32 = [&]() {
		const uint32_t v = db_u32(d.data(), at);
		at += 4;
		return v;
	};
	const uint32_t ncases = u32(), max_out = u32();
	for (uint32_t c = 0; c < ncases; c++) {
		if (d.size() - at < 12)
			return 2;
		const uint32_t in_len = u32(), status = u32(), out_len = u32();
		if (d.size() - at < (size_t)in_len + out_len)
			return 2;
		uint8_t* in = in_len ? (uint8_t*)malloc(in_len) : nullptr;
		if (in_len)
			memcpy(in, d.data() + at, in_len);
		const uint8_t* exp = d.data() + at + in_len;
		at += (size_t)in_len + out_len;
		InflateTabArray* t = (InflateTabArray*)malloc(sizeof(InflateTabArray));
		memset(t, 0xEE, sizeof(*t));  // nothing is assumed about the tables' contents
		const InflateResult r = inflate_stream(in, in_len, (uint8_t*)nullptr, 0, max_out, *t);
		if (r.status != status || (status == kInfOk && r.out_len != out_len)) {
			printf("FAIL case %u: status %u (expected %u), length %llu (expected %u)\n", c, r.status, status,
			       (unsigned long long)r.out_len, out_len);
			g_fail++;
		} else if (status == kInfOk) {
			uint8_t* out = out_len ? (uint8_t*)malloc(out_len) : nullptr;
			memset(t, 0x11, sizeof(*t));
			const InflateResult w = inflate_stream(in, in_len, out, out_len, max_out, *t);
			CHECK(w.status == kInfOk && w.out_len == out_len);
			CHECK(w.stored == r.stored && w.fixed == r.fixed && w.dynamic == r.dynamic);
			if (out_len && memcmp(out, exp, out_len)) {
				printf("FAIL case %u: bytes differ\n", c);
				g_fail++;
			}
			if (out_len > 1) {  // an extent one byte short stops the writing decode inside the block
				uint8_t* small = (uint8_t*)malloc(out_len - 1);
				CHECK(inflate_stream(in, in_len, small, out_len - 1, max_out, *t).status == kInfTooLong);
				free(small);
			}
			free(out);
		}
		printf("%u %u %u %u\n", r.status, r.stored, r.fixed, r.dynamic);
		free(t);
		free(in);
	}
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

int main(int argc, char** argv)
{
	if (argc == 2 && !strcmp(argv[1], "args"))
		return run_args();
	if (argc == 3 && !strcmp(argv[1], "scan"))
		return run_scan(argv[2]);
	if (argc == 3 && !strcmp(argv[1], "inflate"))
		return run_inflate(argv[2]);
	return 2;
}
