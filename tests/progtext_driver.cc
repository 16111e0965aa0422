// progtext_driver.cc -- the host-compilable halves of syzkaller_amd/csrc/calls.hip
// on the CPU, built under ASan + UBSan by tests/test_progtext_ref_cpu.py:
//   progtext_driver args        every branch of csrc/calls_args.h: the entry points'
//                               argument checks and the name table's build
//   progtext_driver cases FILE  csrc/calls_core.h over the cases of FILE: u32 nnames,
//                               per name u32 len + bytes; u32 ncases, per case u32
//                               len + the program's bytes, then for Deserialize and
//                               for CallSet mode u32 status, err_line, flag, nids
//                               and the ids.  Each program lives in a heap block of
//                               exactly its size, so one byte read past either end
//                               is an ASan report.  Every line is also scanned
//                               through every shorter window: the answer is "more"
//                               or the full window's answer, never another.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/syzsig.h"
#include "../syzkaller_amd/csrc/calls_args.h"

using namespace syz;

static int g_fail = 0;
#define CHECK(c)                                                    \
	do {                                                            \
		if (!(c)) {                                                 \
			printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
			g_fail++;                                               \
		}                                                           \
	} while (0)

struct HostSrc {
	const uint8_t* p;
	uint64_t end, lim;
	int byte(uint64_t q) const { return p[q]; }
	bool ends_before(uint64_t q) const { return q >= end; }
};

static int run_args()
{
	int ctx = 0, tab = 0;
	alignas(16) const uint8_t text[32] = {0};
	const uint64_t off[2] = {0, 1};
	uint64_t coff[2], total = 0;
	uint32_t ids[1], el[1];
	uint8_t st[1], fl[1];
	void* out = nullptr;
	// syzsig_calltab_make
	const uint8_t names[] = "abcab";
	const uint64_t no[4] = {0, 1, 3, 5};  // a, bc, ab
	CHECK(calltab_args(&ctx, names, no, 3, &out).code == SYZSIG_OK);
	CHECK(calltab_args(nullptr, names, no, 3, &out).code == SYZSIG_EINVAL);
	CHECK(calltab_args(&ctx, nullptr, no, 3, &out).code == SYZSIG_EINVAL);
	CHECK(calltab_args(&ctx, names, nullptr, 3, &out).code == SYZSIG_EINVAL);
	CHECK(calltab_args(&ctx, names, no, 3, nullptr).code == SYZSIG_EINVAL);
	CHECK(calltab_args(&ctx, names, no, 0, &out).code == SYZSIG_EINVAL);
	CHECK(calltab_args(&ctx, names, no, kCallTabMaxNames, &out).code == SYZSIG_OK);
	CHECK(calltab_args(&ctx, names, no, kCallTabMaxNames + 1, &out).code == SYZSIG_ERANGE);
	std::vector<CallSlot> slots;
	CHECK(calltab_build(names, no, 3, slots).code == SYZSIG_OK && slots.size() == 8);
	CHECK(calltab_slots_for(1) == 2 && calltab_slots_for(4) == 8 && calltab_slots_for(5) == 16);
	{
		const uint64_t no2[3] = {0, 2, 2};  // an empty name
		CHECK(calltab_build(names, no2, 2, slots).code == SYZSIG_EINVAL);
		const uint64_t no3[4] = {0, 2, 3, 5};  // ab, c, ab: a duplicate
		CHECK(calltab_build(names, no3, 3, slots).code == SYZSIG_EINVAL);
		const uint64_t no4[3] = {0, 3, 2};  // the offsets decrease
		CHECK(calltab_build(names, no4, 2, slots).code == SYZSIG_EINVAL);
		const uint64_t no5[2] = {1, 2};  // do not start at 0
		CHECK(calltab_build(names, no5, 1, slots).code == SYZSIG_EINVAL);
	}
	{  // lookups on the host: every name, a prefix, an extension, the empty span
		CHECK(calltab_build(names, no, 3, slots).code == SYZSIG_OK);
		const CallTabView T{slots.data(), slots.size() - 1, names, no, 3};
		const HostBytes B{names};
		CHECK(calltab_find(T, B, 0, 1) == 0 && calltab_find(T, B, 1, 3) == 1 && calltab_find(T, B, 3, 5) == 2);
		CHECK(calltab_find(T, B, 0, 2) == 2);  // "ab" again, from other bytes
		CHECK(calltab_find(T, B, 1, 2) == kNoCall && calltab_find(T, B, 0, 3) == kNoCall);
		CHECK(calltab_find(T, B, 2, 2) == kNoCall);
	}
	// syzsig_prog_calls_dev
#define PC(c, t, d, nb, o, np, mode, co, id, cap, s, e, f, tot) \
	prog_calls_args(c, t, d, nb, o, np, mode, co, id, cap, s, e, f, tot).code
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_OK);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 1, coff, ids, 1, st, el, fl, &total) == SYZSIG_OK);
	CHECK(PC(nullptr, &tab, text, 1, off, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, nullptr, text, 1, off, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 2, coff, ids, 1, st, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, nullptr, 1, off, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, nullptr, 0, off, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_OK);
	CHECK(PC(&ctx, &tab, text + 1, 1, off, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_EINVAL);  // alignment
	CHECK(PC(&ctx, &tab, text, 1, nullptr, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, nullptr, ids, 1, st, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, coff, nullptr, 0, st, el, fl, &total) == SYZSIG_OK);  // sizing
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, coff, nullptr, 1, st, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, coff, ids, 1, nullptr, el, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, coff, ids, 1, st, nullptr, fl, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, coff, ids, 1, st, el, nullptr, &total) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, text, 1, off, 1, 0, coff, ids, 1, st, el, fl, nullptr) == SYZSIG_EINVAL);
	CHECK(PC(&ctx, &tab, nullptr, 0, nullptr, 0, 0, coff, nullptr, 0, nullptr, nullptr, nullptr, &total) == SYZSIG_OK);
	CHECK(PC(&ctx, &tab, text, 1, off, kProgCallsMaxBatch + 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_ERANGE);
	CHECK(PC(&ctx, &tab, text, kProgCallsMaxBytes + 1, off, 1, 0, coff, ids, 1, st, el, fl, &total) == SYZSIG_ERANGE);
#undef PC
	CHECK(prog_calls_offsets_status(0).code == SYZSIG_OK && prog_calls_offsets_status(1).code == SYZSIG_EINVAL);
	CHECK(prog_calls_room(10, 10, false).code == SYZSIG_OK && prog_calls_room(10, 9, false).code == SYZSIG_ERANGE);
	CHECK(prog_calls_room(10, 0, true).code == SYZSIG_OK && prog_calls_room(1ull << 32, ~0ull, true).code == SYZSIG_ERANGE);
	CHECK(prog_calls_long_cap(0) == 2 && prog_calls_long_cap(255 * 4) == 6);
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

struct Result {
	uint32_t status = 0, err_line = 0, flag = 0;
	std::vector<uint32_t> ids;
};

// the sequential walk over one program's lines with calls_core.h's rules
static Result walk(const uint8_t* p, uint64_t n, uint32_t mode, const CallTabView& T)
{
	Result r;
	bool unknown = false, any = false;
	uint32_t line = 0;
	for (uint64_t pos = 0; pos < n;) {
		line++;
		uint64_t e = pos;
		while (e < n && p[e] != '\n')
			e++;
		uint32_t rec;
		if (e - pos >= kPtMaxLine) {
			rec = kRecErr | SYZSIG_PT_LINE_TOO_LONG;
		} else {
			const HostSrc S{p, n, ~0ull};
			rec = line_record(S, pos, mode, T);
			// every shorter window says "more" or the same
			const Head full = head_scan(S, pos, mode);
			for (uint64_t lim = pos; lim <= e + 1 && lim <= pos + 300; lim++) {
				const HostSrc W{p, n, lim};
				const Head h = head_scan(W, pos, mode);
				if (h.kind != kHdMore &&
				    (h.kind != full.kind || h.status != full.status || h.lo != full.lo || h.hi != full.hi)) {
					printf("FAIL window %llu of line at %llu\n", (unsigned long long)lim, (unsigned long long)pos);
					g_fail++;
				}
			}
			CHECK(full.kind != kHdMore);
		}
		const uint32_t kind = rec & kRecKindMask;
		if (kind == kRecErr || kind == kRecPending) {
			r.status = kind == kRecErr ? (rec & kRecValMask) : 255;
			r.err_line = line;
			r.ids.clear();
			return r;
		}
		any = any || kind == kRecCall || kind == kRecUnknown;
		unknown = unknown || kind == kRecUnknown;
		if (kind == kRecCall)
			r.ids.push_back(rec & kRecValMask);
		pos = e < n ? e + 1 : n;
	}
	if (mode == SYZSIG_PROGTEXT_CALLSET) {
		if (!any) {
			r.status = SYZSIG_PT_NO_CALLS;
			return r;
		}
		std::sort(r.ids.begin(), r.ids.end());
		r.ids.erase(std::unique(r.ids.begin(), r.ids.end()), r.ids.end());
		r.flag = (unknown ? 2u : 1u);
	}
	return r;
}

static int run_cases(const char* path)
{
	FILE* f = fopen(path, "rb");
	if (!f)
		return 2;
	std::vector<uint8_t> d;
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;)
		d.insert(d.end(), buf, buf + k);
	fclose(f);
	size_t at = 0;
	auto u32 = [&]() {
		uint32_t v = 0;
		if (d.size() - at >= 4)
			memcpy(&v, d.data() + at, 4);
		at += 4;
		return v;
	};
	const uint32_t nnames = u32();
	std::vector<uint8_t> names;
	std::vector<uint64_t> no{0};
	for (uint32_t i = 0; i < nnames; i++) {
		const uint32_t l = u32();
		names.insert(names.end(), d.begin() + at, d.begin() + at + l);
		at += l;
		no.push_back(names.size());
	}
	std::vector<CallSlot> slots;
	CHECK(calltab_build(names.data(), no.data(), nnames, slots).code == SYZSIG_OK);
	const CallTabView T{slots.data(), slots.size() - 1, names.data(), no.data(), nnames};
	const uint32_t ncases = u32();
	for (uint32_t c = 0; c < ncases; c++) {
		const uint32_t len = u32();
		uint8_t* prog = len ? (uint8_t*)malloc(len) : nullptr;
		if (len)
			memcpy(prog, d.data() + at, len);
		at += len;
		for (uint32_t mode = 0; mode < 2; mode++) {
			const uint32_t status = u32(), err_line = u32(), flag = u32(), nids = u32();
			const Result r = walk(prog, len, mode, T);
			bool ok = r.status == status && r.err_line == err_line && r.flag == flag && r.ids.size() == nids;
			for (uint32_t k = 0; k < nids; k++) {
				const uint32_t id = u32();
				ok = ok && k < r.ids.size() && r.ids[k] == id;
			}
			if (!ok) {
				printf("FAIL case %u mode %u: status %u (expected %u), line %u (%u), flag %u (%u), %zu ids (%u)\n", c,
				       mode, r.status, status, r.err_line, err_line, r.flag, flag, r.ids.size(), nids);
				g_fail++;
			}
		}
		free(prog);
	}
	CHECK(at == d.size());
	printf("%u cases\n%d failures\n", ncases, g_fail);
	return g_fail != 0;
}

int main(int argc, char** argv)
{
	if (argc == 2 && !strcmp(argv[1], "args"))
		return run_args();
	if (argc == 3 && !strcmp(argv[1], "cases"))
		return run_cases(argv[2]);
	return 2;
}
