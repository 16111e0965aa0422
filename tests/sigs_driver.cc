// sigs_driver.cc -- the host-compilable halves of syzkaller_amd/csrc/sigs.hip on
// the CPU, built under ASan + UBSan by tests/test_hash_ref_cpu.py:
//   sigs_driver args          every branch of csrc/sigs_args.h, the argument
//                             checks of syzsig_hash_dev and the Sig-set entry
//                             points (EINVAL, ERANGE, the NULL-set forms)
//   sigs_driver hash FILE     csrc/sha1.h over the messages of FILE, through both
//                             readers the kernels use; prints one hex Sig per
//                             message for the test to hold against hashlib
// FILE: u32 nmsg, u32 shift, u64 off[nmsg + 1], then off[nmsg] bytes.  Every
// message is hashed from a heap block of exactly its size that starts `(shift +
// off[i]) % 16` bytes into an aligned block, so a load past a message's end is
// an ASan error; then, when the span fits, from a staging array laid out as
// k_hash_wave lays it out, which must give the same Sigs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/syzsig.h"
#include "../syzkaller_amd/csrc/sha1.h"
#include "../syzkaller_amd/csrc/sigs_args.h"

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
	const uint64_t off[2] = {0, 0};
	uint8_t sig[20];
	// syzsig_hash_dev
	CHECK(hash_args(&ctx, nullptr, nullptr, 0, 0, nullptr).code == SYZSIG_OK);  // nmsg = 0 asks for nothing
	CHECK(hash_args(nullptr, &byte, off, 1, 1, sig).code == SYZSIG_EINVAL);
	CHECK(hash_args(&ctx, &byte, nullptr, 1, 1, sig).code == SYZSIG_EINVAL);
	CHECK(hash_args(&ctx, &byte, off, 1, 1, nullptr).code == SYZSIG_EINVAL);
	CHECK(hash_args(&ctx, nullptr, off, 1, 1, sig).code == SYZSIG_EINVAL);
	CHECK(hash_args(&ctx, nullptr, off, 1, 0, sig).code == SYZSIG_OK);  // only empty messages: no data
	CHECK(hash_args(&ctx, &byte, off, 1ull << 32, 1, sig).code == SYZSIG_ERANGE);
	CHECK(hash_args(&ctx, &byte, off, (1ull << 32) - 1, 1, sig).code == SYZSIG_OK);
	CHECK(hash_offsets_status(0, 0).code == SYZSIG_OK);
	CHECK(hash_offsets_status(1, 0).code == SYZSIG_EINVAL);
	CHECK(hash_offsets_status(0, 1).code == SYZSIG_ERANGE);
	CHECK(hash_offsets_status(2, 3).code == SYZSIG_EINVAL);  // a bad offset makes the lengths meaningless
	CHECK(hash_offsets_status(1, 0).msg && hash_offsets_status(0, 1).msg);
	// a batch of Sigs
	CHECK(sigs_batch_args("null", "range", &ctx, nullptr, 0, false).code == SYZSIG_OK);
	CHECK(sigs_batch_args("null", "range", nullptr, sig, 1, true).code == SYZSIG_EINVAL);
	CHECK(sigs_batch_args("null", "range", &ctx, nullptr, 1, true).code == SYZSIG_EINVAL);
	CHECK(sigs_batch_args("null", "range", &ctx, sig, 1, false).code == SYZSIG_EINVAL);
	CHECK(sigs_batch_args("null", "range", &ctx, sig, kSigsMaxBatch, true).code == SYZSIG_OK);
	CHECK(sigs_batch_args("null", "range", &ctx, sig, kSigsMaxBatch + 1, true).code == SYZSIG_ERANGE);
	CHECK(sigs_batch_args("null", "range", &ctx, nullptr, kSigsMaxBatch + 1, false).code == SYZSIG_ERANGE);
	CHECK(!strcmp(sigs_batch_args("null", "range", &ctx, sig, kSigsMaxBatch + 1, true).msg, "range"));
	CHECK(!strcmp(sigs_batch_args("null", "range", &ctx, sig, 1, false).msg, "null"));
	// a set's room; the NULL set is len 0
	CHECK(sigset_room(0, 0).code == SYZSIG_OK);
	CHECK(sigset_room(0, kSigsMaxBatch).code == SYZSIG_OK);
	CHECK(sigset_room(kSigsetMaxLen, 0).code == SYZSIG_OK);
	CHECK(sigset_room(kSigsetMaxLen, 1).code == SYZSIG_ERANGE);
	CHECK(sigset_room(kSigsetMaxLen - kSigsMaxBatch, kSigsMaxBatch).code == SYZSIG_OK);
	// export / Del capacities
	CHECK(sigs_cap(0, 0, nullptr, "null", "range").code == SYZSIG_OK);  // an empty (or NULL) set into nothing
	CHECK(sigs_cap(3, 2, sig, "null", "range").code == SYZSIG_ERANGE);
	CHECK(sigs_cap(3, 2, nullptr, "null", "range").code == SYZSIG_ERANGE);  // the size comes first
	CHECK(sigs_cap(3, 3, nullptr, "null", "range").code == SYZSIG_EINVAL);
	CHECK(sigs_cap(3, 3, sig, "null", "range").code == SYZSIG_OK);
	// the key's byte order is memcmp's, and packing round-trips
	uint8_t a[20], b[20], back[20];
	for (int i = 0; i < 20; i++) {
		memset(a, 0x55, 20);
		memset(b, 0x55, 20);
		b[i] = 0x56;
		uint64_t ka[3], kb[3];
		sig_pack(a, 7, ka);
		sig_pack(b, 3, kb);
		const bool lt = ka[0] != kb[0] ? ka[0] < kb[0] : ka[1] != kb[1] ? ka[1] < kb[1] : ka[2] < kb[2];
		CHECK(lt);
		CHECK((uint32_t)kb[2] == 3);
		sig_unpack(kb, back);
		CHECK(!memcmp(back, b, 20));
	}
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

static void put_hex(const uint32_t (&h)[5])
{
	printf("%08x%08x%08x%08x%08x\n", h[0], h[1], h[2], h[3], h[4]);
}

static int run_hash(const char* path)
{
	FILE* f = fopen(path, "rb");
	if (!f)
		return 2;
	uint32_t hdr[2];
	if (fread(hdr, 4, 2, f) != 2)
		return 2;
	const uint32_t nmsg = hdr[0], shift = hdr[1] & 15;
	std::vector<uint64_t> off(nmsg + 1);
	if (fread(off.data(), 8, nmsg + 1, f) != nmsg + 1)
		return 2;
	std::vector<uint8_t> data(off[nmsg]);
	if (!data.empty() && fread(data.data(), 1, data.size(), f) != data.size())
		return 2;
	fclose(f);
	std::vector<uint32_t> sigs(5 * (size_t)nmsg);
	for (uint32_t i = 0; i < nmsg; i++) {
		const uint64_t len = off[i + 1] - off[i];
		const uint32_t lead = (uint32_t)((shift + off[i]) & 15);
		// (the allocator's blocks are 16-aligned; the block ends where the message ends)
		uint8_t* tight = lead + len ? (uint8_t*)malloc(lead + len) : nullptr;
		if (lead)
			memset(tight, 0xEE, lead);
		if (len)
			memcpy(tight + lead, data.data() + off[i], len);
		uint32_t h[5];
		const Sha1MemReader r = Sha1MemReader::make(tight, lead, len);
		sha1_msg(r, r.shift(), len, h);
		memcpy(&sigs[5 * (size_t)i], h, 20);
		put_hex(h);
		free(tight);
	}
	// the staged form of the whole file as one wave's span
	const uint32_t nwords = SYZSIG_HASH_STAGE / 4 + 4;
	if (off[nmsg] <= SYZSIG_HASH_STAGE) {
		uint32_t* st = (uint32_t*)malloc(nwords * 4);
		memset(st, 0xEE, nwords * 4);
		if (!data.empty())
			memcpy((uint8_t*)st + shift, data.data(), data.size());
		for (uint32_t i = 0; i < nmsg; i++) {
			const uint32_t pos = shift + (uint32_t)off[i];
			uint32_t h[5];
			sha1_msg(Sha1StageReader::make(st, nwords, pos), pos & 3, off[i + 1] - off[i], h);
			CHECK(!memcmp(&sigs[5 * (size_t)i], h, 20));
		}
		free(st);
		printf("staged\n");
	}
	printf("%d failures\n", g_fail);
	return g_fail != 0;
}

int main(int argc, char** argv)
{
	if (argc == 2 && !strcmp(argv[1], "args"))
		return run_args();
	if (argc == 3 && !strcmp(argv[1], "hash"))
		return run_hash(argv[2]);
	return 2;
}
