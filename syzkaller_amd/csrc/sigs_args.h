// sigs_args.h -- the host-side argument checks of sigs.hip's entry points: what
// is rejected before any device work, and how the counters of the offsets check
// become a status.  No HIP here, so that tests/sigs_driver.cc runs every branch
// on the CPU under ASan + UBSan.  Whoever includes this has syzsig.h's codes.
#pragma once

#include <cstdint>

namespace syz {

constexpr uint64_t kSigsMaxBatch = 1ull << 25;     // rows of one call, as hint_mutants
constexpr uint64_t kSigsetMaxLen = (1ull << 32) - 2;  // a set's ranks and binary searches are 32-bit

struct ArgStatus {
	int code;  // SYZSIG_OK: go on
	const char* msg;
};

inline ArgStatus arg_ok() { return ArgStatus{SYZSIG_OK, nullptr}; }

// syzsig_hash_dev before the offsets are looked at (they are device memory)
inline ArgStatus hash_args(const void* ctx, const uint8_t* d_data, const uint64_t* d_off, uint64_t nmsg,
                           uint64_t nbytes, const uint8_t* d_sig)
{
	if (!ctx)
		return ArgStatus{SYZSIG_EINVAL, "hash: NULL context"};
	if (nmsg && (!d_off || !d_sig || (nbytes && !d_data)))
		return ArgStatus{SYZSIG_EINVAL, "hash: NULL argument"};
	if (nmsg >= 1ull << 32)
		return ArgStatus{SYZSIG_ERANGE, "hash: 2^32 or more messages"};
	return arg_ok();
}

// ... and after: `bad` offsets that decrease or pass nbytes, `huge` messages past SYZSIG_HASH_MAX_MSG
inline ArgStatus hash_offsets_status(uint64_t bad, uint64_t huge)
{
	if (bad)
		return ArgStatus{SYZSIG_EINVAL, "hash: the offsets decrease or pass nbytes"};
	if (huge)
		return ArgStatus{SYZSIG_ERANGE, "hash: a message is longer than SYZSIG_HASH_MAX_MSG"};
	return arg_ok();
}

// the entry points over a batch of n Sigs: `outs_ok` = every output of n entries is given
inline ArgStatus sigs_batch_args(const char* who_null, const char* who_range, const void* ctx, const uint8_t* d_sig,
                                 uint64_t n, bool outs_ok)
{
	if (!ctx)
		return ArgStatus{SYZSIG_EINVAL, who_null};
	if (n > kSigsMaxBatch)
		return ArgStatus{SYZSIG_ERANGE, who_range};
	if (n && (!d_sig || !outs_ok))
		return ArgStatus{SYZSIG_EINVAL, who_null};
	return arg_ok();
}

// a set of `len` Sigs that takes up to n more
inline ArgStatus sigset_room(uint64_t len, uint64_t n)
{
	if (len + n > kSigsetMaxLen)
		return ArgStatus{SYZSIG_ERANGE, "sigset: more than 2^32 - 2 Sigs"};
	return arg_ok();
}

// a result of `need` entries into a buffer of `cap`
inline ArgStatus sigs_cap(uint64_t need, uint64_t cap, const void* buf, const char* who_null, const char* who_range)
{
	if (need > cap)
		return ArgStatus{SYZSIG_ERANGE, who_range};
	if (need && !buf)
		return ArgStatus{SYZSIG_EINVAL, who_null};
	return arg_ok();
}

}  // namespace syz
