// calls_args.h -- the host-side half of calls.hip: what its entry points reject
// before any device work, and the call-name table as it is built on the host
// (syzsig_calltab_make's body).  No HIP here, so that tests/progtext_driver.cc
// runs every branch on the CPU under ASan + UBSan.  Whoever includes this has
// syzsig.h's codes.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "calls_core.h"
#include "sigs_args.h"

namespace syz {

constexpr uint64_t kCallTabMaxNames = 1ull << 24;  // an id fits a line record with room to spare
constexpr uint64_t kCallTabMaxBytes = 1ull << 32;
constexpr uint64_t kProgCallsMaxBatch = 1ull << 25;  // programs of one call, as a batch of Sigs
constexpr uint64_t kProgCallsMaxBytes = 1ull << 40;

struct HostBytes {
	const uint8_t* p;
	int byte(uint64_t q) const { return p[q]; }
};

inline ArgStatus calltab_args(const void* ctx, const uint8_t* names, const uint64_t* name_off, uint64_t n,
                              const void* out)
{
	if (!ctx || !out)
		return ArgStatus{SYZSIG_EINVAL, "calltab_make: NULL argument"};
	if (n == 0)
		return ArgStatus{SYZSIG_EINVAL, "calltab_make: no names"};
	if (n > kCallTabMaxNames)
		return ArgStatus{SYZSIG_ERANGE, "calltab_make: more than 2^24 names"};
	if (!names || !name_off)
		return ArgStatus{SYZSIG_EINVAL, "calltab_make: NULL argument"};
	return arg_ok();
}

inline uint64_t calltab_slots_for(uint64_t n)
{
	uint64_t s = 2;
	while (s < 2 * n)
		s <<= 1;
	return s;
}

// The table of names[name_off[i] .. name_off[i + 1]), i < n, in id order: linear
// probing from calltab_home.  An empty name, a duplicate, offsets that decrease
// or do not start at 0: SYZSIG_EINVAL, slots unspecified.
inline ArgStatus calltab_build(const uint8_t* names, const uint64_t* name_off, uint64_t n,
                               std::vector<CallSlot>& slots)
{
	if (name_off[0] != 0)
		return ArgStatus{SYZSIG_EINVAL, "calltab_make: name_off[0] is not 0"};
	for (uint64_t i = 0; i < n; i++) {
		if (name_off[i + 1] < name_off[i])
			return ArgStatus{SYZSIG_EINVAL, "calltab_make: the offsets decrease"};
		if (name_off[i + 1] == name_off[i])
			return ArgStatus{SYZSIG_EINVAL, "calltab_make: an empty name"};
		if (name_off[i + 1] - name_off[i] > 0xffffffffull)
			return ArgStatus{SYZSIG_ERANGE, "calltab_make: a name of 2^32 bytes or more"};
	}
	if (name_off[n] > kCallTabMaxBytes)
		return ArgStatus{SYZSIG_ERANGE, "calltab_make: more than 2^32 bytes of names"};
	const uint64_t mask = calltab_slots_for(n) - 1;
	CallSlot empty;
	empty.hash = 0;
	empty.id = kNoCall;
	empty.len = 0;
	slots.assign(mask + 1, empty);
	const HostBytes B{names};
	for (uint64_t i = 0; i < n; i++) {
		const uint64_t lo = name_off[i], len = name_off[i + 1] - lo;
		const uint64_t h = name_hash(B, lo, lo + len);
		uint64_t s = calltab_home(h, mask);
		while (slots[s].id != kNoCall) {  // (n < nslots: an empty slot exists)
			const CallSlot& e = slots[s];
			if (e.hash == h && e.len == len && !memcmp(names + name_off[e.id], names + lo, len))
				return ArgStatus{SYZSIG_EINVAL, "calltab_make: a duplicate name"};
			s = (s + 1) & mask;
		}
		slots[s].hash = h;
		slots[s].id = (uint32_t)i;
		slots[s].len = (uint32_t)len;
	}
	return arg_ok();
}

// syzsig_prog_calls_dev before the offsets are looked at (they are device memory)
inline ArgStatus prog_calls_args(const void* ctx, const void* tab, const uint8_t* d_data, uint64_t nbytes,
                                 const uint64_t* d_off, uint64_t nprog, uint32_t mode, const uint64_t* d_call_off,
                                 const uint32_t* d_call_id, uint64_t cap, const uint8_t* d_status,
                                 const uint32_t* d_err_line, const uint8_t* d_flag, const uint64_t* total)
{
	if (!ctx)
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: NULL context"};
	if (!tab)
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: NULL table"};
	if (mode != SYZSIG_PROGTEXT_DESERIALIZE && mode != SYZSIG_PROGTEXT_CALLSET)
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: mode is neither DESERIALIZE nor CALLSET"};
	if (!total || !d_call_off)
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: NULL argument"};
	if (nprog > kProgCallsMaxBatch)
		return ArgStatus{SYZSIG_ERANGE, "prog_calls: more than 2^25 programs in one call"};
	if (nbytes > kProgCallsMaxBytes)
		return ArgStatus{SYZSIG_ERANGE, "prog_calls: more than 2^40 bytes of text"};
	if (nprog && (!d_off || !d_status || !d_err_line || !d_flag || (nbytes && !d_data)))
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: NULL argument"};
	if ((uintptr_t)d_data & 15)
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: d_data is not 16-byte aligned"};
	if (!d_call_id && cap)
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: NULL output with a capacity"};
	return arg_ok();
}

// ... and after: `bad` offsets that decrease or pass nbytes
inline ArgStatus prog_calls_offsets_status(uint64_t bad)
{
	if (bad)
		return ArgStatus{SYZSIG_EINVAL, "prog_calls: the offsets decrease or pass nbytes"};
	return arg_ok();
}

// ... and once the total is known.  sizing = a NULL d_call_id: everything but the ids.
inline ArgStatus prog_calls_room(uint64_t total, uint64_t cap, bool sizing)
{
	if (total >= 1ull << 32)
		return ArgStatus{SYZSIG_ERANGE, "prog_calls: 2^32 or more calls"};
	if (!sizing && total > cap)
		return ArgStatus{SYZSIG_ERANGE, "prog_calls: more calls than cap"};
	return arg_ok();
}

// the most lines that can be left undecided by a window of W bytes: each has at least W - 1 bytes
inline uint64_t prog_calls_long_cap(uint64_t nbytes) { return nbytes / (SYZSIG_PROGTEXT_WINDOW - 1) + 2; }

}  // namespace syz
