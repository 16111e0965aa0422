// receiver.h -- the host-side protocol of an entry point that merges into
// `syzsig_set**` receivers which may be nil: sets made by the call are freed
// unless it hands them out, and a receiver is published only by its commit.
//
// No HIP here, so that oracle/recv_driver.cc can drive these guards on the CPU
// over stubs.  Whoever includes this (internal.h; the driver) declares before
// it: syzsig.h's C ABI, a complete `syzsig_set` with `slots`, `nbuckets` and
// `len`, and syz::set_alloc, syz::set_reserve, syz::buckets_for.
//
// FreshNs / commit_run (internal.h) are the triage runs' own guard: a newSignal
// made for a run is kept only when the run changed something, which the run
// learns after its launch.  A Receiver's keep-or-drop is decided by the caller
// before the commit (commit it, or let it go out of scope), so the two do not
// share code.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

namespace syz {

// Sets this call made: freed again unless it release()s them to the caller.
struct OwnedSets {
	std::vector<syzsig_set*> sets;
	OwnedSets() = default;
	OwnedSets(const OwnedSets&) = delete;
	OwnedSets& operator=(const OwnedSets&) = delete;
	~OwnedSets()
	{
		for (syzsig_set* x : sets)
			syzsig_set_free(x);
	}
	void add(syzsig_set* s)  // (nil: nothing to own)
	{
		if (s)
			sets.push_back(s);
	}
	void release() { sets.clear(); }
};

// One `syzsig_set**` that may be nil, from the reservation to the commit.
// Which nil receivers are opened at all is the caller's rule: Signal.Merge
// leaves a nil receiver nil when nothing non-empty reaches it (signal.go:
// 118-125, fuzzer.go:454, :469), Cover.Merge allocates it even for an empty
// cover (cover.go:9-18).  A non-nil receiver keeps its handle.
class Receiver {
	syzsig_set** pp_ = nullptr;
	syzsig_set* s_ = nullptr;
	bool made_ = false;  // s_ was allocated here and is not handed out yet

public:
	Receiver() = default;
	Receiver(const Receiver&) = delete;
	Receiver& operator=(const Receiver&) = delete;
	~Receiver() { drop(); }
	// room for `extra` more entries: in *pp, or in a table made here for a nil *pp
	int open(syzsig_ctx* ctx, syzsig_set** pp, uint64_t extra)
	{
		pp_ = pp;
		s_ = *pp;
		if (s_)
			return set_reserve(s_, extra);  // (a growth keeps the contents and the handle)
		const int rc = set_alloc(ctx, buckets_for(extra), &s_);
		made_ = rc == SYZSIG_OK;
		return rc;
	}
	// for the launch; a receiver that was never opened gives nullptr / 0
	syzsig_set* set() const { return s_; }
	uint64_t* slots() const { return s_ ? s_->slots : nullptr; }
	uint64_t bmask() const { return s_ ? s_->nbuckets - 1 : 0; }
	// the launch went through: the length takes the inserts, the caller the set
	void commit(uint64_t inserted)
	{
		if (!s_)
			return;
		s_->len += inserted;
		*pp_ = s_;
		made_ = false;
	}
	// a set made here and not committed goes away; *pp was never written
	void drop()
	{
		if (made_) {
			syzsig_set_free(s_);
			s_ = nullptr;
			made_ = false;
		}
	}
};

// Signal.Merge / Cover.Merge into a working set `*set` whose sets `owned`
// frees on failure: a receiver that Merge allocated is registered before the
// return code is looked at, so no later early return can lose it.
inline int merge_into(syzsig_ctx* ctx, OwnedSets& owned, syzsig_set** set, const syzsig_set* src)
{
	const bool nil = !*set;
	const int rc = syzsig_merge(ctx, set, src);
	if (nil)
		owned.add(*set);
	return rc;
}

inline int cover_merge_into(syzsig_ctx* ctx, OwnedSets& owned, syzsig_set** set, const uint32_t* raw, uint64_t n)
{
	const bool nil = !*set;
	const int rc = syzsig_cover_merge(ctx, set, raw, n);
	if (nil)
		owned.add(*set);
	return rc;
}

// The end of a sequential fallback that ran on a clone: *dst keeps its handle
// (callers hold it) and takes the clone's contents, the old storage is freed;
// a nil *dst takes the clone itself (nil still, or allocated by a Merge).
// The clone must be out of every OwnedSets by now.  Cannot fail.
inline void swap_in(syzsig_set** dst, syzsig_set* clone)
{
	if (!clone)
		return;
	if (*dst) {
		std::swap(**dst, *clone);
		syzsig_set_free(clone);
	} else {
		*dst = clone;
	}
}

}  // namespace syz
