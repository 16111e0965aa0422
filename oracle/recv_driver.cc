// recv_driver.cc -- the receiver guards of syzkaller_amd/csrc/receiver.h on the
// CPU, under ASan + UBSan (make -C oracle san; tests/test_sanitizers.py).
//
// receiver.h holds no HIP, so it is driven here over stub tables: every set
// the stubs hand out is counted, any stub can be told to fail, and each case
// ends with the live-set count back at its start -- a guard that loses a set
// shows as a failed case and as a leak report, one that frees a set twice or
// touches a freed one as an ASan error.
#include <cstdint>
#include <cstdio>

#include "../include/syzsig.h"

struct syzsig_ctx {
	int unused;
};
struct syzsig_set {
	uint64_t* slots;
	uint64_t nbuckets;
	uint64_t len;
};

static int g_live = 0;
static bool g_fail_alloc = false, g_fail_reserve = false, g_fail_merge_after_alloc = false;

namespace syz {
uint64_t buckets_for(uint64_t n) { return n < 2 ? 2 : n; }
int set_alloc(syzsig_ctx*, uint64_t nbuckets, syzsig_set** out)
{
	if (g_fail_alloc)
		return SYZSIG_ENOMEM;
	*out = new syzsig_set{new uint64_t[nbuckets * 8](), nbuckets, 0};
	g_live++;
	return SYZSIG_OK;
}
int set_reserve(syzsig_set* s, uint64_t extra)
{
	if (g_fail_reserve)
		return SYZSIG_ENOMEM;
	if (s->len + extra > s->nbuckets * 8) {  // grow: new storage, same handle
		delete[] s->slots;
		s->nbuckets = s->len + extra;
		s->slots = new uint64_t[s->nbuckets * 8]();
	}
	return SYZSIG_OK;
}
}  // namespace syz

extern "C" void syzsig_set_free(syzsig_set* s)
{
	if (!s)
		return;
	delete[] s->slots;
	delete s;
	g_live--;
}

// Merge as the library did before it went through Receiver: a nil receiver is
// allocated first, and a failure after that leaves it with the caller.
static int stub_merge(syzsig_ctx* ctx, syzsig_set** sp, uint64_t n)
{
	if (!*sp && syz::set_alloc(ctx, syz::buckets_for(n), sp) != SYZSIG_OK)
		return SYZSIG_ENOMEM;
	if (g_fail_merge_after_alloc)
		return SYZSIG_EIO;
	(*sp)->len += n;
	return SYZSIG_OK;
}
extern "C" int syzsig_merge(syzsig_ctx* ctx, syzsig_set** sp, const syzsig_set* s1)
{
	return s1 && s1->len ? stub_merge(ctx, sp, s1->len) : SYZSIG_OK;
}
extern "C" int syzsig_cover_merge(syzsig_ctx* ctx, syzsig_set** cov, const uint32_t*, uint64_t n)
{
	return stub_merge(ctx, cov, n);
}

#include "../syzkaller_amd/csrc/receiver.h"

using namespace syz;

static int g_failures = 0;
#define CHECK(cond)                                                         \
	do {                                                                    \
		if (!(cond)) {                                                      \
			std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
			g_failures++;                                                   \
		}                                                                   \
	} while (0)

static syzsig_ctx g_ctx;

static syzsig_set* make(uint64_t len)
{
	syzsig_set* s = nullptr;
	set_alloc(&g_ctx, 4, &s);
	s->len = len;
	return s;
}

// an entry point's shape: open, then a launch that fails or not, then the commit
static int entry(syzsig_set** pp, uint64_t extra, bool launch_fails, uint64_t inserted)
{
	Receiver r;
	const int rc = r.open(&g_ctx, pp, extra);
	if (rc != SYZSIG_OK)
		return rc;
	CHECK(r.slots() != nullptr && r.bmask() == r.set()->nbuckets - 1);
	if (launch_fails)
		return SYZSIG_EIO;
	r.commit(inserted);
	return SYZSIG_OK;
}

static void receiver_cases()
{
	const int live0 = g_live;
	// open-nil then failure: nil again, nothing left behind
	syzsig_set* p = nullptr;
	CHECK(entry(&p, 10, true, 0) == SYZSIG_EIO && p == nullptr && g_live == live0);
	// open-nil, the allocation itself fails
	g_fail_alloc = true;
	CHECK(entry(&p, 10, false, 0) == SYZSIG_ENOMEM && p == nullptr && g_live == live0);
	g_fail_alloc = false;
	// open-nil then commit: a set of the right length, the caller's now
	CHECK(entry(&p, 10, false, 7) == SYZSIG_OK && p != nullptr && p->len == 7 && g_live == live0 + 1);
	// open-existing then failure: the handle and the length stay
	syzsig_set* const h = p;
	CHECK(entry(&p, 100, true, 0) == SYZSIG_EIO && p == h && p->len == 7 && g_live == live0 + 1);
	g_fail_reserve = true;
	CHECK(entry(&p, 100, false, 0) == SYZSIG_ENOMEM && p == h && p->len == 7 && g_live == live0 + 1);
	g_fail_reserve = false;
	// open-existing then commit (the reservation grew the table): the handle is kept
	CHECK(entry(&p, 100, false, 5) == SYZSIG_OK && p == h && p->len == 12 && p->nbuckets >= 107 && g_live == live0 + 1);
	{
		// a second commit adds to the length only (a second round of one call)
		Receiver r;
		CHECK(r.open(&g_ctx, &p, 1) == SYZSIG_OK);
		r.commit(1);
		r.commit(2);
		CHECK(p == h && p->len == 15);
	}
	{
		// never opened: nullptr / 0 for the launch, commit and drop do nothing
		Receiver r;
		CHECK(r.set() == nullptr && r.slots() == nullptr && r.bmask() == 0);
		r.commit(3);
		r.drop();
		CHECK(p == h && p->len == 15);
	}
	{
		// drop: a set made here goes at once, an existing one is not touched
		syzsig_set* q = nullptr;
		Receiver a, b;
		CHECK(a.open(&g_ctx, &q, 4) == SYZSIG_OK && g_live == live0 + 2);
		a.drop();
		CHECK(q == nullptr && a.set() == nullptr && g_live == live0 + 1);
		CHECK(b.open(&g_ctx, &p, 4) == SYZSIG_OK);
		b.drop();
		CHECK(p == h && g_live == live0 + 1);
	}
	syzsig_set_free(p);
	CHECK(g_live == live0);
}

// the sequential fallbacks' loop body: merges into working sets that `work` owns
static int loop_body(OwnedSets& work, syzsig_set** sig, syzsig_set** cov, const syzsig_set* src)
{
	int rc = merge_into(&g_ctx, work, sig, src);
	if (rc != SYZSIG_OK)
		return rc;
	return cover_merge_into(&g_ctx, work, cov, nullptr, 3);
}

static void merge_into_cases()
{
	const int live0 = g_live;
	syzsig_set* src = make(5);
	{
		// Merge allocates a nil working set and then fails: the set is registered
		// before the return code is looked at, and freed with `work`
		OwnedSets work;
		syzsig_set *sig = nullptr, *cov = nullptr;
		g_fail_merge_after_alloc = true;
		CHECK(loop_body(work, &sig, &cov, src) == SYZSIG_EIO);
		CHECK(work.sets.size() == 1 && g_live == live0 + 2);
		g_fail_merge_after_alloc = false;
	}
	CHECK(g_live == live0 + 1);
	{
		// the first merge goes through, the cover's allocates and fails
		OwnedSets work;
		syzsig_set *sig = nullptr, *cov = nullptr;
		CHECK(merge_into(&g_ctx, work, &sig, src) == SYZSIG_OK && sig && sig->len == 5);
		g_fail_merge_after_alloc = true;
		CHECK(cover_merge_into(&g_ctx, work, &cov, nullptr, 3) == SYZSIG_EIO);
		g_fail_merge_after_alloc = false;
		CHECK(work.sets.size() == 2 && g_live == live0 + 3);
	}
	CHECK(g_live == live0 + 1);
	{
		// an existing working set (a clone) is registered once, by whoever made it
		OwnedSets work;
		syzsig_set *sig = make(1), *cov = nullptr;
		work.add(sig);
		work.add(nullptr);
		CHECK(loop_body(work, &sig, &cov, src) == SYZSIG_OK);
		CHECK(work.sets.size() == 2 && sig->len == 6 && cov && cov->len == 3);
		// an empty source allocates nothing
		syzsig_set* none = nullptr;
		CHECK(merge_into(&g_ctx, work, &none, nullptr) == SYZSIG_OK && none == nullptr && work.sets.size() == 2);
		// the loop ran to its end: the sets are handed out
		work.release();
		CHECK(work.sets.empty());
		syzsig_set_free(sig);
		syzsig_set_free(cov);
	}
	syzsig_set_free(src);
	CHECK(g_live == live0);
}

static void swap_in_cases()
{
	const int live0 = g_live;
	// nil <- nil
	syzsig_set* dst = nullptr;
	swap_in(&dst, nullptr);
	CHECK(dst == nullptr && g_live == live0);
	// nil <- a set (allocated by a Merge of the loop): the caller gets the set itself
	syzsig_set* c = make(3);
	swap_in(&dst, c);
	CHECK(dst == c && dst->len == 3 && g_live == live0 + 1);
	// a set <- its clone: the handle stays, the contents are the clone's, the old storage is gone
	syzsig_set* const h = dst;
	c = make(9);
	uint64_t* const cslots = c->slots;
	swap_in(&dst, c);
	CHECK(dst == h && dst->len == 9 && dst->slots == cslots && g_live == live0 + 1);
	// a set <- nil (no clone was made): untouched
	swap_in(&dst, nullptr);
	CHECK(dst == h && dst->len == 9 && g_live == live0 + 1);
	syzsig_set_free(dst);
	CHECK(g_live == live0);
}

int main()
{
	receiver_cases();
	merge_into_cases();
	swap_in_cases();
	CHECK(g_live == 0);
	std::printf("%d failures\n", g_failures);
	return g_failures != 0;
}
