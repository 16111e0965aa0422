// sigs.hip -- corpus identity on device: pkg/hash over a batch of programs
// (syzsig_hash_dev) and the sets keyed by hash.Sig (syzsig_sigset_*,
// syzsig_number_sigs_dev, syzsig_hub_sync_dev), and on the same sort the
// last-write-wins of pkg/db's replay (syzsig_db_live_dev) and its Save / Delete
// over a batch (syzsig_db_apply_dev, at the end of this file); the rest of
// pkg/db is db.hip.
//
// References:
//   pkg/hash/hash.go:14-26    type Sig [sha1.Size]byte; Hash = sha1 of the pieces
//   syz-fuzzer/fuzzer.go:446-452   addInputToCorpus: sig := hash.Hash(data); a
//       program already in fuzzer.corpusHashes is not appended to fuzzer.corpus
//   syz-manager/manager.go:1110-1113   hubSync's Connect: every corpus Sig into
//       hubCorpus and the Corpus of the HubConnectArgs
//   syz-manager/manager.go:1142-1158   hubSync: Add = corpus \ hubCorpus (then
//       in hubCorpus), Del = hubCorpus \ corpus (then deleted)
//   syz-manager/manager.go:976-1025    NewInput: sig := hash.String(a.Prog) keys
//       mgr.corpus (numberSigs gives syzsig_manager_new_input_batch its keys)
//   pkg/db/db.go:185-200   deserializeDB's loop: a delete (seq == ^0) removes the
//       key, any other record overwrites it
//
// Hashing.  SHA-1 is serial inside a message, so a lane owns a message and a
// wave 64 consecutive ones, whose bytes are one contiguous span of d_data:
//   k_hash_prep   per message: the offsets checked (nothing else runs when one
//                 is bad), the messages longer than kHashLong listed
//   k_hash_wave   one wave per workgroup.  A span of at most kHashStage bytes
//                 is loaded coalesced into LDS -- aligned 16-byte loads, the up
//                 to 15 bytes before the first and after the last aligned chunk
//                 byte by byte -- and each lane reads its message from there; a
//                 longer span is read from global memory directly, each lane its
//                 own 64 bytes per block.  Either way through sha1.h's readers:
//                 aligned words, funnel-shifted by the start's misalignment.
//                 A listed message is skipped: it would hold up its 63
//                 neighbours.
//   k_hash_long   the list, one message per lane, from global memory
// No kernel waits for another wave; every loop is bounded by a block count that
// comes from the offsets, or by the span's length.
//
// Sets.  A syzsig_sigset is its Sigs sorted ascending as memcmp orders them, one
// key of three u64 words each (sha1.h sig_pack): segsort.h's SuU64<3>.  A batch
// is sorted once with its arrival index in the free low half of the third word
// -- k_su_tile_sort and k_su_merge over a one-segment tile table -- so that the
// head of every run of equal Sigs is the Sig's first row:
//   k_sg_pack      Sigs -> keys, and the tile table
//   k_sg_mark      per sorted key: head of its run? in the set (su_bound, a
//                  bounded search)?
//   k_sg_rank      flags -> exclusive ranks, tile by tile over k_su_scan's
//                  offsets of the tiles' counts (count, scan, write)
//   k_sg_compact   the flagged keys, bare, to their ranks
//   k_sg_merge     set and new keys into a new buffer by rank: a key goes to its
//                  index plus the keys of the other list below it (the lists
//                  are disjoint), the bijection of k_su_merge
//   k_sg_last      (db_live) per sorted key: the tail of its run is the key's last
//                  record; it is live unless it is a delete
// Outputs are staged in the workspace and the new buffer is allocated before
// anything of the caller's is written; the set takes the new buffer last.
#include <algorithm>
#include <memory>

#include "segsort.h"
#include "sha1.h"
#include "sigs_args.h"
#include "db_args.h"

struct syzsig_sigset {
	syzsig_ctx* ctx = nullptr;
	uint64_t* recs = nullptr;  // len keys of three words, ascending, low half of the third zero
	uint64_t len = 0;
};

namespace syz {

constexpr uint32_t kHashLong = SYZSIG_HASH_LONG;
constexpr uint32_t kHashStage = SYZSIG_HASH_STAGE;
constexpr uint32_t kHashStageWords = kHashStage / 4 + 4;  // the span may start at byte 15 of its first chunk
constexpr uint32_t kSgTile = SYZSIG_SIGSET_TILE;
constexpr int kHsStaged = kCntInserted, kHsDirect = kCntChanged, kHsLong = kCntTouched, kHsBlocks = kCntCandidates,
              kHsHuge = kCntAux;
static_assert(kHashStage % 16 == 0 && kHashStageWords * 4 <= 64 * 1024, "the staging buffer is static LDS");
static_assert(kSgTile * 24 <= 48 * 1024 && kSgTile % kSuThreads == 0, "a tile of keys in LDS, whole sweeps");

using SgKey = SuU64<3>;
using SgT = SuWords<3>;
using SgTile = SuWordsTile<3, kSgTile>;

// ---- hashing ----

// Per message: its offsets checked; longer than kHashLong: listed.
__global__ __launch_bounds__(256) void k_hash_prep(const uint64_t* __restrict__ off, uint64_t nmsg, uint64_t nbytes,
                                                   uint32_t* list, uint64_t list_cap, unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad = 0, huge = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nmsg; i += T) {
		const uint64_t a = off[i], b = off[i + 1];
		if (a > b || b > nbytes) {
			bad++;
			continue;
		}
		if (b - a > SYZSIG_HASH_MAX_MSG) {
			huge++;
		} else if (b - a > kHashLong) {
			const uint64_t x = atomicAdd(&cnt[kHsLong], 1ull);
			if (x < list_cap)  // (messages past kHashLong bytes inside nbytes: cannot fail for valid offsets)
				list[x] = (uint32_t)i;
		}
	}
	block_count(&cnt[kCntError], bad);
	block_count(&cnt[kHsHuge], huge);
}

// the Sig of message m: the state words big-endian, at any alignment of d_sig
__device__ __forceinline__ void hash_store(uint8_t* sig, uint64_t m, const uint32_t (&h)[5])
{
	uint8_t* p = sig + 20 * m;
	if (((uintptr_t)sig & 3) == 0) {
		uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
		for (int i = 0; i < 5; i++)
			q[i] = __builtin_bswap32(h[i]);
	} else {
#pragma unroll
		for (int i = 0; i < 20; i++)
			p[i] = (uint8_t)(h[i >> 2] >> (24 - 8 * (i & 3)));
	}
}

__global__ __launch_bounds__(64) void k_hash_wave(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                  uint64_t nmsg, uint8_t* sig, bool stage_on, unsigned long long* cnt)
{
	__shared__ uint4 st[kHashStageWords / 4];
	const uint32_t lane = threadIdx.x;
	const uint64_t m0 = (uint64_t)blockIdx.x * 64, m1 = m0 + 64 < nmsg ? m0 + 64 : nmsg, m = m0 + lane;
	const uint64_t lo = off[m0], span = off[m1] - lo;  // (uniform; the offsets passed k_hash_prep)
	const bool staged = stage_on && span <= kHashStage;
	uint64_t a = lo, len = 0;
	if (m < m1) {
		a = off[m];
		len = off[m + 1] - a;
	}
	const bool mine = m < m1 && len <= kHashLong;
	const uintptr_t A = (uintptr_t)data + lo;
	const uint32_t shift = (uint32_t)(A & 15);  // LDS byte j = the byte at A - shift + j
	if (staged && span) {
		uint8_t* st8 = reinterpret_cast<uint8_t*>(st);
		const uintptr_t E = A + span, c0 = (A + 15) & ~(uintptr_t)15, c1 = E & ~(uintptr_t)15;
		for (uintptr_t c = c0 + 16 * lane; c < c1; c += 16 * 64)  // (c0 >= c1: no whole chunk inside the span)
			st[(c - (A - shift)) >> 4] = *reinterpret_cast<const uint4*>(c);
		const uintptr_t he = c0 < E ? c0 : E;                       // head: [A, he), fewer than 16 bytes
		if (A + lane < he)
			st8[shift + lane] = *reinterpret_cast<const uint8_t*>(A + lane);
		const uintptr_t ts = c1 > he ? c1 : he;                     // tail: [ts, E), fewer than 16 bytes
		if (ts + lane < E)
			st8[ts + lane - (A - shift)] = *reinterpret_cast<const uint8_t*>(ts + lane);
	}
	__syncthreads();
	uint64_t nb = 0;
	if (mine) {
		uint32_t h[5];
		if (staged) {
			const uint32_t pos = shift + (uint32_t)(a - lo);
			sha1_msg(Sha1StageReader::make(reinterpret_cast<const uint32_t*>(st), kHashStageWords, pos), pos & 3, len, h);
		} else {
			const Sha1MemReader r = Sha1MemReader::make(data, a, len);
			sha1_msg(r, r.shift(), len, h);
		}
		hash_store(sig, m, h);
		nb = sha1_blocks(len);
	}
	const uint64_t nmine = __popcll(__ballot(mine));
	nb = wave_sum_u64(nb);
	if (lane == 0) {
		if (nmine)
			atomicAdd(&cnt[staged ? kHsStaged : kHsDirect], (unsigned long long)nmine);
		if (nb)
			atomicAdd(&cnt[kHsBlocks], (unsigned long long)nb);
	}
}

__global__ __launch_bounds__(64) void k_hash_long(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                  const uint32_t* __restrict__ list, uint64_t nlong, uint8_t* sig,
                                                  unsigned long long* cnt)
{
	const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
	uint64_t nb = 0;
	if (i < nlong) {
		const uint64_t m = list[i], a = off[m], len = off[m + 1] - a;
		uint32_t h[5];
		const Sha1MemReader r = Sha1MemReader::make(data, a, len);
		sha1_msg(r, r.shift(), len, h);
		hash_store(sig, m, h);
		nb = sha1_blocks(len);
	}
	nb = wave_sum_u64(nb);
	if (threadIdx.x == 0 && nb)
		atomicAdd(&cnt[kHsBlocks], (unsigned long long)nb);
}

// ---- sets of Sigs ----

__device__ __forceinline__ SgT sg_load(const uint8_t* __restrict__ sig, uint64_t i, uint32_t low)
{
	uint64_t w[3];
	sig_pack(sig + 20 * i, low, w);
	return SgT{{w[0], w[1], w[2]}};
}

__device__ __forceinline__ void sg_store(uint8_t* sig, uint64_t i, const SgT& x)
{
	const uint64_t w[3] = {x.w[0], x.w[1], x.w[2]};
	sig_unpack(w, sig + 20 * i);
}

__device__ __forceinline__ SgT sg_bare(SgT x)
{
	x.w[2] &= ~0xFFFFFFFFull;
	return x;
}

__device__ __forceinline__ uint32_t sg_row(const SgT& x) { return (uint32_t)x.w[2]; }

__device__ __forceinline__ bool sg_same(const SgT& a, const SgT& b)
{
	return a.w[0] == b.w[0] && a.w[1] == b.w[1] && (a.w[2] >> 32) == (b.w[2] >> 32);
}

// The first of the sorted keys p[0 .. n) that carries x's Sig (any low halves), or n.
__device__ __forceinline__ uint64_t sg_find(const uint64_t* __restrict__ p, uint64_t n, const SgT& x)
{
	if (n == 0)
		return 0;
	const SgT b = sg_bare(x);
	const uint64_t pos = su_bound<SgKey, false>(p, 0, n, b);
	return pos < n && sg_same(SgKey::get(p, pos), b) ? pos : n;
}

// the sum of x over the threads below this one, and over the workgroup (uniform); every thread calls it
__device__ __forceinline__ uint32_t sg_block_scan(uint32_t x, uint32_t& total)
{
	__shared__ uint32_t s_w[kSuThreads / 64];
	const uint32_t w = threadIdx.x >> 6, incl = wave_incl_scan(x);
	__syncthreads();  // the last call's sums are read
	if (lane_id() == 63)
		s_w[w] = incl;
	__syncthreads();
	uint32_t wb = 0;
	total = 0;
#pragma unroll
	for (uint32_t k = 0; k < kSuThreads / 64; k++) {
		wb += k < w ? s_w[k] : 0;
		total += s_w[k];
	}
	return wb + incl - x;
}

// the one-segment tile table of a batch of n keys in ntiles tiles
struct SgTable {
	uint64_t* base;       // [1] = 0
	uint64_t* src_start;  // [1] = 0
	uint32_t* len;        // [1] = n
	uint32_t* owner;      // [ntiles] = 0
	uint32_t* idx;        // [ntiles] = the tile
};

__global__ __launch_bounds__(256) void k_sg_pack(const uint8_t* __restrict__ sig, uint64_t n, uint64_t* keys,
                                                 SgTable t, uint64_t ntiles)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x, i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (uint64_t i = i0; i < n; i += T)
		SgKey::put(keys, i, sg_load(sig, i, (uint32_t)i));
	for (uint64_t i = i0; i < ntiles; i += T) {
		t.owner[i] = 0;
		t.idx[i] = (uint32_t)i;
	}
	if (i0 == 0) {
		*t.base = 0;
		*t.src_start = 0;
		*t.len = (uint32_t)n;
	}
}

// Per sorted key j of the batch: head[j] = it is the first row of its Sig;
// fresh[j] = ... and the Sig is not in the set; row_fresh[its row] = fresh.
// Each of the three outputs may be nullptr.
__global__ __launch_bounds__(256) void k_sg_mark(const uint64_t* __restrict__ b, uint64_t n,
                                                 const uint64_t* __restrict__ set, uint64_t m, uint32_t* head,
                                                 uint32_t* fresh, uint8_t* row_fresh)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T) {
		const SgT x = SgKey::get(b, j);
		const bool hd = j == 0 || !sg_same(x, SgKey::get(b, j - 1));
		const bool fr = hd && sg_find(set, m, x) == m;
		if (head)
			head[j] = hd;
		if (fresh)
			fresh[j] = fr;
		if (row_fresh)
			row_fresh[sg_row(x)] = fr;
	}
}

// absent[i] = key i of the set has its Sig nowhere in the sorted batch
__global__ __launch_bounds__(256) void k_sg_absent(const uint64_t* __restrict__ set, uint64_t m,
                                                   const uint64_t* __restrict__ b, uint64_t n, uint32_t* absent)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += T)
		absent[i] = sg_find(b, n, SgKey::get(set, i)) == n;
}

// Tile t of the flags f[0 .. n): kCount: its sum to tcnt[t]; else r[i] = toff[t] + the flags before i in the tile.
template <bool kCount>
__global__ __launch_bounds__(kSuThreads) void k_sg_rank(const uint32_t* __restrict__ f, uint64_t n, uint64_t ntiles,
                                                        uint32_t* tcnt, const uint64_t* __restrict__ toff, uint32_t* r)
{
	for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		uint32_t run = kCount ? 0 : (uint32_t)toff[t];
		for (uint32_t s = 0; s < kSgTile; s += kSuThreads) {
			const uint64_t i = t * kSgTile + s + threadIdx.x;
			const uint32_t x = i < n ? f[i] : 0;
			uint32_t total;
			const uint32_t before = sg_block_scan(x, total);
			if (!kCount && i < n)
				r[i] = run + before;
			run += total;
		}
		if (kCount && threadIdx.x == 0)
			tcnt[t] = run;
	}
}

// the flagged keys of b, bare, to out[their rank]
__global__ __launch_bounds__(256) void k_sg_compact(const uint64_t* __restrict__ b, uint64_t n,
                                                    const uint32_t* __restrict__ f, const uint32_t* __restrict__ r,
                                                    uint64_t* out)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T)
		if (f[j])
			SgKey::put(out, r[j], sg_bare(SgKey::get(b, j)));
}

// the flagged keys of b as Sigs to sig[20 * their rank ..]
__global__ __launch_bounds__(256) void k_sg_export(const uint64_t* __restrict__ b, uint64_t n,
                                                   const uint32_t* __restrict__ f, const uint32_t* __restrict__ r,
                                                   uint8_t* sig)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T)
		if (!f || f[j])
			sg_store(sig, f ? r[j] : j, SgKey::get(b, j));
}

// The sorted, disjoint key lists a[0 .. na) and b[0 .. nb) merged into out by
// rank: a key's place is its index plus the keys of the other list below it.
__global__ __launch_bounds__(256) void k_sg_merge(const uint64_t* __restrict__ a, uint64_t na,
                                                  const uint64_t* __restrict__ b, uint64_t nb, uint64_t* out)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += T) {
		const bool left = i < na;
		const uint64_t li = left ? i : i - na;
		const SgT x = SgKey::get(left ? a : b, li);
		SgKey::put(out, li + (left ? su_bound<SgKey, false>(b, 0, nb, x) : su_bound<SgKey, false>(a, 0, na, x)), x);
	}
}

__global__ __launch_bounds__(256) void k_sg_contains(const uint8_t* __restrict__ sig, uint64_t n,
                                                     const uint64_t* __restrict__ set, uint64_t m, uint8_t* in)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T)
		in[i] = sg_find(set, m, sg_load(sig, i, 0)) != m;
}

// first_row[r] = 1 for the first row r of every distinct Sig (first_row zeroed)
__global__ __launch_bounds__(256) void k_sg_heads(const uint64_t* __restrict__ b, uint64_t n, uint32_t* first_row)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T) {
		const SgT x = SgKey::get(b, j);
		if (j == 0 || !sg_same(x, SgKey::get(b, j - 1)))
			first_row[sg_row(x)] = 1;
	}
}

// numberSigs: a row's key = the rank of its Sig's first row among the first rows
__global__ __launch_bounds__(256) void k_sg_number(const uint64_t* __restrict__ b, uint64_t n,
                                                   const uint32_t* __restrict__ row_rank,
                                                   const uint64_t* __restrict__ known, uint64_t m, uint32_t* key,
                                                   uint32_t* first, uint8_t* is_known)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T) {
		const SgT x = SgKey::get(b, j);
		const uint64_t hp = sg_find(b, n, x);  // the head of x's run (<= j)
		const uint32_t hrow = sg_row(SgKey::get(b, hp < n ? hp : j)), k = row_rank[hrow];
		key[sg_row(x)] = k;
		if (hp == j) {
			first[k] = hrow;
			is_known[k] = sg_find(known, m, x) != m;
		}
	}
}

// live[row] = 1 for the last row of every distinct Sig unless its seq is `deleted`, else 0: every
// row of the batch is written once.  The live rows are counted into *cnt.
__global__ __launch_bounds__(256) void k_sg_last(const uint64_t* __restrict__ b, uint64_t n,
                                                 const uint64_t* __restrict__ seq, uint64_t deleted, uint8_t* live,
                                                 unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t k = 0;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T) {
		const SgT x = SgKey::get(b, j);
		const uint32_t row = sg_row(x);
		const bool lv = (j + 1 == n || !sg_same(x, SgKey::get(b, j + 1))) && seq[row] != deleted;
		live[row] = lv;
		k += lv;
	}
	block_count(cnt, k);
}

// ---- host ----

struct SgWork {
	uint32_t *f0, *f1, *r0, *r1, *tcnt;
	uint64_t* toff;
	SgTable tab;
};

// the arrays of a call over L flags and a batch of nt sort tiles, carved from `p` (nullptr: sizing); returns the bytes
static size_t sg_carve(char* p, uint64_t L, uint64_t nt, SgWork* w)
{
	size_t o = 0;
	auto take = [&](size_t bytes) {
		char* r = p ? p + o : nullptr;
		o += align256(bytes + 8);
		return r;
	};
	const uint64_t lt = L / kSgTile + 1;
	w->f0 = (uint32_t*)take(L * 4);
	w->f1 = (uint32_t*)take(L * 4);
	w->r0 = (uint32_t*)take(L * 4);
	w->r1 = (uint32_t*)take(L * 4);
	w->tcnt = (uint32_t*)take(lt * 4);
	w->toff = (uint64_t*)take((lt + 1) * 8);
	w->tab.base = (uint64_t*)take(8);
	w->tab.src_start = (uint64_t*)take(8);
	w->tab.len = (uint32_t*)take(4);
	w->tab.owner = (uint32_t*)take((nt + 1) * 4);
	w->tab.idx = (uint32_t*)take((nt + 1) * 4);
	return o;
}

static int sg_work(syzsig_ctx* ctx, uint64_t L, uint64_t n, SgWork* w)
{
	const uint64_t nt = (n + kSgTile - 1) / kSgTile;
	char* p;
	SYZ_TRY(ws_get(ctx, kWsSgMeta, sg_carve(nullptr, L, nt, w), (void**)&p));
	sg_carve(p, L, nt, w);
	return SYZSIG_OK;
}

// The n keys packed into bb, with w's tile table, sorted through ba: *sorted, and *spare = the other buffer.
static int sg_sort_packed(syzsig_ctx* ctx, uint64_t n, const SgWork& w, uint64_t* ba, uint64_t* bb,
                          const uint64_t** sorted, uint64_t** spare = nullptr)
{
	const hipStream_t s = ctx->stream;
	const uint64_t nt = (n + kSgTile - 1) / kSgTile;
	const SuSegs S{bb, 3, w.tab.src_start, w.tab.len, 1, w.tab.len, 1};
	const SuTiles T{nullptr, w.tab.base, w.tab.len, w.tab.owner, w.tab.idx, 1, nt};
	uint64_t *src = ba, *dst = bb;
	k_su_tile_sort<SgTile><<<grid_cap(nt), kSuThreads, 0, s>>>(S, T, src, nullptr);
	for (uint64_t width = kSgTile; width < n; width <<= 1) {
		k_su_merge<SgKey, kSgTile><<<grid_cap(nt), kSuThreads, 0, s>>>(T, width, src, dst, nullptr);
		std::swap(src, dst);
	}
	SYZ_HIP(hipGetLastError());
	*sorted = src;
	if (spare)
		*spare = dst;
	return SYZSIG_OK;
}

// The batch's keys (Sig, row) sorted: *sorted; *spare = the other buffer, n keys of room.  Enqueues only.
static int sg_sort(syzsig_ctx* ctx, const uint8_t* d_sig, uint64_t n, const SgWork& w, const uint64_t** sorted,
                   uint64_t** spare)
{
	const hipStream_t s = ctx->stream;
	const uint64_t nt = (n + kSgTile - 1) / kSgTile;
	void *ba, *bb;
	SYZ_TRY(ws_get(ctx, kWsSgBufA, n * 24 + 256, &ba));
	SYZ_TRY(ws_get(ctx, kWsSgBufB, n * 24 + 256, &bb));
	k_sg_pack<<<grid_for(std::max(n, nt), 256), 256, 0, s>>>(d_sig, n, (uint64_t*)bb, w.tab, nt);
	return sg_sort_packed(ctx, n, w, (uint64_t*)ba, (uint64_t*)bb, sorted, spare);
}

// r[i] = the set flags of f before i; *total = all of them.  Synchronizes.
static int sg_rank(syzsig_ctx* ctx, const uint32_t* f, uint64_t n, const SgWork& w, uint32_t* r, uint64_t* total)
{
	const hipStream_t s = ctx->stream;
	*total = 0;
	if (n == 0)
		return SYZSIG_OK;
	const uint64_t lt = (n + kSgTile - 1) / kSgTile;
	k_sg_rank<true><<<grid_cap(lt, 4096), kSuThreads, 0, s>>>(f, n, lt, w.tcnt, nullptr, nullptr);
	k_su_scan<<<1, kSuThreads, 0, s>>>(w.tcnt, lt, w.toff);
	k_sg_rank<false><<<grid_cap(lt, 4096), kSuThreads, 0, s>>>(f, n, lt, nullptr, w.toff, r);
	SYZ_HIP(hipGetLastError());
	SYZ_HIP(hipMemcpyAsync(total, w.toff + lt, 8, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipStreamSynchronize(s));
	return SYZSIG_OK;
}

// device memory this call allocated: freed again unless the set takes it
struct DevBuf {
	void* p = nullptr;
	hipStream_t s;
	explicit DevBuf(hipStream_t st) : s(st) {}
	DevBuf(const DevBuf&) = delete;
	~DevBuf()
	{
		if (p)
			(void)hipFreeAsync(p, s);
	}
	int alloc(uint64_t keys)
	{
		if (keys)
			SYZ_HIP(hipMallocAsync(&p, keys * 24, s));
		return SYZSIG_OK;
	}
	uint64_t* release() { return (uint64_t*)std::exchange(p, nullptr); }
};

static int arg_fail(const ArgStatus& a) { return fail(a.code, a.msg); }

#define SYZ_ARGS(expr)                                                             \
	do {                                                                           \
		const syz::ArgStatus a__ = (expr);                                         \
		if (a__.code != SYZSIG_OK)                                                 \
			return syz::arg_fail(a__);                                             \
	} while (0)

// the set takes the buffer `recs` of `len` keys; a nil *pp takes the set made for the call
static void sg_commit(syzsig_sigset** pp, std::unique_ptr<syzsig_sigset>& made, syzsig_ctx* ctx, uint64_t* recs,
                      uint64_t len)
{
	syzsig_sigset* set = *pp ? *pp : made.release();
	if (set->recs)
		(void)hipFreeAsync(set->recs, ctx->stream);
	set->recs = recs;
	set->len = len;
	*pp = set;
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_hash_dev(syzsig_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off, uint64_t nmsg,
                               uint64_t nbytes, uint8_t* d_sig)
{
	SYZ_LOCK(ctx);
	SYZ_ARGS(hash_args(ctx, d_data, d_off, nmsg, nbytes, d_sig));
	std::fill(ctx->hs_stats, ctx->hs_stats + 4, 0);
	if (nmsg == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	const uint64_t list_cap = std::min<uint64_t>(nmsg, nbytes / (kHashLong + 1)) + 1;
	uint32_t* list;
	SYZ_TRY(ws_get(ctx, kWsHashList, list_cap * 4, (void**)&list));
	SYZ_TRY(counters_reset(ctx));
	SYZ_TRY(su_time_begin(ctx));
	k_hash_prep<<<grid_for(nmsg, 256), 256, 0, s>>>(d_off, nmsg, nbytes, list, list_cap, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	SYZ_ARGS(hash_offsets_status(ctx->h_cnt[kCntError], ctx->h_cnt[kHsHuge]));
	const uint64_t nlong = ctx->h_cnt[kHsLong];
	if (nlong >= list_cap)
		return fail(SYZSIG_EIO, "hash: internal: more long messages than nbytes holds");
	k_hash_wave<<<(unsigned)((nmsg + 63) / 64), 64, 0, s>>>(d_data, d_off, nmsg, d_sig, ctx->hash_stage, ctx->d_cnt);
	if (nlong)
		k_hash_long<<<(unsigned)((nlong + 63) / 64), 64, 0, s>>>(d_data, d_off, list, nlong, d_sig, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_TRY(counters_fetch(ctx));
	ctx->hs_stats[0] = ctx->h_cnt[kHsStaged];
	ctx->hs_stats[1] = ctx->h_cnt[kHsDirect];
	ctx->hs_stats[2] = nlong;
	ctx->hs_stats[3] = ctx->h_cnt[kHsBlocks];
	return SYZSIG_OK;
}

extern "C" int syzsig_hash_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::hs_stats, out, "hash_stats");
}

extern "C" int syzsig_sigset_make(syzsig_ctx* ctx, syzsig_sigset** out)
{
	SYZ_LOCK(ctx);
	if (!ctx || !out)
		return fail(SYZSIG_EINVAL, "sigset_make: NULL argument");
	*out = new syzsig_sigset();
	(*out)->ctx = ctx;
	return SYZSIG_OK;
}

extern "C" void syzsig_sigset_free(syzsig_sigset* s)
{
	if (!s)
		return;
	{
		SYZ_LOCK(s->ctx);
		if (s->recs)
			(void)hipFreeAsync(s->recs, s->ctx->stream);
	}
	delete s;
}

extern "C" uint64_t syzsig_sigset_len(const syzsig_sigset* s) { return s ? s->len : 0; }

extern "C" int syzsig_sigset_add_dev(syzsig_ctx* ctx, syzsig_sigset** sp, const uint8_t* d_sig, uint64_t n,
                                     uint8_t* d_is_new)
{
	SYZ_LOCK(ctx);
	SYZ_ARGS(sigs_batch_args("sigset_add: NULL argument", "sigset_add: more than 2^25 Sigs in one call", ctx, d_sig, n,
	                         d_is_new != nullptr));
	if (!sp || (*sp && (*sp)->ctx != ctx))
		return fail(SYZSIG_EINVAL, "sigset_add: NULL receiver, or a set of another context");
	const uint64_t m = *sp ? (*sp)->len : 0;
	SYZ_ARGS(sigset_room(m, n));
	if (n == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	const uint64_t* set = *sp ? (*sp)->recs : nullptr;
	SgWork w;
	uint8_t* row_new;
	SYZ_TRY(sg_work(ctx, n, n, &w));
	SYZ_TRY(ws_get(ctx, kWsSgOut, n + 256, (void**)&row_new));
	const uint64_t* b;
	uint64_t *spare, k;
	SYZ_TRY(su_time_begin(ctx));
	SYZ_TRY(sg_sort(ctx, d_sig, n, w, &b, &spare));
	k_sg_mark<<<grid_for(n, 256), 256, 0, s>>>(b, n, set, m, nullptr, w.f0, row_new);
	SYZ_TRY(sg_rank(ctx, w.f0, n, w, w.r0, &k));
	DevBuf nb(s);
	std::unique_ptr<syzsig_sigset> made;
	if (k) {  // (else the set is what it was)
		SYZ_TRY(nb.alloc(m + k));
		if (!*sp) {
			made.reset(new syzsig_sigset());
			made->ctx = ctx;
		}
		k_sg_compact<<<grid_for(n, 256), 256, 0, s>>>(b, n, w.f0, w.r0, spare);
		k_sg_merge<<<grid_for(m + k, 256), 256, 0, s>>>(set, m, spare, k, (uint64_t*)nb.p);
	}
	SYZ_HIP(hipMemcpyAsync(d_is_new, row_new, n, hipMemcpyDeviceToDevice, s));
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(su_time_end(ctx));
	SYZ_HIP(hipStreamSynchronize(s));
	if (k)
		sg_commit(sp, made, ctx, nb.release(), m + k);
	return SYZSIG_OK;
}

extern "C" int syzsig_sigset_contains_dev(syzsig_ctx* ctx, const syzsig_sigset* set, const uint8_t* d_sig, uint64_t n,
                                          uint8_t* d_in)
{
	SYZ_LOCK(ctx);
	SYZ_ARGS(sigs_batch_args("sigset_contains: NULL argument", "sigset_contains: more than 2^25 Sigs in one call", ctx,
	                         d_sig, n, d_in != nullptr));
	if (set && set->ctx != ctx)
		return fail(SYZSIG_EINVAL, "sigset_contains: a set of another context");
	if (n == 0)
		return SYZSIG_OK;
	k_sg_contains<<<grid_for(n, 256), 256, 0, ctx->stream>>>(d_sig, n, set ? set->recs : nullptr, set ? set->len : 0,
	                                                        d_in);
	SYZ_HIP(hipGetLastError());
	SYZ_HIP(hipStreamSynchronize(ctx->stream));
	return SYZSIG_OK;
}

extern "C" int syzsig_sigset_export_dev(syzsig_ctx* ctx, const syzsig_sigset* set, uint8_t* d_sig, uint64_t cap,
                                        uint64_t* n_out)
{
	SYZ_LOCK(ctx);
	if (n_out)
		*n_out = 0;
	if (!ctx || !n_out || (set && set->ctx != ctx))
		return fail(SYZSIG_EINVAL, "sigset_export: NULL argument, or a set of another context");
	const uint64_t m = set ? set->len : 0;
	*n_out = m;
	SYZ_ARGS(sigs_cap(m, cap, d_sig, "sigset_export: NULL output", "sigset_export: the set holds more than cap Sigs"));
	if (m == 0)
		return SYZSIG_OK;
	k_sg_export<<<grid_for(m, 256), 256, 0, ctx->stream>>>(set->recs, m, nullptr, nullptr, d_sig);
	SYZ_HIP(hipGetLastError());
	SYZ_HIP(hipStreamSynchronize(ctx->stream));
	return SYZSIG_OK;
}

extern "C" int syzsig_number_sigs_dev(syzsig_ctx* ctx, const syzsig_sigset* known, const uint8_t* d_sig, uint64_t n,
                                      uint32_t* d_key, uint32_t* d_first, uint8_t* d_known, uint64_t* nkeys)
{
	SYZ_LOCK(ctx);
	if (nkeys)
		*nkeys = 0;
	SYZ_ARGS(sigs_batch_args("number_sigs: NULL argument", "number_sigs: more than 2^25 Sigs in one call", ctx, d_sig, n,
	                         d_key && d_first && d_known));
	if (!nkeys || (known && known->ctx != ctx))
		return fail(SYZSIG_EINVAL, "number_sigs: NULL argument, or a set of another context");
	if (n == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	SgWork w;
	SYZ_TRY(sg_work(ctx, n, n, &w));
	const uint64_t* b;
	uint64_t *spare, K;
	SYZ_TRY(sg_sort(ctx, d_sig, n, w, &b, &spare));
	SYZ_HIP(hipMemsetAsync(w.f0, 0, n * 4, s));
	k_sg_heads<<<grid_for(n, 256), 256, 0, s>>>(b, n, w.f0);
	SYZ_TRY(sg_rank(ctx, w.f0, n, w, w.r0, &K));
	k_sg_number<<<grid_for(n, 256), 256, 0, s>>>(b, n, w.r0, known ? known->recs : nullptr, known ? known->len : 0,
	                                             d_key, d_first, d_known);
	SYZ_HIP(hipGetLastError());
	SYZ_HIP(hipStreamSynchronize(s));
	*nkeys = K;
	return SYZSIG_OK;
}

extern "C" int syzsig_hub_sync_dev(syzsig_ctx* ctx, syzsig_sigset** hub, const uint8_t* d_sig, uint64_t n,
                                   uint8_t* d_add, uint8_t* d_del_sig, uint64_t del_cap, uint64_t* ndel)
{
	SYZ_LOCK(ctx);
	if (ndel)
		*ndel = 0;
	SYZ_ARGS(sigs_batch_args("hub_sync: NULL argument", "hub_sync: more than 2^25 Sigs in one call", ctx, d_sig, n,
	                         d_add != nullptr));
	if (!hub || !ndel || (*hub && (*hub)->ctx != ctx))
		return fail(SYZSIG_EINVAL, "hub_sync: NULL argument, or a set of another context");
	const uint64_t m = *hub ? (*hub)->len : 0;
	if (n == 0 && m == 0)
		return SYZSIG_OK;  // (a nil hubCorpus stays nil)
	const hipStream_t s = ctx->stream;
	const uint64_t* set = *hub ? (*hub)->recs : nullptr;
	SgWork w;
	uint8_t* row_add = nullptr;
	SYZ_TRY(sg_work(ctx, std::max(n, m), n, &w));
	SYZ_TRY(ws_get(ctx, kWsSgOut, n + 256, (void**)&row_add));
	const uint64_t* b = nullptr;
	uint64_t *spare = nullptr, distinct = 0, nd = 0;
	if (n) {
		SYZ_TRY(sg_sort(ctx, d_sig, n, w, &b, &spare));
		k_sg_mark<<<grid_for(n, 256), 256, 0, s>>>(b, n, set, m, w.f1, nullptr, row_add);
		SYZ_TRY(sg_rank(ctx, w.f1, n, w, w.r1, &distinct));
	}
	if (m) {
		k_sg_absent<<<grid_for(m, 256), 256, 0, s>>>(set, m, b, n, w.f0);
		SYZ_TRY(sg_rank(ctx, w.f0, m, w, w.r0, &nd));
	}
	*ndel = nd;
	SYZ_ARGS(sigs_cap(nd, del_cap, d_del_sig, "hub_sync: NULL output", "hub_sync: more deleted Sigs than del_cap"));
	DevBuf nb(s);
	std::unique_ptr<syzsig_sigset> made;
	SYZ_TRY(nb.alloc(distinct));
	if (!*hub) {
		made.reset(new syzsig_sigset());
		made->ctx = ctx;
	}
	if (n) {
		k_sg_compact<<<grid_for(n, 256), 256, 0, s>>>(b, n, w.f1, w.r1, (uint64_t*)nb.p);
		SYZ_HIP(hipMemcpyAsync(d_add, row_add, n, hipMemcpyDeviceToDevice, s));
	}
	if (nd)
		k_sg_export<<<grid_for(m, 256), 256, 0, s>>>(set, m, w.f0, w.r0, d_del_sig);
	SYZ_HIP(hipGetLastError());
	SYZ_HIP(hipStreamSynchronize(s));
	sg_commit(hub, made, ctx, nb.release(), distinct);
	return SYZSIG_OK;
}

extern "C" int syzsig_db_live_dev(syzsig_ctx* ctx, const uint8_t* d_sig, const uint64_t* d_seq, uint64_t n,
                                  uint64_t nvalid, uint8_t* d_live, uint64_t* nlive, uint64_t* uncompacted)
{
	SYZ_LOCK(ctx);
	if (nlive)
		*nlive = 0;
	if (uncompacted)
		*uncompacted = 0;
	SYZ_ARGS(db_live_args(ctx, d_sig, d_seq, n, nvalid, d_live, nlive, uncompacted));
	if (n == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	uint8_t* row_live;
	SYZ_TRY(ws_get(ctx, kWsSgOut, n + 256, (void**)&row_live));
	SYZ_TRY(counters_reset(ctx));
	SYZ_HIP(hipMemsetAsync(row_live, 0, n, s));  // (the rows from nvalid on)
	if (nvalid) {
		SgWork w;
		SYZ_TRY(sg_work(ctx, nvalid, nvalid, &w));
		const uint64_t* b;
		uint64_t* spare;
		SYZ_TRY(sg_sort(ctx, d_sig, nvalid, w, &b, &spare));
		k_sg_last<<<grid_for(nvalid, 256), 256, 0, s>>>(b, nvalid, d_seq, kDbSeqDeleted, row_live,
		                                                &ctx->d_cnt[kCntInserted]);
		SYZ_HIP(hipGetLastError());
	}
	SYZ_TRY(counters_fetch(ctx));
	SYZ_HIP(hipMemcpyAsync(d_live, row_live, n, hipMemcpyDeviceToDevice, s));
	SYZ_HIP(hipStreamSynchronize(s));
	*nlive = ctx->h_cnt[kCntInserted];
	*uncompacted = nvalid;
	return SYZSIG_OK;
}

// ---- Save and Delete over a batch (pkg/db/db.go:55-74) ----
//
// The rows are the nl live records, then the m ops: row r < nl is live record
// r, row nl + j is op j.  Sorted by (Sig, row), a run holds a key's rows in the
// order the reference would have met them, and what an op sees is what the row
// before it in the run left -- whether or not that row was itself a no-op.
//   k_ap_check    the two offset arrays, the deletes' values, the live seqs
//   k_ap_pack     k_sg_pack over the two Sig arrays
//   k_ap_written  per sorted row: does it reach the log (a live record does by
//                 definition)?  A Save is compared with its predecessor byte by
//                 byte only where seq and length agree
//   k_ap_keep     per sorted row that is written and no delete: is every later
//                 row of its run a no-op?  Then it is the key's record.

namespace syz {

struct ApRows {
	const uint64_t *lseq, *loff, *oseq, *ooff;
	const uint8_t *ldata, *odata;
	uint64_t nl;
	__device__ __forceinline__ uint64_t seq(uint64_t r) const { return r < nl ? lseq[r] : oseq[r - nl]; }
	__device__ __forceinline__ const uint8_t* val(uint64_t r, uint64_t& len) const
	{
		const uint64_t* off = r < nl ? loff + r : ooff + (r - nl);
		len = off[1] - off[0];
		return (r < nl ? ldata : odata) + off[0];
	}
};

__global__ __launch_bounds__(256) void k_ap_check(ApRows R, uint64_t m, uint64_t lbytes, uint64_t obytes,
                                                  unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t bad = 0, delv = 0, ldel = 0;
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R.nl + m; r += T) {
		const bool live = r < R.nl;
		const uint64_t* off = live ? R.loff + r : R.ooff + (r - R.nl);
		const uint64_t a = off[0], b = off[1];
		if (a > b || b > (live ? lbytes : obytes))
			bad++;
		else if (R.seq(r) != kDbSeqDeleted)
			continue;
		else if (live)
			ldel++;
		else
			delv += b != a;
	}
	block_count(&cnt[kCntError], bad);
	block_count(&cnt[kCntAux], delv);
	block_count(&cnt[kCntTouched], ldel);
}

__global__ __launch_bounds__(256) void k_ap_pack(const uint8_t* __restrict__ lsig, uint64_t nl,
                                                 const uint8_t* __restrict__ osig, uint64_t n, uint64_t* keys, SgTable t,
                                                 uint64_t ntiles)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x, i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (uint64_t i = i0; i < n; i += T)
		SgKey::put(keys, i, i < nl ? sg_load(lsig, i, (uint32_t)i) : sg_load(osig, i - nl, (uint32_t)i));
	for (uint64_t i = i0; i < ntiles; i += T) {
		t.owner[i] = 0;
		t.idx[i] = (uint32_t)i;
	}
	if (i0 == 0) {
		*t.base = 0;
		*t.src_start = 0;
		*t.len = (uint32_t)n;
	}
}

// wr[j] = sorted row j reaches the log (or is a live record); row_written[op] for the ops
__global__ __launch_bounds__(256) void k_ap_written(const uint64_t* __restrict__ b, uint64_t n, ApRows R, uint32_t* wr,
                                                    uint8_t* row_written, unsigned long long* cnt)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t k = 0;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T) {
		const SgT x = SgKey::get(b, j);
		const uint64_t r = sg_row(x);
		if (r < R.nl) {
			wr[j] = 1;
			continue;
		}
		const uint64_t sq = R.seq(r);
		bool present = false;
		uint64_t p = 0;
		if (j > 0) {
			const SgT y = SgKey::get(b, j - 1);
			p = sg_row(y);
			present = sg_same(x, y) && R.seq(p) != kDbSeqDeleted;
		}
		bool w;
		if (sq == kDbSeqDeleted) {
			w = present;  // db.go:68-70
		} else {
			w = true;
			if (present && R.seq(p) == sq) {  // db.go:59-61
				uint64_t la, lb;
				const uint8_t *va = R.val(p, la), *vb = R.val(r, lb);
				if (la == lb) {
					uint64_t i = 0;
					while (i < la && va[i] == vb[i])
						i++;
					w = i < la;
				}
			}
		}
		wr[j] = w;
		row_written[r - R.nl] = w;
		k += w;
	}
	block_count(cnt, k);
}

// keep[row] = 1 iff the row is written, no delete, and every later row of its run is a no-op
__global__ __launch_bounds__(256) void k_ap_keep(const uint64_t* __restrict__ b, uint64_t n, ApRows R,
                                                 const uint32_t* __restrict__ wr, uint8_t* row_keep,
                                                 unsigned long long* cnt_live, unsigned long long* cnt_op)
{
	const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
	uint64_t kl = 0, ko = 0;
	for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += T) {
		const SgT x = SgKey::get(b, j);
		const uint64_t r = sg_row(x);
		bool keep = wr[j] && R.seq(r) != kDbSeqDeleted;
		for (uint64_t q = j + 1; keep && q < n && sg_same(x, SgKey::get(b, q)); q++)
			keep = !wr[q];
		row_keep[r] = keep;
		(r < R.nl ? kl : ko) += keep;
	}
	block_count(cnt_live, kl);
	block_count(cnt_op, ko);
}

}  // namespace syz

extern "C" int syzsig_db_apply_dev(syzsig_ctx* ctx, const uint8_t* d_live_sig, const uint64_t* d_live_seq, uint64_t nl,
                                   const uint8_t* d_live_data, uint64_t live_bytes, const uint64_t* d_live_off,
                                   const uint8_t* d_op_sig, const uint64_t* d_op_seq, uint64_t m,
                                   const uint8_t* d_op_data, uint64_t op_bytes, const uint64_t* d_op_off,
                                   uint8_t* d_written, uint8_t* d_keep_live, uint8_t* d_keep_op, uint64_t* nwritten,
                                   uint64_t* nkeep_live, uint64_t* nkeep_op)
{
	SYZ_LOCK(ctx);
	for (uint64_t* c : {nwritten, nkeep_live, nkeep_op})
		if (c)
			*c = 0;
	SYZ_ARGS(db_apply_args(ctx, d_live_sig, d_live_seq, nl, d_live_data, live_bytes, d_live_off, d_op_sig, d_op_seq, m,
	                       d_op_data, op_bytes, d_op_off, d_written, d_keep_live, d_keep_op, nwritten, nkeep_live,
	                       nkeep_op));
	const uint64_t n = nl + m;
	if (n == 0)
		return SYZSIG_OK;
	const hipStream_t s = ctx->stream;
	const ApRows R{d_live_seq, d_live_off, d_op_seq, d_op_off, d_live_data, d_op_data, nl};
	SYZ_TRY(counters_reset(ctx));
	k_ap_check<<<grid_for(n, 256), 256, 0, s>>>(R, m, live_bytes, op_bytes, ctx->d_cnt);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	SYZ_ARGS(db_apply_status(ctx->h_cnt[kCntError], ctx->h_cnt[kCntAux], ctx->h_cnt[kCntTouched]));
	uint8_t* stage;  // row_keep[n], then row_written[m]: held back until nothing can fail
	SYZ_TRY(ws_get(ctx, kWsSgOut, n + m + 512, (void**)&stage));
	uint8_t *row_keep = stage, *row_written = stage + align256(n);
	SgWork w;
	SYZ_TRY(sg_work(ctx, n, n, &w));
	const uint64_t nt = (n + kSgTile - 1) / kSgTile;
	void *ba, *bb;
	SYZ_TRY(ws_get(ctx, kWsSgBufA, n * 24 + 256, &ba));
	SYZ_TRY(ws_get(ctx, kWsSgBufB, n * 24 + 256, &bb));
	SYZ_TRY(counters_reset(ctx));
	k_ap_pack<<<grid_for(std::max(n, nt), 256), 256, 0, s>>>(d_live_sig, nl, d_op_sig, n, (uint64_t*)bb, w.tab, nt);
	const uint64_t* b;
	SYZ_TRY(sg_sort_packed(ctx, n, w, (uint64_t*)ba, (uint64_t*)bb, &b));
	k_ap_written<<<grid_for(n, 256), 256, 0, s>>>(b, n, R, w.f0, row_written, &ctx->d_cnt[kCntInserted]);
	k_ap_keep<<<grid_for(n, 256), 256, 0, s>>>(b, n, R, w.f0, row_keep, &ctx->d_cnt[kCntChanged],
	                                           &ctx->d_cnt[kCntCandidates]);
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (nl)
		SYZ_HIP(hipMemcpyAsync(d_keep_live, row_keep, nl, hipMemcpyDeviceToDevice, s));
	if (m) {
		SYZ_HIP(hipMemcpyAsync(d_keep_op, row_keep + nl, m, hipMemcpyDeviceToDevice, s));
		SYZ_HIP(hipMemcpyAsync(d_written, row_written, m, hipMemcpyDeviceToDevice, s));
	}
	SYZ_HIP(hipStreamSynchronize(s));
	*nwritten = ctx->h_cnt[kCntInserted];
	*nkeep_live = ctx->h_cnt[kCntChanged];
	*nkeep_op = ctx->h_cnt[kCntCandidates];
	return SYZSIG_OK;
}
