// corpus.hip -- syz-manager/manager.go:976-1025 Manager.NewInput over a batch
// of inputs, on device.
//
// Reference, per input i (in arrival order, under mgr.mu):
//   inputSignal := a.Signal.Deserialize()            (a later duplicate wins)
//   if corpusSignal.Diff(inputSignal).Empty() return                  (:993)
//   corpusSignal.Merge(inputSignal); corpusCover.Merge(a.Cover)       (:997-998)
//   if inp, ok := corpus[sig]; ok { inp.Signal = max-merge; inp.Cover = union }
//   else { corpus[sig] = a.RPCInput; ... }                            (:1000-1022)
//
// Batch restatement.  For element e let p_i(e) be the prio of the last entry
// of e in input i's Serial, C0 corpusSignal before the batch.  A rejected
// input has p_j(e) <= corpusSignal[e] for each of its e, so merging it would
// change nothing and the running maximum may run over all earlier inputs:
// input i is accepted  <=>  some e has p_i(e) > max(C0[e], p_j(e) for every
// j < i carrying e) -- Poll's event rule (poll.hip) with M0 = C0.  The final
// corpusSignal is the max-merge of the events, the final corpusCover the union
// of the accepted inputs' covers, and key k's entry the max-merge (union) of
// the Deserialized Signals (covers) of k's old entry -- a row flagged
// SYZSIG_INPUT_PRESENT -- and k's accepted inputs.
//
// Acceptance:
//   k_ni_rows / rp_group   the non-PRESENT entries, e << 32 | entry index,
//                          grouped by element through the LDS partitions of
//                          recs.hip
//   k_ni_walk              segsort.h's su_sort_walk, as k_poll_part_walk: one
//                          workgroup per partition sorts its entries by
//                          (element, entry index) in LDS, one thread per element
//                          run emits the events; here an event also marks its
//                          row accepted (read-only on corpusSignal)
//   k_ni_commit            corpusSignal.Merge of the events and, flagged by
//                          `accepted`, every accepted row's cover into
//                          corpusCover -- one launch, after every allocation
//   ni_accept_sequential   the reference loop over the set ops on clones, for a
//                          batch past 2^23 entries or a partition past
//                          kRpCap; swapped in only at the end
// Per-key merge (both paths): each touched key's rows laid consecutively in
// arrival order (host), then
//   k_ni_gather            keys elem << 32 | index-in-group, and per entry its
//                          row and prio
//   k_su_tile_sort, k_su_merge   segsort.h's tile sort (tiles of kNiTile keys)
//                          and rank-merge passes over a tile table built on the
//                          host; keys are distinct
//   k_ni_reduce            one workgroup per group streams its sorted keys: per
//                          run of one element, per row the last entry
//                          (Deserialize), the max over rows (Merge), block scan,
//                          compacted write
//   k_su_gather            the groups' results packed into the CSR output
// and the covers through cover.hip's instance of the segmented sort-unique
// (syzsig_triage_cover_dev, one run per group).  No device atomic per entry;
// every loop is bounded by a group, run or tile length known at launch.
#include <algorithm>
#include <chrono>
#include <vector>

#include "segsort.h"

namespace syz {

constexpr uint64_t kNiMaxEntries = 1ull << 23;  // entries of one batched acceptance (the element partitions' capacity)
constexpr uint32_t kNiTile = SYZSIG_CORPUS_TILE;
constexpr uint32_t kNiThreads = kSuThreads;
constexpr uint64_t kNiMaxGrid = 1u << 16;
constexpr int kNiCovIns = kCntAux2;  // PCs new to corpusCover (kCntInserted counts corpusSignal's)
static_assert((kNiTile & (kNiTile - 1)) == 0 && kNiTile >= 2 && kNiTile * 8 <= 64 * 1024, "tile: a power of two in LDS");
using NiTile = SuWordsTile<1, kNiTile>;

// Acceptance row j (a non-PRESENT row) owns the entries src[j] .. + len[j] of
// the uploaded Serials; they become the compact entries dst[j] ..: x = e << 32 |
// compact index for rp_group, with the entry's row and prio beside it.
__global__ __launch_bounds__(kNiThreads) void k_ni_rows(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                        const uint32_t* __restrict__ len,
                                                        const uint32_t* __restrict__ row, uint32_t nrows,
                                                        const uint32_t* __restrict__ elems,
                                                        const int8_t* __restrict__ prios, uint64_t* x,
                                                        uint32_t* rec_row, int8_t* rec_prio)
{
	for (uint32_t j = blockIdx.x; j < nrows; j += gridDim.x) {
		const uint64_t s = src[j], d = dst[j];
		const uint32_t n = len[j], r = row[j];
		for (uint32_t t = threadIdx.x; t < n; t += kNiThreads) {
			x[d + t] = ((uint64_t)elems[s + t] << 32) | (d + t);
			rec_row[d + t] = r;
			rec_prio[d + t] = prios[s + t];
		}
	}
}

// su_sort_walk over the acceptance entries: an event marks its row accepted
// (every writer stores the same 1).  Read-only on corpusSignal (cs == nullptr:
// a nil corpusSignal); the events are committed by k_ni_commit.
__global__ __launch_bounds__(kNiThreads) void k_ni_walk(const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ base, uint32_t pbits,
                                                        const uint32_t* __restrict__ rec_row,
                                                        const int8_t* __restrict__ rec_prio, const uint64_t* cs,
                                                        uint64_t cs_bmask, uint64_t* ev, uint64_t ev_cap,
                                                        unsigned long long* nev, uint8_t* accepted,
                                                        const unsigned long long* ctr)
{
	su_sort_walk(keys, base, pbits, rec_row, rec_prio, cs, cs_bmask, ev, ev_cap, nev, ctr,
	             [&](uint32_t e, uint32_t row, int pr) {
		             accepted[row] = 1;
		             return ((uint64_t)e << 32) | prio_biased((int8_t)pr);
	             });
}

// The commit, one launch: workgroups [0, ev_blocks) max-merge the events into
// corpusSignal (an element's last event carries its final max), the others
// take the rows -- a non-PRESENT row flagged accepted inserts its cover into
// corpusCover.
__global__ __launch_bounds__(kNiThreads) void k_ni_commit(const uint64_t* __restrict__ ev, uint64_t nev, uint32_t ev_blocks,
                                                          uint64_t* cs, uint64_t cs_bmask,
                                                          const uint8_t* __restrict__ accepted,
                                                          const uint8_t* __restrict__ flags,
                                                          const uint64_t* __restrict__ cover_off, uint32_t nrows,
                                                          const uint32_t* __restrict__ cover, uint64_t* cv,
                                                          uint64_t cv_bmask, unsigned long long* ctr)
{
	uint64_t ins = 0, cins = 0, ovf = 0;
	if (blockIdx.x < ev_blocks) {
		merge_events(ev, nev, blockIdx.x * (uint64_t)kNiThreads + threadIdx.x, (uint64_t)ev_blocks * kNiThreads, cs,
		             cs_bmask, ins, ovf);
	} else {
		const uint32_t rb = gridDim.x - ev_blocks;  // (cover_off is relative to the uploaded covers)
		for (uint32_t i = blockIdx.x - ev_blocks; i < nrows; i += rb) {
			if ((flags[i] & SYZSIG_INPUT_PRESENT) || !accepted[i])
				continue;
			for (uint64_t c = cover_off[i] + threadIdx.x; c < cover_off[i + 1]; c += kNiThreads) {
				const int rr = tbl_merge(cv, cv_bmask, cover[c], 0);
				cins += rr == 1;
				ovf += rr < 0;
			}
		}
	}
	block_count(&ctr[kCntInserted], ins);
	block_count(&ctr[kNiCovIns], cins);
	block_count(&ctr[kCntOverflow], ovf);
}

// ---- the per-key merge ----

// Merge row j (an accepted or PRESENT row of a touched key) owns the entries
// src[j] .. + len[j]; in its group grp[j] (base g_base) they are the entries
// dst[j] ..: key = e << 32 | index in the group, with the entry's merge row and
// prio beside it.  Its cover csrc[j] .. + clen[j] moves to cdst[j] .., so that
// a group's covers are one range.
struct NiRows {
	const uint64_t *src, *dst, *csrc, *cdst;
	const uint32_t *len, *clen, *grp;
	uint32_t nrows;
};

__global__ __launch_bounds__(kNiThreads) void k_ni_gather(NiRows R, const uint64_t* __restrict__ g_base,
                                                          const uint32_t* __restrict__ elems,
                                                          const int8_t* __restrict__ prios,
                                                          const uint32_t* __restrict__ cover, uint64_t* keys,
                                                          uint32_t* ent_row, int8_t* ent_prio, uint32_t* gcover)
{
	for (uint32_t j = blockIdx.x; j < R.nrows; j += gridDim.x) {
		const uint64_t s = R.src[j], d = R.dst[j], gb = g_base[R.grp[j]];
		const uint32_t n = R.len[j];
		for (uint32_t t = threadIdx.x; t < n; t += kNiThreads) {
			keys[d + t] = ((uint64_t)elems[s + t] << 32) | (uint32_t)(d + t - gb);
			ent_row[d + t] = j;
			ent_prio[d + t] = prios[s + t];
		}
		const uint64_t cs = R.csrc[j], cd = R.cdst[j];
		const uint32_t cn = R.clen[j];
		for (uint32_t t = threadIdx.x; t < cn; t += kNiThreads)
			gcover[cd + t] = cover[cs + t];
	}
}

// One workgroup per group streams its sorted keys.  An element's entries are
// one run in arrival order; the run's head thread walks it: per merge row the
// last entry (Deserialize: a later duplicate wins, signal.go:59-71), the max
// over the rows (Merge, signal.go:117-131).  Heads are counted by a block scan
// with a running total: element and prio go out densely from the group's base.
__global__ __launch_bounds__(kNiThreads) void k_ni_reduce(const uint64_t* __restrict__ sorted,
                                                          const uint64_t* __restrict__ g_base,
                                                          const uint32_t* __restrict__ g_len, uint32_t G,
                                                          const uint32_t* __restrict__ ent_row,
                                                          const int8_t* __restrict__ ent_prio, uint32_t* st_e,
                                                          int8_t* st_p, uint32_t* cnt)
{
	__shared__ uint32_t s_w[2][kNiThreads / 64];
	const uint32_t tid = threadIdx.x, wv = tid >> 6;
	for (uint32_t g = blockIdx.x; g < G; g += gridDim.x) {
		const uint64_t gb = g_base[g], n = g_len[g];
		const uint64_t* s = sorted + gb;
		uint32_t run = 0, it = 0;
		for (uint64_t b0 = 0; b0 < n; b0 += kNiThreads, it ^= 1) {
			const uint64_t i = b0 + tid;
			uint32_t e = 0;
			bool head = false;
			if (i < n) {
				e = (uint32_t)(s[i] >> 32);
				head = i == 0 || (uint32_t)(s[i - 1] >> 32) != e;
			}
			const uint32_t incl = wave_incl_scan((uint32_t)head);
			if (lane_id() == 63)
				s_w[it][wv] = incl;
			__syncthreads();  // (s_w[it] is rewritten two sweeps on, past the next sweep's barrier)
			uint32_t wb = 0, tot = 0;
#pragma unroll
			for (uint32_t x = 0; x < kNiThreads / 64; x++) {
				wb += x < wv ? s_w[it][x] : 0;
				tot += s_w[it][x];
			}
			if (head) {
				int m = kPrioAbsent;
				uint32_t row_next = 0;
				for (uint64_t q = i; q < n && (uint32_t)(s[q] >> 32) == e; q++) {
					const uint32_t idx = (uint32_t)s[q], row = q == i ? ent_row[gb + idx] : row_next;
					const bool more = q + 1 < n && (uint32_t)(s[q + 1] >> 32) == e;
					row_next = more ? ent_row[gb + (uint32_t)s[q + 1]] : 0;
					if (more && row_next == row)
						continue;  // an earlier duplicate inside one Serial
					const int pr = ent_prio[gb + idx];
					m = pr > m ? pr : m;
				}
				const uint64_t pos = gb + run + wb + incl - 1;
				st_e[pos] = e;
				st_p[pos] = (int8_t)m;
			}
			run += tot;
		}
		if (tid == 0)
			cnt[g] = run;
		__syncthreads();  // s_w starts over with the next group
	}
}

// host array -> scratch slot (the copy is stream-ordered; `h` outlives the call's last synchronisation)
static int ni_upload(syzsig_ctx* ctx, int slot, const void* h, size_t bytes, void** d)
{
	SYZ_TRY(ws_get(ctx, slot, bytes + 256, d));
	if (bytes)
		SYZ_HIP(hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
	return SYZSIG_OK;
}

// one batch, as the entry point validated it
struct NiBatch {
	uint32_t K, nkeys;
	const uint32_t* key;
	const uint8_t* flags;
	const uint64_t *sig_off, *cover_off;
	const uint32_t* elems;
	const int8_t* prios;
	const uint32_t* cover;
	uint64_t n_all, c_all;  // entries and PCs of all rows
	// device copies of the Serials and covers from sig_off[0] / cover_off[0] on
	const uint32_t* d_elems;
	const int8_t* d_prios;
	const uint32_t* d_cover;
	bool present(uint32_t i) const { return flags[i] & SYZSIG_INPUT_PRESENT; }
	uint64_t sig_at(uint32_t i) const { return sig_off[i] - sig_off[0]; }
	uint64_t sig_len(uint32_t i) const { return sig_off[i + 1] - sig_off[i]; }
	uint64_t cov_at(uint32_t i) const { return cover_off[i] - cover_off[0]; }
	uint64_t cov_len(uint32_t i) const { return cover_off[i + 1] - cover_off[i]; }
};

// what acceptance leaves for the commit
struct NiAccept {
	bool sequential = false;
	// batched: the events, the rows' flags on device
	uint64_t* d_ev = nullptr;
	uint64_t E = 0;
	uint8_t* d_acc = nullptr;
	// sequential: the clones the loop ran on (nullptr = still nil)
	syzsig_set *cs = nullptr, *cv = nullptr;
	OwnedSets work;
};

// The reference loop itself (manager.go:976-998), one input after the other
// over the set ops, on clones of corpusSignal and corpusCover: the exact path
// for a batch past kNiMaxEntries or with an element partition past
// kRpCap.  Nothing the caller holds is touched; ni_commit swaps the
// clones in.
static int ni_accept_sequential(syzsig_ctx* ctx, const NiBatch& B, syzsig_set* corpus_signal, syzsig_set* corpus_cover,
                                uint8_t* acc, NiAccept* A)
{
	A->sequential = true;
	SYZ_TRY(syzsig_set_clone(ctx, corpus_signal, &A->cs));
	A->work.add(A->cs);
	SYZ_TRY(syzsig_set_clone(ctx, corpus_cover, &A->cv));
	A->work.add(A->cv);
	for (uint32_t i = 0; i < B.K; i++) {
		if (B.present(i))
			continue;
		const uint64_t a = B.sig_off[i], n = B.sig_len(i);
		OwnedSets tmp;  // inputSignal and the Diff, freed at the end of the iteration
		syzsig_set *in = nullptr, *diff = nullptr;
		SYZ_TRY(syzsig_deserialize(ctx, n ? B.elems + a : nullptr, n, n ? B.prios + a : nullptr, n, &in));
		tmp.add(in);
		SYZ_TRY(syzsig_diff(ctx, A->cs, in, &diff));
		tmp.add(diff);
		if (syzsig_empty(diff))
			continue;  // :993
		SYZ_TRY(merge_into(ctx, A->work, &A->cs, in));  // :997
		SYZ_TRY(cover_merge_into(ctx, A->work, &A->cv, B.cov_len(i) ? B.cover + B.cover_off[i] : nullptr,
		                         B.cov_len(i)));  // :998
		acc[i] = 1;
	}
	return SYZSIG_OK;
}

// The batched acceptance: acc[i] for the non-PRESENT rows, the events left on
// the device.  *spilled: a partition past kRpCap (nothing usable).
static int ni_accept_batched(syzsig_ctx* ctx, const NiBatch& B, const syzsig_set* cs, uint64_t nA, uint8_t* acc,
                             NiAccept* A, bool* spilled)
{
	*spilled = false;
	const hipStream_t s = ctx->stream;
	const uint32_t K = B.K;
	// the acceptance rows' tables: src, dst (u64), len, row (u32)
	uint32_t R = 0;
	for (uint32_t i = 0; i < K; i++)
		R += !B.present(i) && B.sig_len(i) != 0;
	std::vector<uint64_t> tab((size_t)R * 3 + 1);
	uint64_t *h_src = tab.data(), *h_dst = h_src + R;
	uint32_t *h_len = (uint32_t*)(h_dst + R), *h_row = h_len + R;
	uint64_t d = 0;
	for (uint32_t i = 0, j = 0; i < K; i++) {
		if (B.present(i) || B.sig_len(i) == 0)
			continue;
		h_src[j] = B.sig_at(i);
		h_dst[j] = d;
		h_len[j] = (uint32_t)B.sig_len(i);  // (nA <= 2^23)
		h_row[j++] = i;
		d += B.sig_len(i);
	}
	void *dtab, *dx, *drec, *dev, *dacc;
	SYZ_TRY(ni_upload(ctx, kWsNiStageA, tab.data(), (size_t)R * 24, &dtab));
	SYZ_TRY(ws_get(ctx, kWsNiStageB, nA * 8 + 64, &dx));
	SYZ_TRY(ws_get(ctx, kWsNiRecs, align256(nA * 4) + nA + 64, &drec));
	SYZ_TRY(ws_get(ctx, kWsNiEvents, nA * 8 + 64, &dev));
	SYZ_TRY(ws_get(ctx, kWsNiAccepted, (size_t)K + 64, &dacc));
	uint32_t* rec_row = (uint32_t*)drec;
	int8_t* rec_prio = (int8_t*)((char*)drec + align256(nA * 4));
	SYZ_HIP(hipMemsetAsync(dacc, 0, K, s));
	unsigned long long* nev = &ctx->d_cnt[kCntAux];
	if (nA) {
		const uint64_t* t = (const uint64_t*)dtab;
		k_ni_rows<<<grid_cap(R, kNiMaxGrid), kNiThreads, 0, s>>>(t, t + R, (const uint32_t*)(t + 2 * (size_t)R),
		                                            (const uint32_t*)(t + 2 * (size_t)R) + R, R, B.d_elems, B.d_prios,
		                                            (uint64_t*)dx, rec_row, rec_prio);
		uint64_t* keys;
		uint32_t* base;
		uint32_t pbits;
		SYZ_TRY(rp_group(ctx, (const uint64_t*)dx, nA, &keys, &base, &pbits, ctx->d_cnt));  // (zeroes the counters)
		k_ni_walk<<<1u << pbits, kNiThreads, 0, s>>>(keys, base, pbits, rec_row, rec_prio, cs ? cs->slots : nullptr,
		                                             cs ? cs->nbuckets - 1 : 0, (uint64_t*)dev, nA, nev, (uint8_t*)dacc,
		                                             ctx->d_cnt);
		SYZ_HIP(hipGetLastError());
	} else {
		SYZ_TRY(counters_reset(ctx));
	}
	if (K)
		SYZ_HIP(hipMemcpyAsync(acc, dacc, K, hipMemcpyDeviceToHost, s));
	SYZ_TRY(counters_fetch(ctx));  // (synchronizes: tab and acc are consumed)
	if (ctx->h_cnt[kCntSpill]) {
		*spilled = true;
		std::fill(acc, acc + K, 0);
		return SYZSIG_OK;
	}
	A->d_ev = (uint64_t*)dev;
	A->E = std::min<uint64_t>(ctx->h_cnt[kCntAux], nA);
	A->d_acc = (uint8_t*)dacc;
	return SYZSIG_OK;
}

// what the per-key merge computed, in host memory until the commit went through
struct NiKeys {
	std::vector<uint64_t> sig_off, cover_off;  // nkeys + 1
	std::vector<uint32_t> elems, cover;
	std::vector<int8_t> prios;
};

// The per-key merge of the rows acc[] marks (PRESENT rows included) for the
// keys touched[] marks.  Synchronises; writes only `out` and ctx->ni_stats.
static int ni_merge_keys(syzsig_ctx* ctx, const NiBatch& B, const uint8_t* acc, const uint8_t* touched, NiKeys* out)
{
	const hipStream_t s = ctx->stream;
	const uint32_t K = B.K, nkeys = B.nkeys;
	out->sig_off.assign((size_t)nkeys + 1, 0);
	out->cover_off.assign((size_t)nkeys + 1, 0);
	// groups = the touched keys, ascending; their rows in arrival order (a stable counting sort by key)
	std::vector<uint32_t> grp_of(nkeys, ~0u), grp_key;
	for (uint32_t k = 0; k < nkeys; k++)
		if (touched[k]) {
			grp_of[k] = (uint32_t)grp_key.size();
			grp_key.push_back(k);
		}
	const uint32_t G = (uint32_t)grp_key.size();
	if (G == 0)
		return SYZSIG_OK;
	std::vector<uint32_t> g_rows(G + 1, 0);
	for (uint32_t i = 0; i < K; i++)
		if (acc[i] && touched[B.key[i]])
			g_rows[grp_of[B.key[i]] + 1]++;
	for (uint32_t g = 0; g < G; g++)
		g_rows[g + 1] += g_rows[g];
	const uint32_t M = g_rows[G];
	std::vector<uint32_t> mrow(M), cur(g_rows.begin(), g_rows.end() - 1);
	for (uint32_t i = 0; i < K; i++)
		if (acc[i] && touched[B.key[i]])
			mrow[cur[grp_of[B.key[i]]]++] = i;
	// row tables (src, dst, csrc, cdst: u64; len, clen, grp: u32) and group tables (g_base: u64; g_len: u32)
	std::vector<uint64_t> rt((size_t)M * 6 + 2), gt((size_t)G * 2 + 2);
	uint64_t *r_src = rt.data(), *r_dst = r_src + M, *r_csrc = r_dst + M, *r_cdst = r_csrc + M;
	uint32_t *r_len = (uint32_t*)(r_cdst + M), *r_clen = r_len + M, *r_grp = r_clen + M;
	uint64_t* g_base = gt.data();
	uint32_t* g_len = (uint32_t*)(g_base + G);
	std::vector<uint64_t> gc_start(G);
	std::vector<uint32_t> gc_len(G);
	uint64_t nM = 0, cM = 0, maxlen = 0, ntiles = 0, nlarge = 0;
	for (uint32_t g = 0; g < G; g++) {
		g_base[g] = nM;
		gc_start[g] = cM;
		uint64_t gl = 0, gcl = 0;
		for (uint32_t j = g_rows[g]; j < g_rows[g + 1]; j++) {
			const uint32_t i = mrow[j];
			r_src[j] = B.sig_at(i);
			r_dst[j] = nM + gl;
			r_len[j] = (uint32_t)B.sig_len(i);  // (a key's rows hold < 2^32 entries: checked by the entry)
			r_csrc[j] = B.cov_at(i);
			r_cdst[j] = cM + gcl;
			r_clen[j] = (uint32_t)B.cov_len(i);
			r_grp[j] = g;
			gl += B.sig_len(i);
			gcl += B.cov_len(i);
		}
		g_len[g] = (uint32_t)gl;
		gc_len[g] = (uint32_t)gcl;
		nM += gl;
		cM += gcl;
		maxlen = std::max(maxlen, gl);
		ntiles += (gl + kNiTile - 1) / kNiTile;
		nlarge += gl > kNiTile;
	}
	std::vector<uint32_t> tt((size_t)ntiles * 2 + 1);
	uint32_t *t_g = tt.data(), *t_idx = t_g + ntiles;
	for (uint32_t g = 0, b = 0; g < G; g++)
		for (uint32_t t = 0; t < (g_len[g] + (uint64_t)kNiTile - 1) / kNiTile; t++) {
			t_g[b] = g;
			t_idx[b++] = t;
		}
	void *drt, *dgt, *dtt, *dkeys, *dba, *dbb = nullptr, *dent, *dst_, *dgcov;
	SYZ_TRY(ni_upload(ctx, kWsNiRecTab, rt.data(), (size_t)M * 44, &drt));
	SYZ_TRY(ni_upload(ctx, kWsNiGroupTab, gt.data(), (size_t)G * 12, &dgt));
	SYZ_TRY(ni_upload(ctx, kWsNiTiles, tt.data(), (size_t)ntiles * 8, &dtt));
	SYZ_TRY(ws_get(ctx, kWsNiKeys, nM * 8 + 64, &dkeys));
	SYZ_TRY(ws_get(ctx, kWsNiBufA, nM * 8 + 64, &dba));
	if (maxlen > kNiTile)
		SYZ_TRY(ws_get(ctx, kWsNiBufB, nM * 8 + 64, &dbb));
	SYZ_TRY(ws_get(ctx, kWsNiEntries, align256(nM * 4) + nM + 64, &dent));
	SYZ_TRY(ws_get(ctx, kWsNiState, align256(nM * 4) + align256(nM) + align256((size_t)G * 4) + ((size_t)G + 1) * 8 + 64, &dst_));
	SYZ_TRY(ws_get(ctx, kWsNiGroupCover, cM * 4 + 64, &dgcov));
	const uint64_t* drt64 = (const uint64_t*)drt;
	const uint32_t* drt32 = (const uint32_t*)(drt64 + 4 * (size_t)M);
	const NiRows R{drt64, drt64 + M, drt64 + 2 * (size_t)M, drt64 + 3 * (size_t)M, drt32, drt32 + M, drt32 + 2 * (size_t)M, M};
	const uint64_t* dg_base = (const uint64_t*)dgt;
	const uint32_t* dg_len = (const uint32_t*)(dg_base + G);
	// every group is a "long segment" of the tile table, in place: group g's keys at g_base[g] of keys and buffers
	const SuTiles T{nullptr, (uint64_t*)dgt, (uint32_t*)dg_len, (uint32_t*)dtt, (uint32_t*)dtt + ntiles, G, ntiles};
	const SuSegs S{dkeys, 1, dg_base, dg_len, 1, dg_len, G};
	uint32_t* ent_row = (uint32_t*)dent;
	int8_t* ent_prio = (int8_t*)((char*)dent + align256(nM * 4));
	uint32_t* st_e = (uint32_t*)dst_;
	int8_t* st_p = (int8_t*)((char*)dst_ + align256(nM * 4));
	uint32_t* d_cnt_g = (uint32_t*)((char*)st_p + align256(nM));
	uint64_t* d_off = (uint64_t*)((char*)d_cnt_g + align256((size_t)G * 4));
	k_ni_gather<<<grid_cap(M, kNiMaxGrid), kNiThreads, 0, s>>>(R, dg_base, B.d_elems, B.d_prios, B.d_cover, (uint64_t*)dkeys, ent_row,
	                                              ent_prio, (uint32_t*)dgcov);
	k_su_tile_sort<NiTile><<<grid_cap(ntiles, kNiMaxGrid), kNiThreads, 0, s>>>(S, T, (uint64_t*)dba, nullptr);
	uint64_t *src = (uint64_t*)dba, *dst = (uint64_t*)dbb, passes = 0;
	for (uint64_t w = kNiTile; w < maxlen; w <<= 1, passes++) {
		k_su_merge<NiTile::Key, kNiTile><<<grid_cap(ntiles, kNiMaxGrid), kNiThreads, 0, s>>>(T, w, src, dst, nullptr);
		std::swap(src, dst);
	}
	k_ni_reduce<<<grid_cap(G, kNiMaxGrid), kNiThreads, 0, s>>>(src, dg_base, dg_len, G, ent_row, ent_prio, st_e, st_p, d_cnt_g);
	SYZ_HIP(hipGetLastError());
	std::vector<uint32_t> cnt(G);
	SYZ_HIP(hipMemcpyAsync(cnt.data(), d_cnt_g, (size_t)G * 4, hipMemcpyDeviceToHost, s));
	SYZ_HIP(hipStreamSynchronize(s));  // (rt, gt, tt are consumed)
	std::vector<uint64_t> off((size_t)G + 1, 0);
	for (uint32_t g = 0; g < G; g++)
		off[g + 1] = off[g] + std::min<uint32_t>(cnt[g], g_len[g]);
	const uint64_t total = off[G];
	void* dout;
	SYZ_TRY(ws_get(ctx, kWsNiOut, align256(total * 4) + total + 64, &dout));
	int8_t* out_p = (int8_t*)((char*)dout + align256(total * 4));
	SYZ_HIP(hipMemcpyAsync(d_off, off.data(), ((size_t)G + 1) * 8, hipMemcpyHostToDevice, s));
	k_su_gather<<<grid_cap(G, kNiMaxGrid), kNiThreads, 0, s>>>(st_e, dg_base, 1, 1, d_off, G, (uint32_t*)dout, nullptr);
	k_su_gather<<<grid_cap(G, kNiMaxGrid), kNiThreads, 0, s>>>(st_p, dg_base, 1, 1, d_off, G, out_p, nullptr);
	SYZ_HIP(hipGetLastError());
	out->elems.resize(total);
	out->prios.resize(total);
	if (total) {
		SYZ_HIP(hipMemcpyAsync(out->elems.data(), dout, total * 4, hipMemcpyDeviceToHost, s));
		SYZ_HIP(hipMemcpyAsync(out->prios.data(), out_p, total, hipMemcpyDeviceToHost, s));
	}
	SYZ_HIP(hipStreamSynchronize(s));
	for (uint32_t g = 0; g < G; g++)
		out->sig_off[(size_t)grp_key[g] + 1] = off[g + 1] - off[g];
	for (uint32_t k = 0; k < nkeys; k++)
		out->sig_off[(size_t)k + 1] += out->sig_off[k];
	ctx->ni_stats[1] = nlarge;
	ctx->ni_stats[2] = passes;
	// the covers: one item per group with one run, the group's gathered covers
	// (cover.hip's segmented sort-unique; a run with signal, executed, no errno)
	if (cM) {
		const size_t o_keep = align256(G), o_exec = o_keep + align256(G), o_errno = o_exec + align256(G),
		             o_roff = o_errno + align256((size_t)G * 4), o_cs = o_roff + align256(((size_t)G + 1) * 8),
		             o_cl = o_cs + align256((size_t)G * 8), o_ooff = o_cl + align256((size_t)G * 4),
		             o_end = o_ooff + align256(((size_t)G + 1) * 8);
		std::vector<char> it(o_end, 0);
		std::fill(it.begin() + o_keep, it.begin() + o_keep + G, 1);
		std::fill(it.begin() + o_exec, it.begin() + o_exec + G, 1);
		for (uint32_t g = 0; g <= G; g++)
			((uint64_t*)(it.data() + o_roff))[g] = g;
		std::copy(gc_start.begin(), gc_start.end(), (uint64_t*)(it.data() + o_cs));
		std::copy(gc_len.begin(), gc_len.end(), (uint32_t*)(it.data() + o_cl));
		char* dit;
		void* dcout;
		SYZ_TRY(ni_upload(ctx, kWsNiItems, it.data(), o_end, (void**)&dit));
		SYZ_TRY(ws_get(ctx, kWsNiCoverOut, cM * 4 + 64, &dcout));
		uint64_t ctot = 0;
		SYZ_TRY(syzsig_triage_cover_dev(ctx, G, 1, (const uint8_t*)dit, (const uint8_t*)(dit + o_keep),
		                                (const uint64_t*)(dit + o_roff), (const int32_t*)(dit + o_errno),
		                                (const uint8_t*)(dit + o_exec), (const uint32_t*)dgcov, cM,
		                                (const uint64_t*)(dit + o_cs), (const uint32_t*)(dit + o_cl),
		                                (uint64_t*)(dit + o_ooff), (uint32_t*)dcout, cM, &ctot));
		ctx->ni_stats[3] = ctx->h_cnt[kSuLarge];  // (the groups past cover.hip's tile)
		std::vector<uint64_t> coff((size_t)G + 1);
		SYZ_HIP(hipMemcpyAsync(coff.data(), dit + o_ooff, ((size_t)G + 1) * 8, hipMemcpyDeviceToHost, s));
		out->cover.resize(ctot);
		if (ctot)
			SYZ_HIP(hipMemcpyAsync(out->cover.data(), dcout, ctot * 4, hipMemcpyDeviceToHost, s));
		SYZ_HIP(hipStreamSynchronize(s));
		for (uint32_t g = 0; g < G; g++)
			out->cover_off[(size_t)grp_key[g] + 1] = coff[g + 1] - coff[g];
		for (uint32_t k = 0; k < nkeys; k++)
			out->cover_off[(size_t)k + 1] += out->cover_off[k];
	}
	return SYZSIG_OK;
}

// The commit.  Batched: every allocation first, then one launch (its only
// failure an internal overflow).  Sequential: the clones swapped in.
static int ni_commit(syzsig_ctx* ctx, const NiBatch& B, const uint8_t* acc, NiAccept* A, syzsig_set** corpus_signal,
                     syzsig_set** corpus_cover)
{
	if (A->sequential) {
		A->work.release();
		swap_in(corpus_signal, A->cs);
		swap_in(corpus_cover, A->cv);
		return SYZSIG_OK;
	}
	uint64_t cacc = 0;
	bool any = false;
	for (uint32_t i = 0; i < B.K; i++)
		if (acc[i] && !B.present(i)) {
			any = true;
			cacc += B.cov_len(i);
		}
	if (!any)
		return SYZSIG_OK;  // nil sets stay nil
	const hipStream_t s = ctx->stream;
	Receiver cs, cv;
	SYZ_TRY(cs.open(ctx, corpus_signal, A->E));  // Merge allocates a nil receiver (signal.go:121-125)
	SYZ_TRY(cv.open(ctx, corpus_cover, cacc));   // cover.go:9-18: even for an empty cover
	void *dfl, *dco;
	SYZ_TRY(ni_upload(ctx, kWsNiStageA, B.flags, B.K, &dfl));
	std::vector<uint64_t> co((size_t)B.K + 1);
	for (uint32_t i = 0; i <= B.K; i++)
		co[i] = B.cover_off[i] - B.cover_off[0];
	SYZ_TRY(ni_upload(ctx, kWsNiStageB, co.data(), ((size_t)B.K + 1) * 8, &dco));
	SYZ_TRY(counters_reset(ctx));
	const uint32_t eb = (uint32_t)grid_for(A->E, kNiThreads, 8192), rb = cacc ? (uint32_t)grid_cap(B.K, kNiMaxGrid) : 0;
	k_ni_commit<<<eb + rb, kNiThreads, 0, s>>>(A->d_ev, A->E, eb, cs.slots(), cs.bmask(), A->d_acc,
	                                           (const uint8_t*)dfl, (const uint64_t*)dco, B.K, B.d_cover, cv.slots(),
	                                           cv.bmask(), ctx->d_cnt);
	SYZ_TRY(commit_tail(ctx, "manager_new_input_batch"));  // (synchronizes: co is consumed)
	cs.commit(ctx->h_cnt[kCntInserted]);
	cv.commit(ctx->h_cnt[kNiCovIns]);
	return SYZSIG_OK;
}

}  // namespace syz

using namespace syz;

extern "C" int syzsig_new_input_stats(syzsig_ctx* ctx, uint64_t out[4])
{
	return stats_copy(ctx, &syzsig_ctx::ni_stats, out, "new_input_stats");
}

extern "C" int syzsig_manager_new_input_batch(syzsig_ctx* ctx, syzsig_set** corpus_signal, syzsig_set** corpus_cover,
                                              uint32_t ninputs, uint32_t nkeys, const uint32_t* input_key,
                                              const uint8_t* input_flags, const uint64_t* sig_off,
                                              const uint32_t* elems, const int8_t* prios, const uint64_t* cover_off,
                                              const uint32_t* cover, uint8_t* accepted, uint8_t* new_key,
                                              uint8_t* key_touched, uint64_t* key_sig_off, uint32_t* key_elems,
                                              int8_t* key_prios, uint64_t sig_cap, uint64_t* key_cover_off,
                                              uint32_t* key_cover, uint64_t cover_cap)
{
	SYZ_LOCK(ctx);
	const uint32_t K = ninputs;
	if (!ctx || !corpus_signal || !corpus_cover || !key_sig_off || !key_cover_off || (nkeys && !key_touched) ||
	    (K && (!input_key || !input_flags || !sig_off || !cover_off || !accepted || !new_key)))
		return fail(SYZSIG_EINVAL, "manager_new_input_batch: NULL argument");
	SYZ_TRY(set_check_idle(*corpus_signal));
	SYZ_TRY(set_check_idle(*corpus_cover));
	// ---- checks, before anything is touched ----
	std::vector<uint64_t> key_n(nkeys, 0), key_c(nkeys, 0);
	for (uint32_t i = 0; i < K; i++) {
		if (input_key[i] >= nkeys || (input_flags[i] & ~SYZSIG_INPUT_PRESENT) || sig_off[i + 1] < sig_off[i] ||
		    cover_off[i + 1] < cover_off[i])
			return fail(SYZSIG_EINVAL, "manager_new_input_batch: a key >= nkeys, an unknown flag or a non-monotone offset");
		key_n[input_key[i]] += sig_off[i + 1] - sig_off[i];
		key_c[input_key[i]] += cover_off[i + 1] - cover_off[i];
	}
	const uint64_t n_all = K ? sig_off[K] - sig_off[0] : 0, c_all = K ? cover_off[K] - cover_off[0] : 0;
	if ((n_all && (!elems || !prios || !key_elems || !key_prios)) || (c_all && (!cover || !key_cover)))
		return fail(SYZSIG_EINVAL, "manager_new_input_batch: NULL Serial, cover or output arrays");
	if (sig_cap < n_all || cover_cap < c_all)
		return fail(SYZSIG_ERANGE, "manager_new_input_batch: sig_cap / cover_cap below the rows' total entries / PCs");
	for (uint32_t k = 0; k < nkeys; k++)
		if (key_n[k] >= (1ull << 32) || key_c[k] >= (1ull << 31))
			return fail(SYZSIG_ERANGE, "manager_new_input_batch: a key's rows hold 2^32 entries or 2^31 PCs or more");
	const auto t0 = std::chrono::steady_clock::now();
	std::fill(ctx->ni_stats, ctx->ni_stats + 4, 0);
	NiBatch B{K, nkeys, input_key, input_flags, sig_off, cover_off, elems, prios, cover, n_all, c_all, nullptr, nullptr, nullptr};
	void *de, *dp, *dc;
	SYZ_TRY(ni_upload(ctx, kWsNiElems, n_all ? elems + sig_off[0] : nullptr, n_all * 4, &de));
	SYZ_TRY(ni_upload(ctx, kWsNiPrios, n_all ? prios + sig_off[0] : nullptr, n_all, &dp));
	SYZ_TRY(ni_upload(ctx, kWsNiCover, c_all ? cover + cover_off[0] : nullptr, c_all * 4, &dc));
	B.d_elems = (const uint32_t*)de;
	B.d_prios = (const int8_t*)dp;
	B.d_cover = (const uint32_t*)dc;
	// ---- acceptance (:993): read-only on the caller's sets ----
	uint64_t nA = 0;
	for (uint32_t i = 0; i < K; i++)
		nA += B.present(i) ? 0 : B.sig_len(i);
	std::vector<uint8_t> acc(K, 0);
	NiAccept A;
	bool seq = nA > kNiMaxEntries;
	if (!seq)
		SYZ_TRY(ni_accept_batched(ctx, B, *corpus_signal, nA, acc.data(), &A, &seq));
	if (seq)
		SYZ_TRY(ni_accept_sequential(ctx, B, *corpus_signal, *corpus_cover, acc.data(), &A));
	ctx->ni_stats[0] = seq;
	// ---- :1000-1022 per key: which rows are new entries, which keys changed ----
	std::vector<uint8_t> nk(K, 0), touched(nkeys, 0), seen(nkeys, 0);
	for (uint32_t i = 0; i < K; i++) {
		const uint32_t k = input_key[i];
		if (B.present(i)) {
			acc[i] = 1;
		} else if (acc[i]) {
			touched[k] = 1;
			nk[i] = !seen[k];
		}
		seen[k] |= acc[i];
	}
	NiKeys keys;
	SYZ_TRY(ni_merge_keys(ctx, B, acc.data(), touched.data(), &keys));
	if (keys.elems.size() > sig_cap || keys.cover.size() > cover_cap)
		return fail(SYZSIG_EIO, "manager_new_input_batch: internal: the keys' entries exceed the rows'");
	// ---- commit (:997-998), then the outputs ----
	SYZ_TRY(ni_commit(ctx, B, acc.data(), &A, corpus_signal, corpus_cover));
	if (K) {
		std::copy(acc.begin(), acc.end(), accepted);
		std::copy(nk.begin(), nk.end(), new_key);
	}
	if (nkeys)
		std::copy(touched.begin(), touched.end(), key_touched);
	std::copy(keys.sig_off.begin(), keys.sig_off.end(), key_sig_off);
	std::copy(keys.cover_off.begin(), keys.cover_off.end(), key_cover_off);
	if (!keys.elems.empty()) {
		std::copy(keys.elems.begin(), keys.elems.end(), key_elems);
		std::copy(keys.prios.begin(), keys.prios.end(), key_prios);
	}
	if (!keys.cover.empty())
		std::copy(keys.cover.begin(), keys.cover.end(), key_cover);
	if (ctx->timing)  // (host wall time over the call; every path ends synchronised)
		ctx->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return SYZSIG_OK;
}
