// internal.h -- private structures and device primitives of libsyzsig.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>

#include "../../include/syzsig.h"
#include "common.h"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
namespace syz {
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
}  // namespace syz

#define SYZ_HIP(expr)                                                              \
	do {                                                                           \
		hipError_t e__ = (expr);                                                   \
		if (e__ != hipSuccess)                                                     \
			return syz::hip_fail(e__, #expr, __FILE__, __LINE__);                  \
	} while (0)

// Serialize this C-ABI call against every other call on the same context
// (NULL-safe: the entry point's own argument check then reports the error).
#define SYZ_LOCK(ctx) syz::CtxLock syz_lock__(ctx)

#define SYZ_TRY(expr)                                                              \
	do {                                                                           \
		int r__ = (expr);                                                          \
		if (r__ != SYZSIG_OK)                                                      \
			return r__;                                                            \
	} while (0)

// ---------------------------------------------------------------------------
// host-side objects
// ---------------------------------------------------------------------------
namespace syz {

// Device counters live in one small array per context (zeroed per operation).
enum Counter : int {
	kCntInserted = 0,   // new keys inserted into the destination table
	kCntOverflow,       // an insert found the whole table occupied (capacity too small) -> retry bigger
	kCntError,          // malformed input detected on device
	kCntCandidates,     // triage: records that passed the prio filter
	kCntTouched,        // triage: distinct elements with a candidate this run
	kCntChanged,        // triage: slots committed (prio raised or inserted)
	kCntAux,            // misc (serialize cursor, minimize winners...)
	kCntAux2,
	kCntDefer,          // triage finalize: elements deferred to the atomic path
	kCntDeferNs,        // triage finalize: newSignal merges deferred to the atomic path
	kCntDistinct,       // one-sync triage run / records mode: distinct elements
	kCntAggOvf,         // one-sync triage run: partitions that overflowed the LDS table
	kCntSpill,          // one-sync triage run: its void flag (low 32 bits; 1 = a cell spilled, 2 = assumptions)
	kCntRecords,        // one-sync triage run: the batch's records
	kNumCounters = 16,
};
// the sharded step's counter blocks in syzsig_ctx::d_step
constexpr int kStepSrc = 0, kStepOwn = 16, kStepBack = 32, kStepCounters = 48;

struct Workspace {
	void* ptr = nullptr;
	size_t size = 0;
};

// The context's grow-only scratch buffers (syzsig_ctx::ws, ws_get), by owner.
// A buffer is keyed by its index alone: two functions of one call chain must
// not take the same one.  Where a number has two names, the owners are entry
// points (or stages of one) that never run inside one another, and neither
// keeps the contents across calls.
enum WsSlot : int {
	// set operations and (de)serialization (table.hip), the stability filter
	// (stable.hip); 3 also the per-call triage path's candidates (triage.hip)
	kWsOp0 = 0,
	kWsOp1 = 1,
	kWsOp2 = 2,
	kWsOp3 = 3,
	// triage.hip: the per-call path's candidates (with kWsOp3), the batch's prio mask
	kWsCandMeta = 4,
	kWsCandCount = 5,
	kWsPrioMask = 6,
	// minimize.hip: the host entry's uploads (9 also synth.hip's tile offsets)
	kWsMinOff = 7,
	kWsMinElems = 8,
	kWsMinPrios = 9,
	kWsSynthTiles = 9,
	kWsMinKeep = 10,
	kWsRestoreKeys = 11,  // table.hip: set_restore_keys
	kWsCallBits = 12,     // triage.hip: per-record bits the caller did not ask for
	// agg.hip: a batch's (call, element) pairs -- raw, the dedup set, the result
	// (kept across the runs of a batch); minimize.hip's rank sort outside a batch
	kWsPairsRaw = 13,
	kWsMinSortKeys = 13,
	kWsPairSet = 14,
	kWsMinRank = 14,
	kWsPairs = 15,
	kWsMinSortHist = 15,
	// agg.hip: one aggregation run
	kWsAggRecs = 16,      // the partitioned records (capped cells: the dummy lines after them)
	kWsAggCells = 17,     // the cells' plan and counts (cap_layout), or the counted layout's offsets
	kWsAggTotals = 18,    // counted layout: per-partition totals and bases
	kWsAggDistE = 19,     // k_agg's distinct lists (agg_lists) ...
	kWsAggDistF = 20,
	kWsAggCnt = 21,       // ... and their region counts
	kWsAggOvfList = 22,   // agg_hbm_fallback: the overflowed partitions
	kWsAggHbmTable = 23,  // ... and their HBM table
	// check_new_signal's uploads (triage.hip) | the NewInput batch's per-key merge (corpus.hip)
	kWsCnsSigs = 24,
	kWsNiRecTab = 24,
	kWsCnsStart = 25,
	kWsNiKeys = 25,
	kWsCnsLen = 26,
	kWsNiBufA = 26,
	kWsCnsPrio = 27,
	kWsNiBufB = 27,
	kWsCnsBits = 28,
	kWsNiEntries = 28,
	kWsCnsNew = 29,
	kWsNiGroupTab = 29,
	// agg.hip: the HBM fallback's distinct lists (agg_aggregate: behind a copy of the LDS regions)
	kWsAggDistE2 = 30,
	kWsAggDistF2 = 31,
	// agg.hip: the slice-exclusive finalize's deferred lists (fin_args)
	kWsFinDefer = 32,
	kWsFinDeferNs = 33,
	// minimize.hip's virtual batch and shard cursors | corpus.hip's merge state and output
	kWsMinBatch = 34,
	kWsNiState = 34,
	kWsAggHbmCnt = 35,  // agg.hip: the one-sync run's fallback region counts | corpus.hip: merged cover
	kWsNiCoverOut = 35,
	kWsMinCursor = 36,
	kWsNiOut = 36,
	kWsSuStage2 = 37,  // comps.hip, items.hip (see kWsSuMeta)
	kWsNiGroupCover = 38,
	// manager poll (poll.hip) | the NewInput batch's acceptance and uploads (corpus.hip)
	// | the fuzzer's poll reply (pollres.hip): its routing arrays and the long segments' scratch tables
	kWsPollTargets = 39,
	kWsPrMeta = 39,
	kWsPollElems = 40,
	kWsNiElems = 40,
	kWsPollPrios = 41,
	kWsNiPrios = 41,
	kWsPollGroupIn = 42,
	kWsNiCover = 42,
	kWsPollKeys = 43,
	kWsNiStageA = 43,  // acceptance: the key table, then the commit: the inputs' flags
	kWsPollEvents = 44,
	kWsNiStageB = 44,  // acceptance: the sort keys, then the commit: cover offsets
	kWsNiRecs = 45,
	kWsPollTable = 46,
	kWsPrTable = 46,
	kWsNiEvents = 46,
	kWsPollCounts = 47,
	kWsNiAccepted = 47,
	// the sort-unique of cover.hip, of the comparison hints and of the triage items (comps.hip,
	// items.hip: with kWsSuStage2)
	// | rp_group, the LDS grouping for Poll (recs.hip): its one segment and its
	// keys; the partition front end's cell counts and bases (rp_partition)
	kWsSuMeta = 48,
	kWsRpgSeg = 48,
	kWsSuTab = 49,
	kWsRpgKeys = 49,
	kWsSuBufA = 50,
	kWsRpgCounts = 50,
	kWsSuBufB = 51,
	kWsRpgBase = 51,
	kWsSuStage = 52,
	// agg.hip: reserve_slices' histogram, the fast plan's partials | corpus.hip's merge tables
	kWsPartHist = 53,
	kWsNiTiles = 53,
	kWsFastPart = 54,
	kWsNiItems = 54,
	// the sharded step (agg.hip, recs.hip) and the LDS records path (recs.hip)
	kWsStepPairs = 55,
	kWsRpKeys = 56,    // rp_run: the keys, the records' slots, the element arrays
	kWsRpCounts = 57,  // rp_partition for rp_run: the cell counts / offsets ...
	kWsRpBase = 58,    // ... the partition bases; behind them rp_run's per-partition sums
	kWsRpSeg = 59,     // rp_triage_records: its one segment
	kWsStepShards = 60,
	kWsStepRecs = 61,
	kWsStepFlags = 62,
	kWsStepCursor = 63,
	// hints.hip: the args' counts and offsets, the fast path's staged mutants, the fallback's queries
	// (its fallback runs comps.hip's sort-unique inside the call: slots of its own)
	kWsHmMeta = 64,
	kWsHmStage = 65,
	kWsHmQuery = 66,
	// sigs.hip: the long messages' list | a batch of Sigs: its keys and the merge's other buffer, the
	// flags / ranks / tile table, the outputs held back until the commit
	kWsHashList = 67,
	kWsSgBufA = 68,
	kWsSgBufB = 69,
	kWsSgMeta = 70,
	kWsSgOut = 71,
	// prio.hip: the histogram, offsets, cursors and slice plan | the postings | the slices' partial rows
	kWsPqMeta = 72,
	kWsPqPost = 73,
	kWsPqPart = 74,
	// report.hip: a call's counts, offsets and cursors; the PCs in call order | the keys of report_pcs;
	// the sorted survivors before the gather | uncovered_pcs' add / del words and block counts
	// | file_set's per-file counts, offsets and the funcs bitmap; the keys in file order; the sorted lists
	kWsRcMeta = 75,
	kWsRcStage = 76,
	kWsRcStage2 = 77,
	// db.hip: the long streams' (values') list | the statuses, lengths and offsets held back until the call's
	// end (inflate, deflate, db_records)
	kWsInfList = 78,
	kWsInfMeta = 79,
	// calls.hip: the tiles' line counts and bases, the programs' first lines and held-back outputs | the
	// lines' starts and records | the long list | CallSet's raw ids and the sorted survivors
	kWsPcMeta = 80,
	kWsPcLines = 81,
	kWsPcList = 82,
	kWsPcStage = 83,
	kWsPcStage2 = 84,
	kWsCount = 85,
};

// the debug flags that change only the path taken, never a result
constexpr uint32_t kDebugResultPreserving =
    SYZSIG_DEBUG_FIN_DEFER | SYZSIG_DEBUG_MIN_ATOMIC | SYZSIG_DEBUG_EXACT_CELLS | SYZSIG_DEBUG_CAP_SPILL |
    SYZSIG_DEBUG_RECS_GATE | SYZSIG_DEBUG_EDGE_MARKALL | SYZSIG_DEBUG_EDGE_PASSES | SYZSIG_DEBUG_AGG_IDX64;
// ... and those a product build accepts: the above plus fault injection
constexpr uint32_t kDebugAccepted = kDebugResultPreserving | SYZSIG_DEBUG_POLL_FAIL;

// capped cells of the aggregation path (agg.hip): default slack, in standard deviations
constexpr float kCapSdDefault = 6.0f;

// ctx->h_pin layout
constexpr size_t kPinMask = 0, kPinPairs = 64, kPinCounts = 1024, kPinBytes = 64 * 1024;

}  // namespace syz

struct syzsig_ctx {
	// Every C-ABI entry point holds this for its whole duration (SYZ_LOCK): the
	// context's stream, scratch slots, counters and pinned staging are shared by
	// all callers, and the reference runs Diff/DiffRaw concurrently under
	// signalMu.RLock (syz-fuzzer/fuzzer.go:488-498).  Recursive: entry points
	// call each other (e.g. triage allocates newSignal through syzsig_set_make).
	std::recursive_mutex mu;
	int device = 0;
	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr;
	unsigned long long* d_cnt = nullptr;  // kNumCounters
	unsigned long long* h_cnt = nullptr;  // pinned mirror
	// pinned staging for the small per-batch copies (a pageable copy is staged
	// and synchronous): syz::kPin* offsets
	char* h_pin = nullptr;
	// grow-only scratch buffers, one per syz::WsSlot
	syz::Workspace ws[syz::kWsCount];
	bool timing = false;                  // HIP events around triage kernels
	// tuning knobs (defaults; SYZSIG_* environment overrides read at ctx creation)
	int part_mode = 1;                    // 0 = never use the aggregation path (agg.hip)
	uint32_t agg_parts = 0;               // fixed partition count of the aggregation path (0 = adaptive)
	double agg_distinct_ratio = 0;        // distinct/records of the last aggregated run (sizes the next)
	float cap_sd = syz::kCapSdDefault;    // capped-cell slack in standard deviations (agg.hip; 0 = counted cells)
	float cap_sd_entry = syz::kCapSdDefault;  // the same for Minimize's runs
	bool agg_counted_once = false;        // the next agg_aggregate takes counted cells (a one-sync run spilled)
	uint32_t edge_waves = 4;              // waves per program of k_edge_dedup (4 or 8; SYZSIG_EDGE_WAVES)
	bool edge_mark_all = true;            // k_edge_dedup's marking mode for the next launch (edge.hip)
	uint32_t agg_dbg = 0;                 // SYZSIG_DEBUG_* path flags (kDebugAccepted)
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	double last_ms = 0;                   // device time of the last timed entry point's kernels
	// the stream-ordered sharded step (syzsig_step_*): its counters, read once by
	// syzsig_step_finish -- [0,16) source, [16,32) owner, [32,48) flags back
	unsigned long long* d_step = nullptr;
	unsigned long long* h_step = nullptr;  // pinned mirror
	syzsig_set* step_ms = nullptr;         // the owner's shard and newSignal until finish
	syzsig_set* step_ns = nullptr;
	uint64_t step_parts = 0;
	bool step_own_exact = false;           // the owner step took the per-record path, which commits the lengths itself
	uint64_t step_src_parts = 1;           // the source run's aggregation partitions
	bool step_own_timed = false, step_src_timed = false, step_back_timed = false;
	hipEvent_t ev_step[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	uint64_t ni_stats[4] = {0, 0, 0, 0};  // syzsig_new_input_stats: the last NewInput batch's paths (corpus.hip)
	uint64_t it_stats[4] = {0, 0, 0, 0};  // syzsig_triage_items_stats: the last triage_items call's paths (items.hip)
	uint64_t pr_stats[4] = {0, 0, 0, 0};  // syzsig_poll_res_stats: the last fuzzer_poll_res call's paths (pollres.hip)
	uint64_t hm_stats[4] = {0, 0, 0, 0};  // syzsig_hint_mutants_stats: the last hint_mutants call's paths (hints.hip)
	uint64_t hs_stats[4] = {0, 0, 0, 0};  // syzsig_hash_stats: the last hash call's paths (sigs.hip)
	uint64_t pq_stats[4] = {0, 0, 0, 0};  // syzsig_prio_stats: the last calc_prios call's paths (prio.hip)
	uint64_t rc_stats[4] = {0, 0, 0, 0};  // syzsig_report_stats: the last coverage-report call's paths (report.hip)
	uint64_t fs_stats[4] = {0, 0, 0, 0};  // syzsig_file_set_stats: the last file_set call's paths (report.hip)
	uint64_t if_stats[4] = {0, 0, 0, 0};  // syzsig_inflate_stats: the last inflate call's paths (db.hip)
	uint64_t df_stats[4] = {0, 0, 0, 0};  // syzsig_deflate_stats: the last deflate call's paths (db.hip)
	uint64_t pc_stats[4] = {0, 0, 0, 0};  // syzsig_prog_calls_stats: the last prog_calls call's paths (calls.hip)
	bool hash_stage = true;             // syzsig_hash_dev stages a wave's span in LDS (SYZSIG_HASH_STAGE=0: never, for A/B)
};

struct syzsig_set {
	syzsig_ctx* ctx = nullptr;
	uint64_t* slots = nullptr;   // nbuckets * 8
	uint64_t nbuckets = 0;       // power of two
	uint64_t len = 0;            // live entries (host mirror of device truth)
	// triage side state, allocated on first batch
	uint32_t* firsts = nullptr;  // 4 per slot: epoch_rev << 24 | serial, per prio level
	uint32_t* touched = nullptr; // 1 bit per slot
	uint32_t epoch = 0;          // current epoch_rev (counts down 254..1)
	bool step_busy = false;      // an owner step is in flight on it (len not final until syzsig_step_finish)
	uint64_t nslots() const { return nbuckets * syz::kBucketSlots; }
};

namespace syz {

struct CtxLock {
	syzsig_ctx* c;
	explicit CtxLock(syzsig_ctx* x) : c(x)
	{
		if (c)
			c->mu.lock();
	}
	~CtxLock()
	{
		if (c)
			c->mu.unlock();
	}
	CtxLock(const CtxLock&) = delete;
	CtxLock& operator=(const CtxLock&) = delete;
};

// scratch buffer `i` of the context, grown to at least `bytes` (contents lost on growth)
int ws_get(syzsig_ctx* ctx, int i, size_t bytes, void** out);
// same, keeping the first `keep` bytes across a growth
int ws_grow_keep(syzsig_ctx* ctx, int i, size_t bytes, size_t keep, void** out);
int counters_reset(syzsig_ctx* ctx);
int counters_fetch(syzsig_ctx* ctx);  // sync + copy to ctx->h_cnt

// table lifecycle (table.hip)
uint64_t buckets_for(uint64_t n_entries);
int set_alloc(syzsig_ctx* ctx, uint64_t nbuckets, syzsig_set** out);
int set_reserve(syzsig_set* s, uint64_t extra);  // ensure room for len+extra
int set_reserve_load(syzsig_set* s, uint64_t extra, double load);  // ... at most `load` full
int set_rehash(syzsig_set* s, uint64_t nbuckets, bool drop_absent);
int set_ensure_triage_state(syzsig_set* s);
int merge_pairs_dev(syzsig_ctx* ctx, syzsig_set* dst, const uint64_t* d_pairs, uint64_t n);

// Prio levels of one triage run: DiffRaw compares prios as int8
// (signal.go:93), so levels follow signed order.
struct LevelMap {
	uint8_t lvl[256];  // prio (as u8) -> level, 0xff = not in this run
	int8_t val[4];     // level -> prio
	uint32_t n;
};
constexpr uint32_t kSerialMask = 0xFFFFFF;  // 24-bit serial index inside a run
int level_map_from_levels(const int8_t* levels, uint32_t nlevels, LevelMap* lm);

// aggregation path (agg.hip)
constexpr uint32_t kAggRegion = 7424;  // distinct-list region per partition (= LDS slots of k_agg)
struct AggOut {
	const uint32_t* dist_e;  // distinct elements; region r at [r * kAggRegion, + cnt[r])
	const uint4* dist_f;     // their first serial per level (0xFFFFFFFF = none)
	const uint32_t* cnt;     // per region, device
	uint32_t nregions;
	uint32_t parts;          // partitions P; regions [0, P) are partitions (nregions > P: HBM fallback lists)
	uint64_t D;              // distinct elements in all regions
};
// Per-record extras of an aggregation run, for Minimize (minimize.hip); triage
// passes none.
struct AggSrc {
	const int8_t* elem_prio;  // per-record prio, parallel to sigs (level lm.lvl[prio]); nullptr = the call's
	uint32_t nshards, shard;  // keep only the records whose element this shard owns (owner_of)
	double distinct_hint;     // expected distinct elements (0: the batch-ratio policy)
	unsigned int* bad_level = nullptr;  // if set: |= 1 when a record's prio has no level (lm.lvl[prio] == 0xff)
};
int agg_aggregate(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t c0, uint64_t c1, const LevelMap& lm,
                  uint64_t run_recs, syzsig_batch_stats* st, AggOut* out, const AggSrc* x = nullptr);
// validates a batch's call ranges (SYZSIG_EINVAL) and sums its records (triage.hip)
int batch_total_records(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t* total, uint32_t prio_mask[8]);
int agg_triage_run(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const syzsig_batch* b, uint64_t c0, uint64_t c1,
                   const LevelMap& lm, uint64_t run_recs, syzsig_batch_stats* st, uint64_t** pairs,
                   uint64_t* npairs);
// The whole batch as one aggregation run without a presence pass and its
// host round trip: levels 0..3 (signalPrio's range, fuzzer.go:513-521) and at
// most b->nrec records are assumed, checked on device before the scatter
// (k_fast_prep, k_cell_plan_fast), and the run commits nothing when they do not
// hold.  Zeroes b->call_new.  One host synchronisation; stats.records is set.
// *done = false: take the planned path.
int agg_triage_optimistic(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const syzsig_batch* b,
                          syzsig_batch_stats* st, uint64_t** pairs, uint64_t* npairs, bool* done);
int agg_mark_bits(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t c0, uint64_t c1, const uint64_t* pairs,
                  uint64_t p0, uint64_t p1);
// The run policy (agg.hip), for a batch's runs and the sharded step's source run:
// after a capped cell spilled, more slack (0 = counted cells from now on); after
// novf of P LDS partitions overflowed (D distinct in the others), a larger ratio.
int stage_times(syzsig_ctx* ctx, int first, int last, syzsig_batch_stats* st);  // timing on: ev[first..last] into st
void cap_slack_after_spill(float& slack);
void distinct_ratio_after_overflow(syzsig_ctx* ctx, uint64_t P, uint64_t novf, uint64_t D, uint64_t recs);
// records mode (triage.hip: the per-record path, and the entry; recs.hip: the LDS path)
int triage_records_impl(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const uint64_t* recs, uint64_t nrec,
                        const int8_t* levels, uint32_t nlevels, uint8_t* new_flags, syzsig_batch_stats* st,
                        bool allow_lds = true);
// *done = false: the LDS path voided itself (nothing committed), take the per-record path
int rp_triage_records(syzsig_ctx* ctx, syzsig_set* ms, syzsig_set** ns, const uint64_t* recs, uint64_t nrec,
                      const LevelMap& lm, uint8_t* new_flags, syzsig_batch_stats* st, bool* done);
// Entries x[r] = e << 32 | r (r < 2^32) grouped by element through the LDS
// partitions of recs.hip, for Poll (poll.hip): on return (enqueued only)
// keys[base[p] .. base[p + 1]) = h_residual << 32 | r of partition p's entries
// (partition = the top pbits of fmix32(e)), base on device (P + 1 entries);
// ctr zeroed, then ctr[kCntSpill] != 0 when a partition exceeds kRpCap
// entries (nothing after it is valid).
constexpr uint32_t kRpCap = 2048;  // records of one partition in LDS (recs.hip: local positions < 2^13)
int rp_group(syzsig_ctx* ctx, const uint64_t* x, uint64_t n, uint64_t** keys, uint32_t** base, uint32_t* pbits,
             unsigned long long* ctr);
// Stable LSD radix sort of n (u32 key, u32 value) pairs, keys < 2^key_bits
// (sort.hip), ping-pong between the input and tmp buffers; *keys_out /
// *vals_out = the sorted pairs.  Enqueues only; scratch workspace slot ws_slot.
int radix_sort_pairs(syzsig_ctx* ctx, uint32_t* keys, uint32_t* vals, uint32_t* keys_tmp, uint32_t* vals_tmp,
                     uint32_t n, uint32_t key_bits, uint32_t** keys_out, uint32_t** vals_out, int ws_slot);
// a set an owner step holds until syzsig_step_finish takes no other call
inline int set_check_idle(const syzsig_set* s)
{
	return s && s->step_busy ? fail(SYZSIG_EINVAL, "set is held by a sharded step until syzsig_step_finish") : 0;
}
int pairs_from_bits(syzsig_ctx* ctx, const syzsig_batch* b, const uint32_t* bits, uint64_t c0, uint64_t c1,
                    uint64_t bound, uint64_t** pairs, uint64_t* npairs);

// the default load-factor policy: a table is grown when live/slots exceeds this
constexpr double kMaxLoad = 0.75;
constexpr double kTargetLoad = 0.5;
constexpr double kHardLoad = 0.9;  // a reservation for a worst case grows the table only past this
// after a run's inserts: the table grown when it is past kMaxLoad
inline int set_grow_if_loaded(syzsig_set* s)
{
	return (double)s->len > kMaxLoad * (double)s->nslots() ? set_rehash(s, buckets_for(s->len), false) : SYZSIG_OK;
}

// A newSignal set made for this run (newSignal.Merge allocates a nil receiver,
// signal.go:121-125 -- but only when some DiffRaw is non-empty): dropped again,
// *ns back to nil, on every return that does not keep() it.
struct FreshNs {
	syzsig_set** ns;
	bool armed;
	FreshNs(syzsig_set** p, bool fresh) : ns(p), armed(fresh) {}
	FreshNs(const FreshNs&) = delete;
	~FreshNs() { drop(); }
	void keep() { armed = false; }
	bool drop()  // true: the set was this run's and is gone
	{
		if (armed) {
			syzsig_set_free(*ns);
			*ns = nullptr;
		}
		return std::exchange(armed, false);
	}
};

// The bookkeeping of a committed run: newSignal is kept when something
// changed (else a set made for the run is dropped again), the tables' lengths
// take the inserts, the stats the run.
inline void commit_run(syzsig_set* ms, syzsig_set* nsp, FreshNs& fresh, uint64_t inserted, uint64_t changed,
                       uint64_t ns_ins, syzsig_batch_stats* st)
{
	if (changed)
		fresh.keep();
	else if (fresh.drop())
		nsp = nullptr;
	ms->len += inserted;
	if (nsp)
		nsp->len += ns_ins;
	st->inserted += inserted;
	st->changed += changed;
	st->candidates += changed;
	st->runs++;
}

inline int grid_for(uint64_t n, int block, int max_blocks = 2048)
{
	uint64_t g = (n + block - 1) / block;
	if (g < 1)
		g = 1;
	if (g > (uint64_t)max_blocks)
		g = max_blocks;
	return (int)g;
}

// The tail of a launch that inserted into tables with room reserved: the
// launch error, the counters (synchronizes), and an overflow that the
// reservation rules out.  `who` = the entry point, for the message.
inline int commit_tail(syzsig_ctx* ctx, const char* who)
{
	SYZ_HIP(hipGetLastError());
	SYZ_TRY(counters_fetch(ctx));
	if (ctx->h_cnt[kCntOverflow])
		return fail(SYZSIG_EIO, std::string(who) + ": table overflow after reserve (internal error)");
	return SYZSIG_OK;
}

// the body of the syzsig_*_stats entry points: the last call's paths
inline int stats_copy(syzsig_ctx* ctx, uint64_t (syzsig_ctx::*stats)[4], uint64_t* out, const char* who)
{
	SYZ_LOCK(ctx);
	if (!ctx || !out)
		return fail(SYZSIG_EINVAL, std::string(who) + ": NULL argument");
	for (int i = 0; i < 4; i++)
		out[i] = (ctx->*stats)[i];
	return SYZSIG_OK;
}

}  // namespace syz

#include "receiver.h"

// ---------------------------------------------------------------------------
// device primitives
// ---------------------------------------------------------------------------
#if defined(__HIPCC__)
namespace syz {

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// number of set bits of `mask` below this lane
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

// Block-wide sum of v added to *counter by one thread.  Every thread of the
// block must call it (uniform control flow).
__device__ __forceinline__ void block_count(unsigned long long* counter, uint64_t v)
{
	__shared__ unsigned long long part;
	if (threadIdx.x == 0)
		part = 0;
	__syncthreads();
	v = wave_sum_u64(v);
	if (lane_id() == 0 && v)
		atomicAdd(&part, (unsigned long long)v);
	__syncthreads();
	if (threadIdx.x == 0 && part)
		atomicAdd(counter, part);
}

struct Bucket {
	uint64_t s[kBucketSlots];
};

__device__ __forceinline__ Bucket load_bucket(const uint64_t* p)
{
	const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
	Bucket B;
#pragma unroll
	for (uint32_t i = 0; i < kBucketSlots / 2; i++) {
		const ulonglong2 v = q[i];
		B.s[2 * i] = v.x;
		B.s[2 * i + 1] = v.y;
	}
	return B;
}

// Home bucket = the top bits of fmix32(key): slices of the table then hold
// contiguous ranges of h, which is what lets the aggregation path (agg.hip,
// partitioned by the same top bits) probe one slice per partition.
__device__ __forceinline__ uint64_t home_bucket(uint32_t key, uint64_t bmask)
{
	return ((uint64_t)fmix32(key) * (bmask + 1)) >> 32;
}

// The table primitives below have one body each; kPreloaded says whether the
// caller passes the home bucket already loaded (B = load_bucket of
// home_bucket(key)), so that a thread can issue the home-bucket loads of several
// tables or keys before it walks any of them.  A stale B is safe for the same
// reason a fresh one is: slots only go EMPTY -> key, and the CAS sees the
// current word.

// Lookup.  Returns the slot index, or -1 if absent (first empty slot reached:
// slots only ever go EMPTY -> key, so occupied slots form a prefix of every
// probe sequence).
template <bool kPreloaded>
__device__ __forceinline__ int64_t tbl_lookup_impl(const uint64_t* __restrict__ slots, uint64_t bmask, uint32_t key,
                                                   uint64_t& val, const Bucket& B0)
{
	uint64_t b = home_bucket(key, bmask);
	for (uint64_t n = 0; n <= bmask; n++) {
		const Bucket B = kPreloaded && n == 0 ? B0 : load_bucket(slots + (b << kBucketShift));
#pragma unroll
		for (int i = 0; i < (int)kBucketSlots; i++) {
			if (B.s[i] == kSlotEmpty)
				return -1;
			if (slot_key(B.s[i]) == key) {
				val = B.s[i];
				return (int64_t)((b << kBucketShift) + i);
			}
		}
		b = (b + 1) & bmask;
	}
	return -1;
}

__device__ __forceinline__ int64_t tbl_lookup(const uint64_t* __restrict__ slots, uint64_t bmask, uint32_t key,
                                              uint64_t& val)
{
	return tbl_lookup_impl<false>(slots, bmask, key, val, Bucket{});
}

__device__ __forceinline__ int64_t tbl_lookup_from(const uint64_t* __restrict__ slots, uint64_t bmask, uint32_t key,
                                                   uint64_t& val, Bucket B)
{
	return tbl_lookup_impl<true>(slots, bmask, key, val, B);
}

// Find `key`, inserting `ins` (a slot word for `key`) at the first empty slot
// if absent.  old = previous word (0 when this call inserted).  Returns -1
// when max_probe buckets were scanned without success (overflow).
template <bool kPreloaded>
__device__ __forceinline__ int64_t tbl_find_or_insert_impl(uint64_t* slots, uint64_t bmask, uint32_t key, uint64_t ins,
                                                           uint64_t& old, uint64_t max_probe, Bucket B)
{
	uint64_t b = home_bucket(key, bmask);
	for (uint64_t n = 0; n < max_probe; n++) {
		uint64_t* bp = slots + (b << kBucketShift);
		if (!kPreloaded || n)
			B = load_bucket(bp);
#pragma unroll
		for (int i = 0; i < (int)kBucketSlots; i++) {
			uint64_t s = B.s[i];
			if (s == kSlotEmpty) {
				s = atomicCAS(reinterpret_cast<unsigned long long*>(bp + i), 0ull, (unsigned long long)ins);
				if (s == kSlotEmpty) {
					old = 0;
					return (int64_t)((b << kBucketShift) + i);
				}
			}
			if (slot_key(s) == key) {
				old = s;
				return (int64_t)((b << kBucketShift) + i);
			}
		}
		b = (b + 1) & bmask;
	}
	return -1;
}

__device__ __forceinline__ int64_t tbl_find_or_insert(uint64_t* slots, uint64_t bmask, uint32_t key, uint64_t ins,
                                                      uint64_t& old, uint64_t max_probe)
{
	return tbl_find_or_insert_impl<false>(slots, bmask, key, ins, old, max_probe, Bucket{});
}

__device__ __forceinline__ int64_t tbl_find_or_insert_from(uint64_t* slots, uint64_t bmask, uint32_t key,
                                                           uint64_t ins, uint64_t& old, uint64_t max_probe, Bucket B)
{
	return tbl_find_or_insert_impl<true>(slots, bmask, key, ins, old, max_probe, B);
}

// Probe bound of an insert: the whole table.  The set operations reserve room
// first (set_reserve*: below load 1), so an empty slot exists and an insert
// cannot fail however long its chain is -- also when every key shares one home
// bucket; the triage probe path restarts on a bigger table when its table fills.
__device__ __forceinline__ uint64_t max_probe_for(uint64_t bmask)
{
	return bmask + 1;
}

// Insert-or-max (Merge rule).  Returns 1 if inserted, 0 otherwise; -1 overflow.
template <bool kPreloaded>
__device__ __forceinline__ int tbl_merge_impl(uint64_t* slots, uint64_t bmask, uint32_t key, int8_t prio, Bucket B)
{
	uint64_t v = make_slot(key, prio), old;
	int64_t idx = tbl_find_or_insert_impl<kPreloaded>(slots, bmask, key, v, old, max_probe_for(bmask), B);
	if (idx < 0)
		return -1;
	if (old == 0)
		return 1;
	if (old < v)
		atomicMax(reinterpret_cast<unsigned long long*>(slots + idx), (unsigned long long)v);
	return 0;
}

__device__ __forceinline__ int tbl_merge(uint64_t* slots, uint64_t bmask, uint32_t key, int8_t prio)
{
	return tbl_merge_impl<false>(slots, bmask, key, prio, Bucket{});
}

__device__ __forceinline__ int tbl_merge_from(uint64_t* slots, uint64_t bmask, uint32_t key, int8_t prio, Bucket B)
{
	return tbl_merge_impl<true>(slots, bmask, key, prio, B);
}

// corpusSignal.Merge and maxSignal.Merge of one (e, p) (fuzzer.go:456-457), or
// maxSignal's alone (:474) when !input: both tables' home buckets are loaded
// before either chain is walked.  Adds to the caller's counts.
__device__ __forceinline__ void tbl_merge2(uint64_t* corpus, uint64_t c_bmask, uint64_t* max, uint64_t m_bmask,
                                           uint32_t e, int8_t p, bool input, uint64_t& ins_c, uint64_t& ins_m,
                                           uint64_t& ovf)
{
	Bucket bc = {};
	if (input)
		bc = load_bucket(corpus + (home_bucket(e, c_bmask) << kBucketShift));
	const Bucket bm = load_bucket(max + (home_bucket(e, m_bmask) << kBucketShift));
	if (input) {
		const int rc = tbl_merge_from(corpus, c_bmask, e, p, bc);
		ins_c += rc == 1;
		ovf += rc < 0;
	}
	const int rm = tbl_merge_from(max, m_bmask, e, p, bm);
	ins_m += rm == 1;
	ovf += rm < 0;
}

// Merge of a batch's events (e << 32 | ... | prio ^ 0x80 in the low byte: poll.hip,
// corpus.hip) into one table, max-merged: an element's last event carries its
// final max, the earlier ones are below it.  This thread takes ev[first],
// ev[first + stride], ...
__device__ __forceinline__ void merge_events(const uint64_t* __restrict__ ev, uint64_t n, uint64_t first,
                                             uint64_t stride, uint64_t* tbl, uint64_t bmask, uint64_t& ins,
                                             uint64_t& ovf)
{
	for (uint64_t x = first; x < n; x += stride) {
		const uint64_t w = ev[x];
		const int rr = tbl_merge(tbl, bmask, (uint32_t)(w >> 32), (int8_t)((uint8_t)w ^ 0x80u));
		ins += rr == 1;
		ovf += rr < 0;
	}
}

}  // namespace syz
#endif
