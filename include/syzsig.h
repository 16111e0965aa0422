/*
 * syzsig.h -- C ABI of libsyzsig, the MI355X coverage-signal triage engine.
 *
 * This is the drop-in boundary for syzkaller's per-execution coverage-signal
 * path.  Each entry point names the reference interface it replaces
 * (paths relative to the upstream syzkaller tree); INTEGRATION.md shows the
 * cgo binding that keeps pkg/signal's Go API and its callers unchanged.
 *
 * Conventions
 *  - Every function returns int status: SYZSIG_OK (0) or a negative errno-style
 *    code; syzsig_last_error() gives a message (thread-local).
 *  - A `syzsig_set*` is a device-resident Signal.  NULL is Go's nil Signal:
 *    Len()==0, usable as a receiver, and syzsig_merge allocates it
 *    (signal.go:121-125).  Results that Go returns as nil come back as NULL.
 *  - Host arrays passed in are copied during the call and never retained (cgo
 *    pointer rules; CallInfo.Signal aliases executor shmem, pkg/ipc/ipc.go:410).
 *  - Threading: every entry point locks its context for the duration of the
 *    call, so concurrent readers -- Diff / DiffRaw / Intersection / Len from
 *    several goroutines under fuzzer.signalMu.RLock (syz-fuzzer/fuzzer.go:
 *    488-498) -- are safe and see consistent results.  Writers (Merge, triage)
 *    still need the caller's write lock for Go-level atomicity of their
 *    read-modify-write sequences, exactly as in the reference (signalMu.Lock,
 *    fuzzer.go:500-505; mgr.mu, syz-manager/manager.go:66).  A set must not be
 *    freed while another thread uses it.
 *  - "_dev" / batch entry points take device pointers and run on the context's
 *    stream (syzsig_ctx_set_stream); they return after the work completes.
 */
#ifndef SYZSIG_H
#define SYZSIG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYZSIG_OK 0
#define SYZSIG_EIO (-5)        /* HIP runtime / device error */
#define SYZSIG_ENOMEM (-12)
#define SYZSIG_EINVAL (-22)
#define SYZSIG_ERANGE (-34)    /* a size limit of this ABI exceeded */
#define SYZSIG_ECORRUPT (-74)  /* panic("corrupted Serial"), pkg/signal/signal.go:60-62 */

#define SYZSIG_ABI_VERSION 7

typedef struct syzsig_ctx syzsig_ctx;
typedef struct syzsig_set syzsig_set;

int syzsig_abi_version(void);
const char* syzsig_last_error(void);

/* ---- context: one per process and GPU ---- */
int syzsig_ctx_create(int device, syzsig_ctx** out);
void syzsig_ctx_destroy(syzsig_ctx* ctx);
/* Run subsequent work on `stream` (a hipStream_t; NULL = the context's own,
 * which is a blocking stream: ordered against the null stream both ways). */
int syzsig_ctx_set_stream(syzsig_ctx* ctx, void* stream);
void* syzsig_ctx_stream(syzsig_ctx* ctx);
/* Record HIP events around the triage kernels (batch stats probe_ms/decide_ms). */
int syzsig_ctx_set_timing(syzsig_ctx* ctx, int enable);
/* With timing on: device time (ms, HIP events on the context stream) of the
 * kernels of the last syzsig_edge_derive_dev / syzsig_minimize_dev call, or the
 * stream work of the last syzsig_manager_poll_batch, syzsig_edge_cover_dev,
 * syzsig_triage_cover_dev, syzsig_triage_items_dev, syzsig_exec_comps_dev,
 * syzsig_comp_map_dev, syzsig_shrink_expand_dev, syzsig_hint_mutants_dev, syzsig_hash_dev or
 * syzsig_sigset_add_dev call, or of the last syzsig_calc_prios_dev, syzsig_static_prio_finish_dev,
 * syzsig_choice_table_dev, syzsig_choice_lookup_dev, syzsig_call_cover_dev, syzsig_report_pcs_dev,
 * syzsig_uncovered_pcs_dev or syzsig_file_set_dev call (uploads / first kernel to its last kernel,
 * including the host round trips between); for syzsig_manager_new_input_batch
 * the host wall time of the call, which ends synchronised. */
double syzsig_ctx_last_ms(syzsig_ctx* ctx);
/* Measurement: a plain device copy of `bytes` (16-B aligned buffers and size)
 * on the context stream, 16 B per lane per step; *ms = its device time (HIP
 * events).  The achievable-bandwidth companion of the bench's rooflines
 * (SURVEY.md 8(d)); not part of pkg/signal.  Synchronises. */
int syzsig_copy_bw_dev(syzsig_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes, double* ms);
/* Page-locked host memory (hipHostMalloc): host arrays handed to the library
 * from it are uploaded by DMA without a staging copy (the manager's Poll
 * batch builds its Serials there).  *out = NULL for 0 bytes; free with
 * syzsig_host_free (NULL is a no-op). */
int syzsig_host_alloc(syzsig_ctx* ctx, uint64_t bytes, void** out);
int syzsig_host_free(syzsig_ctx* ctx, void* p);
/* Large-batch triage path selection (tests and tuning; results never depend on it):
 * mode 0 = per-call probe path only, 1 = aggregation path for runs of >= 2^20
 * records (default), 2 = aggregation path always; parts = fixed partition
 * count of the aggregation path (0 = adaptive, else 8..2048). */
int syzsig_ctx_set_agg(syzsig_ctx* ctx, int mode, uint32_t parts);

/* Test knobs that change the code path but never the results:
 * SYZSIG_DEBUG_FIN_DEFER = the batch finalize sends every element whose probe
 * sequence leaves its home bucket to the atomic (deferred) path;
 * SYZSIG_DEBUG_MIN_ATOMIC = Minimize takes its per-entry atomicMax path instead
 * of the aggregation path;
 * SYZSIG_DEBUG_EXACT_CELLS = large triage runs partition records into counted
 * cells (count pass + scan) instead of capped cells;
 * SYZSIG_DEBUG_RECS_GATE = the LDS-partitioned records path (records mode,
 * the owner side of a sharded step) reports every input as over its capacity,
 * so the per-record path and the step's owner fix-up run (tests).
 * SYZSIG_DEBUG_CAP_SPILL = capped cells of 64 records, so that dense runs
 * overflow them and take the redo with counted cells.
 * SYZSIG_DEBUG_EDGE_MARKALL / SYZSIG_DEBUG_EDGE_PASSES = syzsig_edge_derive_dev
 * runs the dedup rounds with one marking pass / with marking passes, instead
 * of choosing from the previous launch's duplicate rate.
 * SYZSIG_DEBUG_AGG_IDX64 = the aggregation reads its records with 64-bit
 * indices, the path of runs whose cells reach past record 2^32 (tests).
 * Fault injection (an error, never a wrong result):
 * SYZSIG_DEBUG_POLL_FAIL = the sequential Poll loop (syzsig_manager_poll_batch's
 * exact fallback) fails with SYZSIG_EIO before its last poll, so tests can
 * check that a failed batch leaves every set as it was. */
#define SYZSIG_DEBUG_FIN_DEFER 32u
#define SYZSIG_DEBUG_MIN_ATOMIC 64u
#define SYZSIG_DEBUG_EXACT_CELLS 128u
#define SYZSIG_DEBUG_CAP_SPILL 256u
#define SYZSIG_DEBUG_RECS_GATE 512u
#define SYZSIG_DEBUG_EDGE_MARKALL 1024u
#define SYZSIG_DEBUG_EDGE_PASSES 2048u
#define SYZSIG_DEBUG_POLL_FAIL 4096u
#define SYZSIG_DEBUG_AGG_IDX64 8192u
int syzsig_ctx_set_debug(syzsig_ctx* ctx, uint32_t flags);

/* ---- pkg/signal/signal.go ---- */

/* make(Signal, hint): an empty, non-nil Signal. */
int syzsig_set_make(syzsig_ctx* ctx, uint64_t hint, syzsig_set** out);
void syzsig_set_free(syzsig_set* s);
/* Deep copy (Go copies alias; this is for callers that need a snapshot). */
int syzsig_set_clone(syzsig_ctx* ctx, const syzsig_set* s, syzsig_set** out);
/* Make s empty keeping its storage (grabNewSignal's `fuzzer.newSignal = nil`,
 * syz-fuzzer/fuzzer.go:478-486, without a free/alloc round trip). */
int syzsig_set_clear(syzsig_ctx* ctx, syzsig_set* s);
/* Copy src's contents over dst (same capacity required); for snapshot/restore. */
int syzsig_set_copy_from(syzsig_ctx* ctx, syzsig_set* dst, const syzsig_set* src);
/* Restore dst to the snapshot src it was copied from, given `keys`: a set
 * holding every element whose slot in dst changed since (the newSignal of the
 * batches triaged since, when it was empty at the snapshot).  Only those slots
 * are copied back, so the cost follows the changes, not the table.  Same
 * capacity required (SYZSIG_EINVAL if dst grew).  Stream-ordered. */
int syzsig_set_restore_keys(syzsig_ctx* ctx, syzsig_set* dst, const syzsig_set* src, const syzsig_set* keys);
/* Grow s (if needed) so that `extra` more elements fit under the default load
 * policy -- what a triage call reserves for its worst case; a caller that
 * keeps a snapshot of a set reserves the snapshot alike to keep capacities
 * equal (syzsig_set_restore_keys). */
int syzsig_set_reserve(syzsig_ctx* ctx, syzsig_set* s, uint64_t extra);
/* *equal = 1 iff a and b have the same capacity, length and slot words. */
int syzsig_set_equal(syzsig_ctx* ctx, const syzsig_set* a, const syzsig_set* b, int* equal);
/* Len / Empty, signal.go:23-29. */
uint64_t syzsig_len(const syzsig_set* s);
int syzsig_empty(const syzsig_set* s);
/* Capacity in slots (diagnostics, bench accounting). */
uint64_t syzsig_capacity(const syzsig_set* s);

/* FromRaw, signal.go:31-40 (NULL when n == 0). */
int syzsig_from_raw(syzsig_ctx* ctx, const uint32_t* raw, uint64_t n, uint8_t prio, syzsig_set** out);
/* Serialize, signal.go:42-57.  Order is unspecified (Go: map order).  Writes
 * min(cap, Len) entries and sets *n_out = Len. */
int syzsig_serialize(syzsig_ctx* ctx, const syzsig_set* s, uint32_t* elems, int8_t* prios,
                     uint64_t cap, uint64_t* n_out);
/* Serialize of many sets at once (the manager serializes every Poll reply,
 * manager.go:1049 r.MaxSignal = f.newMaxSignal.Serialize()): one round of
 * kernels and one copy for all of them.  offs[0..nsets] = the sets' Len
 * prefix sums (a NULL set is empty); set i's entries land in
 * elems/prios[offs[i], offs[i+1]).  cap == 0 fills offs only (sizing); a cap
 * below offs[nsets] is SYZSIG_ERANGE. */
int syzsig_serialize_batch(syzsig_ctx* ctx, const syzsig_set* const* sets, uint64_t nsets, uint32_t* elems,
                           int8_t* prios, uint64_t cap, uint64_t* offs);
/* Deserialize, signal.go:59-71: SYZSIG_ECORRUPT if n_elems != n_prios; NULL
 * when empty; a later duplicate element overwrites an earlier one. */
int syzsig_deserialize(syzsig_ctx* ctx, const uint32_t* elems, uint64_t n_elems, const int8_t* prios,
                       uint64_t n_prios, syzsig_set** out);
/* Same, elems/prios already in device memory. */
int syzsig_deserialize_dev(syzsig_ctx* ctx, const uint32_t* d_elems, const int8_t* d_prios, uint64_t n,
                           syzsig_set** out);
/* Diff, signal.go:73-88 (s may be NULL). */
int syzsig_diff(syzsig_ctx* ctx, const syzsig_set* s, const syzsig_set* s1, syzsig_set** out);
/* DiffRaw, signal.go:90-102 (prio compared as int8). */
int syzsig_diff_raw(syzsig_ctx* ctx, const syzsig_set* s, const uint32_t* raw, uint64_t n, uint8_t prio,
                    syzsig_set** out);
/* Intersection, signal.go:104-115: NULL if s1 empty, else non-nil (maybe empty). */
int syzsig_intersection(syzsig_ctx* ctx, const syzsig_set* s, const syzsig_set* s1, syzsig_set** out);
/* (*Signal).Merge, signal.go:117-131: max prio; allocates *s if NULL. */
int syzsig_merge(syzsig_ctx* ctx, syzsig_set** s, const syzsig_set* s1);

/* Minimize, signal.go:133-166.  Contexts as Serial arrays: context i owns
 * elems/prios[ctx_off[i] .. ctx_off[i+1]) (elements distinct within a context,
 * as Serialize produces).  Sort order is (Len desc, index asc) -- a fixed
 * instance of the reference's unstable sort.Slice.  Writes the indices of the
 * surviving contexts, ascending, to out_idx (capacity nctx); *n_out = count.
 * hint_distinct: expected distinct elements (e.g. corpusSignal.Len()), or 0. */
int syzsig_minimize(syzsig_ctx* ctx, const uint64_t* ctx_off, const uint32_t* elems, const int8_t* prios,
                    uint64_t nctx, uint64_t hint_distinct, uint64_t* out_idx, uint64_t* n_out);
/* Same over device arrays; d_keep[i] = 1 iff context i survives. */
int syzsig_minimize_dev(syzsig_ctx* ctx, const uint64_t* d_ctx_off, const uint32_t* d_elems,
                        const int8_t* d_prios, uint64_t nctx, uint64_t hint_distinct, uint8_t* d_keep,
                        uint64_t* n_out);

/* ---- syz-manager/manager.go:1027-1052 Manager.Poll, over a batch of polls ----
 * Poll i (arrival order) comes from fuzzer poll_fuzzer[i] (< nfuzzers) with the
 * Serial a.MaxSignal = elems/prios[poll_off[i] .. poll_off[i+1]) (Deserialize
 * rules, signal.go:59-71: a later duplicate overwrites).  The result is the
 * reference's sequential loop over the polls:
 *   newMax := maxSignal.Diff(Deserialize(a.MaxSignal)); maxSignal.Merge(newMax);
 *   every other fuzzer's newMaxSignal.Merge(newMax);
 *   reply = the polling fuzzer's newMaxSignal, which becomes nil.
 * new_max[g] = fuzzer g's newMaxSignal (NULL = nil): a polling fuzzer's set is
 * freed (nil) and may be replaced by a new one.  replies[i] = poll i's
 * r.MaxSignal as a set (NULL = empty Serial) for the caller to Serialize and
 * free.  Host arrays (the RPC payloads).
 * Limits of one call (SYZSIG_ERANGE, nothing touched): npolls + nfuzzers <
 * 2^24 - 1, npolls * nfuzzers <= 2^28, total entries * nfuzzers <= 2^31.  A
 * caller splits a larger batch into consecutive calls (the loop is sequential,
 * so that is the same result: signal.py manager_poll does).  A call of more
 * than 2^23 entries, or whose entries crowd one element partition past 2048
 * (a hot element in thousands of polls), runs the reference loop poll by poll
 * over the set ops instead of the batch kernels (same result, slower). */
int syzsig_manager_poll_batch(syzsig_ctx* ctx, syzsig_set** max_signal, syzsig_set** new_max, uint32_t nfuzzers,
                              const uint32_t* poll_fuzzer, const uint64_t* poll_off, const uint32_t* elems,
                              const int8_t* prios, uint32_t npolls, syzsig_set** replies);

/* ---- syz-manager/manager.go:976-1025 Manager.NewInput, over a batch of inputs ----
 * Row i (arrival order) is one RPC's a.RPCInput: its Serial a.Signal =
 * elems/prios[sig_off[i] .. sig_off[i+1]) (Deserialize rules: a later duplicate
 * overwrites), its a.Cover = cover[cover_off[i] .. cover_off[i+1]), and
 * input_key[i] < nkeys a dense index of hash.String(a.Prog) (syzsig_hash_dev
 * and syzsig_number_sigs_dev give it for a batch).  The result is the reference's loop over the rows under mgr.mu:
 *   inputSignal := a.Signal.Deserialize()
 *   if corpusSignal.Diff(inputSignal).Empty() return          (:993: rejected)
 *   corpusSignal.Merge(inputSignal); corpusCover.Merge(a.Cover)   (:997-998)
 *   if the program is in the corpus: its entry's Signal is max-merged with
 *   inputSignal and its Cover united with a.Cover (:1000-1008), else the input
 *   becomes the entry (:1009-1022).
 * An old corpus entry the batch may touch is passed as an ordinary row before
 * its key's inputs, flagged SYZSIG_INPUT_PRESENT (its stored Signal and Cover):
 * it takes no part in acceptance and does not go into corpusSignal or
 * corpusCover; it counts as accepted for its key's merge and makes later rows
 * of the key "not new".
 * Outputs (host arrays):
 *  - accepted[i] = 1 iff row i passed :993 (a PRESENT row: 1);
 *  - new_key[i] = 1 iff row i is an accepted non-PRESENT row and no earlier
 *    accepted or PRESENT row has its key (the else branch at :1009: the caller
 *    saves it and queues it for the other fuzzers);
 *  - key_touched[k] = 1 iff key k has an accepted non-PRESENT row.  Only such
 *    keys get CSR ranges: key k's entry Signal -- the max-merge of the
 *    Deserialized Signals of its PRESENT and accepted rows -- at
 *    key_elems/key_prios[key_sig_off[k] .. key_sig_off[k+1]), elements ascending,
 *    and its Cover, the union of the same rows' covers, at
 *    key_cover[key_cover_off[k] .. key_cover_off[k+1]), PCs ascending and
 *    distinct (one fixed instance of Serialize's map order; the old entry keeps
 *    its Call and Prog).  Both offset arrays have nkeys + 1 entries.
 * *corpus_signal / *corpus_cover: a NULL one is allocated by the first accepted
 * input (the cover even when that input's cover is empty, cover.go:9-18); a
 * batch that accepts nothing leaves NULL sets NULL.
 * All or nothing: sig_cap below the rows' total entries or cover_cap below
 * their total PCs is SYZSIG_ERANGE (those totals always suffice), a key >=
 * nkeys or a non-monotone offset SYZSIG_EINVAL, both checked before anything
 * is touched; on any error the sets and the output arrays are as they were.
 * A batch of more than 2^23 non-PRESENT entries, or whose entries crowd one
 * element partition past 2048 (an element present in thousands of inputs),
 * takes the reference loop input by input over the set ops for acceptance
 * (same result, slower).  A key's rows hold fewer than 2^32 entries and fewer
 * than 2^31 PCs (SYZSIG_ERANGE).
 * SYZSIG_CORPUS_TILE: a key whose rows hold at most this many entries is
 * sorted by one workgroup pass in LDS; a longer one is tile-sorted and
 * rank-merged through workspace buffers (its cover alike past
 * SYZSIG_COVER_TILE PCs). */
#define SYZSIG_INPUT_PRESENT 1u
#define SYZSIG_CORPUS_TILE 2048
int syzsig_manager_new_input_batch(syzsig_ctx* ctx, syzsig_set** corpus_signal, syzsig_set** corpus_cover,
                                   uint32_t ninputs, uint32_t nkeys, const uint32_t* input_key,
                                   const uint8_t* input_flags, const uint64_t* sig_off, const uint32_t* elems,
                                   const int8_t* prios, const uint64_t* cover_off, const uint32_t* cover,
                                   uint8_t* accepted, uint8_t* new_key, uint8_t* key_touched, uint64_t* key_sig_off,
                                   uint32_t* key_elems, int8_t* key_prios, uint64_t sig_cap, uint64_t* key_cover_off,
                                   uint32_t* key_cover, uint64_t cover_cap);
/* Which paths the context's last syzsig_manager_new_input_batch took (tests,
 * tuning; results never depend on them): out[0] = 1 when acceptance ran the
 * sequential loop, out[1] = keys whose entries exceeded SYZSIG_CORPUS_TILE,
 * out[2] = the rank-merge passes over them, out[3] = keys whose cover exceeded
 * SYZSIG_COVER_TILE. */
int syzsig_new_input_stats(syzsig_ctx* ctx, uint64_t out[4]);

/* Minimize sharded by element (one process per GPU): shard `shard` of
 * `nshards` takes only the entries whose element it owns (owner_of, as the
 * sharded maxSignal) over the whole corpus description (same ctx_off order on
 * every shard); d_keep[i] = 1 iff context i wins one of the shard's elements.
 * The OR (max) of d_keep over the shards is syzsig_minimize_dev's d_keep:
 * an element's winner depends on that element's entries only.  *n_out = the
 * shard's count. */
int syzsig_minimize_shard_dev(syzsig_ctx* ctx, const uint64_t* d_ctx_off, const uint32_t* d_elems,
                              const int8_t* d_prios, uint64_t nctx, uint32_t nshards, uint32_t shard,
                              uint64_t hint_distinct, uint8_t* d_keep, uint64_t* n_out);

/* Minimize split by data (one process per GPU): part `part` of
 * `nparts` takes a contiguous range of the contexts in sort order (Len desc,
 * index asc), cut at about total/nparts entries per part, and reads only those
 * contexts' entries.  It aggregates them per element and writes one winner
 * record per distinct element of its range,
 *     e << 32 | (prio ^ 0x80) << 24 | (0xFFFFFF - rank)
 * (rank = the context's position in the global sort order; the max of the low
 * 32 bits over the parts is argmax (prio, -rank), the reference's winner),
 * grouped by owner_of(e, nshards) into d_send (send_cap >= the part's entries
 * suffices); send_counts[g] = records for owner g, packed at their exclusive
 * prefix sum.  nshards <= 64; at most 4 distinct prios per part. */
int syzsig_minimize_split_dev(syzsig_ctx* ctx, const uint64_t* d_ctx_off, const uint32_t* d_elems,
                              const int8_t* d_prios, uint64_t nctx, uint32_t nparts, uint32_t part, uint32_t nshards,
                              uint64_t hint_distinct, uint64_t* d_send, uint64_t send_cap, uint64_t* send_counts);
/* Owner side of the split: the winner records every part sent to this owner
 * (d_recs, any order) -> the max per element -> d_keep[i] = 1 iff context i
 * wins one of them.  The OR (max) of d_keep over the owners is
 * syzsig_minimize_dev's d_keep; *n_out = this owner's count. */
int syzsig_minimize_resolve_dev(syzsig_ctx* ctx, const uint64_t* d_ctx_off, uint64_t nctx, const uint64_t* d_recs,
                                uint64_t nrec, uint8_t* d_keep, uint64_t* n_out);

/* ---- pkg/cover/cover.go:7-30: type Cover map[uint32]struct{} ----
 * A Cover is a syzsig_set whose entries all carry prio 0.  Merge(raw)
 * (cover.go:9-18) allocates a NULL *cov even when n == 0, then inserts every
 * PC (manager corpusCover.Merge, syz-manager/manager.go:998).  Len is
 * syzsig_len; Serialize (cover.go:20-26) is syzsig_serialize's elems. */
int syzsig_cover_merge(syzsig_ctx* ctx, syzsig_set** cov, const uint32_t* raw, uint64_t n);
int syzsig_cover_merge_dev(syzsig_ctx* ctx, syzsig_set** cov, const uint32_t* d_raw, uint64_t n);

/* ---- syz-fuzzer/proc.go:107-140 triageInput signal re-runs, over a batch ----
 * Item i's newSignal (corpusSignalDiff of its input signal, serialized) is
 * elems/prios[item_off[i] .. item_off[i+1]); item_flags[i] = SYZSIG_TRIAGE_*.
 * Item i's re-runs are r = i*runs .. i*runs+runs-1 (runs = signalRuns, <= 8):
 * run r's raw signal is run_sigs[run_off[r] .. run_off[r+1]) with
 * run_prio[r] = signalPrio, run_errno[r] = its Errno, run_exec[r] = 0 when
 * len(info) == 0.  Applies the loop of proc.go:119-139 (skip and count runs
 * that did not execute or failed; newSignal = newSignal.Intersection(run);
 * drop the item when it empties unless minimized, or after more than
 * runs/2+1 skipped runs).  Writes item_keep[i] (1 = the item goes on to
 * minimization and the corpus) and elem_keep[j] (1 = element j is in the
 * item's final newSignal).  All pointers are device pointers. */
#define SYZSIG_TRIAGE_MINIMIZED 1 /* item.flags & ProgMinimized */
#define SYZSIG_TRIAGE_ORIG_OK 2   /* item.info.Errno == 0 */
int syzsig_triage_runs_dev(syzsig_ctx* ctx, const uint64_t* d_item_off, uint64_t nitems, const uint32_t* d_elems,
                           const int8_t* d_prios, const uint8_t* d_item_flags, uint32_t runs,
                           const uint64_t* d_run_off, const uint32_t* d_run_sigs, const uint8_t* d_run_prio,
                           const int32_t* d_run_errno, const uint8_t* d_run_exec, uint8_t* d_item_keep,
                           uint8_t* d_elem_keep);

/* The minimize predicate of triageInput (proc.go:141-160) over a batch:
 * same item/run layout as syzsig_triage_runs_dev, with `attempts` runs per
 * item (minimizeAttempts).  pred[i] = 1 iff, going through the attempts in
 * order and skipping ones that did not execute or have no signal, an attempt
 * keeps all of newSignal (newSignal.Intersection(thisSignal).Len() ==
 * newSignal.Len()) before one fails after a successful original. */
int syzsig_minimize_pred_dev(syzsig_ctx* ctx, const uint64_t* d_item_off, uint64_t nitems, const uint32_t* d_elems,
                             const int8_t* d_prios, const uint8_t* d_item_flags, uint32_t attempts,
                             const uint64_t* d_run_off, const uint32_t* d_run_sigs, const uint8_t* d_run_prio,
                             const int32_t* d_run_errno, const uint8_t* d_run_exec, uint8_t* d_pred);

/* ---- syz-fuzzer/fuzzer.go:494-511 checkNewSignal (+ signalPrio :513-521 by caller) ----
 * One program's CallInfo signals in host memory: call i's raw signal is
 * sigs[call_start[i] .. +call_len[i]) with prio call_prio[i].  Sequential over
 * calls as the reference: call i sees merges of calls < i.  Writes indices of
 * calls with new signal to out_calls (capacity ncalls), *n_out = count;
 * merges into *max_signal and *new_signal (allocating NULL ones).
 * new_bits (optional, ceil(nrec/32) words): bit r set iff sigs[r] is in its
 * call's DiffRaw result. */
int syzsig_check_new_signal(syzsig_ctx* ctx, syzsig_set** max_signal, syzsig_set** new_signal,
                            const uint32_t* sigs, uint64_t nrec, const uint64_t* call_start,
                            const uint32_t* call_len, const uint8_t* call_prio, uint32_t ncalls,
                            uint32_t* out_calls, uint32_t* n_out, uint32_t* new_bits);

/* ---- batch triage (device pointers): checkNewSignal over a whole batch ----
 * Serial order = call index order (program-major, call-minor).  Call ranges
 * [call_start, call_start+call_len) must lie inside [0, nrec) and be disjoint.
 * Outputs:
 *  - call_new[c] = 1 iff call c's DiffRaw is non-empty (checkNewSignal's
 *    `calls`, syz-fuzzer/fuzzer.go:498-503);
 *  - new_pairs (optional): every call's DiffRaw result as (call << 32 | elem),
 *    one entry per distinct (call, elem), in unspecified order; at most
 *    new_pairs_cap are written, stats.new_pairs = the total;
 *  - new_bits (optional, NULL = not computed): bit r = record r's element is in
 *    its call's DiffRaw result (every duplicate occurrence is marked).
 * call_new / new_bits are zeroed by the call. */
typedef struct {
	const uint32_t* sigs;       /* nrec raw signal elements */
	const uint64_t* call_start; /* ncalls */
	const uint32_t* call_len;   /* ncalls */
	const uint8_t* call_prio;   /* ncalls, signalPrio values */
	uint64_t ncalls;
	uint64_t nrec;
	uint32_t* new_bits;         /* out (optional): ceil(nrec/32) words, bit r = record r is new */
	uint8_t* call_new;          /* out: ncalls, 1 = call has new signal */
	uint64_t* new_pairs;        /* out (optional): call << 32 | elem per DiffRaw entry */
	uint64_t new_pairs_cap;     /* capacity of new_pairs in entries */
} syzsig_batch;

typedef struct {
	uint64_t records;        /* records processed */
	uint64_t survivors;      /* per-call path: records past the home-bucket filter; aggregation path: distinct elements */
	uint64_t candidates;     /* per-call path: records past the prio filter; aggregation path: = changed */
	uint64_t changed;        /* elements whose maxSignal prio changed (incl. new) */
	uint64_t inserted;       /* elements new to maxSignal */
	uint64_t new_signal_len; /* Len of *new_signal after the batch */
	uint64_t retries;        /* capacity-overflow restarts */
	uint64_t runs;           /* sub-batches (one per <=4 distinct prios) */
	uint64_t parts;          /* aggregation partitions of the last run (0 = per-call path) */
	uint64_t distinct;       /* distinct elements aggregated (aggregation path) */
	uint64_t overflow_parts; /* partitions redone in the HBM table (LDS table too small) */
	uint64_t new_pairs;      /* DiffRaw entries over all calls (see syzsig_batch.new_pairs) */
	double part_ms;          /* device time of record partitioning (0 unless timing enabled) */
	double probe_ms;         /* device time of the probe kernel(s) (0 unless timing enabled) */
	double decide_ms;        /* device time of the decide kernel(s) (0 unless timing enabled) */
} syzsig_batch_stats;

int syzsig_triage_batch(syzsig_ctx* ctx, syzsig_set* max_signal, syzsig_set** new_signal,
                        const syzsig_batch* b, syzsig_batch_stats* stats);

/* ---- executor/executor.h:492-528 + :677-706 on device (K1 edge + K2 dedup) ----
 * Raw KCOV traces for nprog programs; program p owns calls
 * [prog_call[p], prog_call[p+1]); call c's PCs are pcs[call_start[c] .. +call_len[c])
 * (call_len < 262144, executor_linux.cc:186-187).  Each program runs with a
 * fresh 8192-slot dedup table shared by its calls in order, like one forked
 * executor child.  Call c's emitted signals land at sigs[call_start[c] ..
 * +sig_cnt[c]); completed[p] = calls whose record was published (a PC failing
 * cover_check aborts the rest of the program); later calls get sig_cnt = 0.
 * d_sigs has npc entries (same indexing as d_pcs). */
int syzsig_edge_derive_dev(syzsig_ctx* ctx, const uint64_t* d_pcs, uint64_t npc, const uint64_t* d_call_start,
                           const uint32_t* d_call_len, uint64_t ncalls, const uint32_t* d_prog_call,
                           uint64_t nprog, uint32_t* d_sigs, uint32_t* d_sig_cnt, uint32_t* d_completed);

/* ---- executor/executor.h:514-527 on device: the call's cover output ----
 * The second half of write_coverage_signal over the traces of
 * syzsig_edge_derive_dev (same d_pcs .. nprog arguments and limits), with
 * flag_collect_cover on.  d_completed (required) is what syzsig_edge_derive_dev
 * wrote for the same traces: call c of program p has a cover record iff
 * c - prog_call[p] < completed[p]; the aborting call and every later one get
 * cover_cnt = 0 and nothing written (doexit(0) precedes any cover write).
 * flags: SYZSIG_COVER_DEDUP = flag_dedup_cover, the PCs sorted ascending and
 * made unique before the truncation to u32 (the fuzzer's triage executions,
 * proc.go:49-50, :250); without it the truncated PCs in trace order,
 * cover_cnt = call_len.  Call c's cover lands at d_cover[call_start[c] ..
 * +cover_cnt[c]) (d_cover has npc entries, indexed like d_pcs; words outside
 * those ranges are left alone); d_cover_cnt has ncalls entries.  Rejects
 * (SYZSIG_EINVAL, nothing written) NULL arguments, a call_len >= 262144, a
 * range outside [0, npc), and a completed[p] above program p's calls.
 * SYZSIG_COVER_TILE: a segment of at most this many keys is sorted in LDS by
 * one workgroup; a longer one goes through the context's workspace in HBM. */
#define SYZSIG_COVER_DEDUP 1u
#define SYZSIG_COVER_TILE 4096
int syzsig_edge_cover_dev(syzsig_ctx* ctx, const uint64_t* d_pcs, uint64_t npc, const uint64_t* d_call_start,
                          const uint32_t* d_call_len, uint64_t ncalls, const uint32_t* d_prog_call, uint64_t nprog,
                          const uint32_t* d_completed, uint32_t flags, uint32_t* d_cover, uint32_t* d_cover_cnt);

/* ---- the KCOV target of the two functions above ----
 * The reference instantiates write_coverage_signal<cover_t> twice
 * (executor.h:595-598): <uint64> for a 64-bit kernel and <uint32> for a 32-bit
 * one (KCOV_INIT_TRACE32, executor_linux.cc:143-146, :255-275), and its
 * cover_check is the x86 text range only for a uint64 PC in a Linux executor
 * built for i386 / x86_64 (executor_linux.cc:196-204); cover_check(uint32), and
 * cover_check(uint64) of every other build (arm64, ppc64le, executor_bsd.cc:
 * 223-231, executor_fuchsia.cc:59-67, akaros, windows) is `return true`.
 * `target` names one of those three:
 *   0                          u64 PCs, no check;
 *   SYZSIG_TARGET_PC32         u32 PCs (d_pcs is const uint32_t*, npc and
 *                              call_start count u32 words), no check;
 *   SYZSIG_TARGET_CHECK_X86    u64 PCs, the x86 range: syzsig_edge_derive_dev
 *                              and syzsig_edge_cover_dev (= SYZSIG_TARGET_LINUX_AMD64).
 * SYZSIG_TARGET_PC32 | SYZSIG_TARGET_CHECK_X86 (the reference has no such
 * executor) and any other bit are SYZSIG_EINVAL, nothing written.  Every other
 * argument, limit and result is that of the function without `_target`.
 * Signals depend on a PC's low 32 bits only (hash, dedup and write_output take
 * uint32), so the three targets differ in what is loaded and in whether a PC
 * can abort its program.  The cover output differs more with
 * SYZSIG_COVER_DEDUP: std::sort + std::unique run on cover_t (executor.h:
 * 518-522) before the truncation, so under target 0 the u32 output is ordered
 * by the u64 PCs and holds a low word once per distinct u64 PC (PCs
 * 0x100000009, 0x200000003 give 9, 3); under SYZSIG_TARGET_PC32 it is the
 * ascending distinct u32 PCs; under SYZSIG_TARGET_CHECK_X86 every upper word is
 * 0xffffffff and the two coincide. */
#define SYZSIG_TARGET_PC32 1u
#define SYZSIG_TARGET_CHECK_X86 2u
#define SYZSIG_TARGET_LINUX_AMD64 SYZSIG_TARGET_CHECK_X86
int syzsig_edge_derive_target_dev(syzsig_ctx* ctx, const void* d_pcs, uint64_t npc, const uint64_t* d_call_start,
                                  const uint32_t* d_call_len, uint64_t ncalls, const uint32_t* d_prog_call,
                                  uint64_t nprog, uint32_t target, uint32_t* d_sigs, uint32_t* d_sig_cnt,
                                  uint32_t* d_completed);
int syzsig_edge_cover_target_dev(syzsig_ctx* ctx, const void* d_pcs, uint64_t npc, const uint64_t* d_call_start,
                                 const uint32_t* d_call_len, uint64_t ncalls, const uint32_t* d_prog_call,
                                 uint64_t nprog, const uint32_t* d_completed, uint32_t flags, uint32_t target,
                                 uint32_t* d_cover, uint32_t* d_cover_cnt);

/* ---- syz-fuzzer/proc.go:139 inputCover.Merge(inf.Cover) and :173 Cover:
 * inputCover.Serialize(), over the item / run layout of syzsig_triage_runs_dev ----
 * Run r = i * runs + k of item i has the cover list d_cover[run_cover_start[r]
 * .. +run_cover_len[r]) (ranges inside one u32 buffer of ncover words: the
 * output of syzsig_edge_cover_dev, or the executor regions with the
 * cover_start / cover_len of syzsig_ingest_exec_output_dev).  Item i's
 * inputCover is the set union of the lists of its runs that the loop did not
 * skip (a run is skipped when run_exec == 0, its signal is empty --
 * run_off[r + 1] == run_off[r], the only use of d_run_off -- or
 * SYZSIG_TRIAGE_ORIG_OK is set and run_errno != 0; proc.go:122-123), and empty
 * when item_keep[i] == 0 (as syzsig_triage_runs_dev wrote it: every `return`
 * of the loop precedes :173).  Item i's PCs are written sorted ascending (one
 * fixed instance of Serialize's map order) to
 * d_item_cover[item_cover_off[i] .. item_cover_off[i + 1]); item_cover_off has
 * nitems + 1 entries; *n_out = the total.  If it exceeds cap (the capacity of
 * d_item_cover in entries) nothing is written: SYZSIG_ERANGE with the needed
 * total in *n_out.  An item's merged lists hold fewer than 2^31 PCs
 * (SYZSIG_ERANGE); a cover range outside [0, ncover) is SYZSIG_EINVAL. */
int syzsig_triage_cover_dev(syzsig_ctx* ctx, uint64_t nitems, uint32_t runs, const uint8_t* d_item_flags,
                            const uint8_t* d_item_keep, const uint64_t* d_run_off, const int32_t* d_run_errno,
                            const uint8_t* d_run_exec, const uint32_t* d_cover, uint64_t ncover,
                            const uint64_t* d_run_cover_start, const uint32_t* d_run_cover_len,
                            uint64_t* d_item_cover_off, uint32_t* d_item_cover, uint64_t cap, uint64_t* n_out);

/* ---- syz-fuzzer/proc.go:232-245 and :107-111: a batch's triage items, their
 * inputSignal and newSignal ----
 * The step between syzsig_triage_batch and syzsig_triage_runs_dev.  The batch
 * is d_sigs / nrec / d_call_start / d_call_len / d_call_prio / ncalls as
 * syzsig_triage_batch took them, d_call_new (an input here) what it wrote:
 * every call with call_new != 0 is one WorkTriage (proc.go:232-245).  Item i is
 * the i-th such call in ascending call index, the order execute enqueues them
 * in; *n_items = their number.  corpus_signal = fuzzer.corpusSignal (NULL = nil:
 * everything is new).  All array pointers are device pointers.  Per item:
 *  - d_item_call[i] = its call, d_item_prio[i] = (int8)call_prio[call], as
 *    FromRaw casts signalPrio's value (signal.go:35);
 *  - inputSignal = FromRaw(item.info.Signal, prio) (:107) as CSR: the call's
 *    distinct elements, ascending (one fixed instance of Serialize's map
 *    order), at d_input_elems[input_off[i] .. input_off[i + 1]); every one
 *    carries d_item_prio[i].  input_off / input_elems / item_prio are
 *    RPCInput.Signal (:172) and what syzsig_corpus_add_inputs_dev takes;
 *  - newSignal = corpusSignal.Diff(inputSignal) (:108, signal.go:73-88) as CSR,
 *    exactly what syzsig_triage_runs_dev reads: the elements e of inputSignal
 *    except those that corpusSignal holds with corpus[e] >= item_prio[i]
 *    (compared as int8), ascending, at d_elems / d_prios[item_off[i] ..
 *    item_off[i + 1]).  An item with nothing new keeps an empty range, which
 *    syzsig_triage_runs_dev drops as :109-111 does.
 * A flagged call of no records gives two empty ranges (FromRaw of an empty
 * slice is nil, Diff of nil is nil).  Both offset arrays have n_items + 1
 * entries (item_cap + 1 as capacity).
 * Batch semantics: every item's Diff is against corpusSignal as passed in --
 * the interleaving in which every Proc reaches :108 before any reaches :176
 * (the three re-executions lie between).  One item per call gives the strictly
 * sequential order.
 * Capacities: item_cap (items), input_cap (entries of d_input_elems), new_cap
 * (entries of d_elems / d_prios).  The three needed totals always go to
 * *n_items / *n_input / *n_new; if one exceeds its capacity nothing is written
 * to any output array and the result is SYZSIG_ERANGE: grow and call again.
 * SYZSIG_EINVAL (nothing written): a NULL required argument, a call range
 * outside [0, nrec).  SYZSIG_ERANGE: a flagged call of 2^31 or more records,
 * 2^32 or more calls.
 * SYZSIG_ITEMS_TILE: a call of at most this many records is sorted in LDS by
 * one workgroup; a longer one is tile-sorted and rank-merged through the
 * context's workspace in HBM. */
#define SYZSIG_ITEMS_TILE 4096
int syzsig_triage_items_dev(syzsig_ctx* ctx, const uint32_t* d_sigs, uint64_t nrec, const uint64_t* d_call_start,
                            const uint32_t* d_call_len, const uint8_t* d_call_prio, uint64_t ncalls,
                            const uint8_t* d_call_new, const syzsig_set* corpus_signal, uint32_t* d_item_call,
                            int8_t* d_item_prio, uint64_t item_cap, uint64_t* d_input_off, uint32_t* d_input_elems,
                            uint64_t input_cap, uint64_t* d_item_off, uint32_t* d_elems, int8_t* d_prios,
                            uint64_t new_cap, uint64_t* n_items, uint64_t* n_input, uint64_t* n_new);
/* Which paths the context's last syzsig_triage_items_dev took (tests, tuning;
 * results never depend on them): out[0] = items, out[1] = items longer than
 * SYZSIG_ITEMS_TILE, out[2] = the rank-merge passes over them, out[3] = probes
 * of corpusSignal (one per distinct element of an item; 0 for a nil set). */
int syzsig_triage_items_stats(syzsig_ctx* ctx, uint64_t out[4]);

/* ---- syz-fuzzer/fuzzer.go:446-460 addInputToCorpus, over the items that
 * triageInput kept ----
 * d_input_off / d_input_elems / d_item_prio as syzsig_triage_items_dev wrote
 * them (n_items items, n_input = the entries of d_input_elems: a range that is
 * reversed or ends past it is SYZSIG_EINVAL); d_item_keep[i] != 0 = item i
 * reached :176 (NULL = all; syzsig_triage_runs_dev's item_keep and the caller's
 * minimization decide).  For every kept item whose sign is not empty (:454):
 * corpusSignal.Merge(sign); maxSignal.Merge(sign) (:456-457).  Max-merge
 * commutes, so the batch is the sequential loop exactly.  A NULL *corpus_signal
 * or *max_signal is nil and is allocated only if some kept item is non-empty
 * (signal.go:117-131).  Room is reserved in both tables before the one launch
 * that commits; an error before it leaves both sets' contents (and NULL sets
 * NULL) as they were.  The two sets must be distinct (SYZSIG_EINVAL). */
int syzsig_corpus_add_inputs_dev(syzsig_ctx* ctx, const uint64_t* d_input_off, const uint32_t* d_input_elems,
                                 uint64_t n_input, const int8_t* d_item_prio, uint64_t n_items,
                                 const uint8_t* d_item_keep, syzsig_set** corpus_signal, syzsig_set** max_signal);

/* ---- syz-fuzzer/fuzzer.go:344-350: what the fuzzer does with the reply to its
 * poll, over a batch of Serials ----
 * Segment s is one Serial, d_elems / d_prios[seg_off[s] .. seg_off[s + 1]) (a
 * range that is reversed or ends past n_entries is SYZSIG_EINVAL), in arrival
 * order, with d_seg_kind[s]:
 *  - SYZSIG_SEG_MAXSIGNAL: r.MaxSignal.  D = Deserialize(segment) (:344); if
 *    D.Len() != 0, maxSignal.Merge(D) (addMaxSignal, :468-475);
 *  - SYZSIG_SEG_INPUT: the Signal of one of r.NewInputs (at most 100 per poll,
 *    syz-manager/manager.go:1053-1057).  D = Deserialize(segment)
 *    (addInputFromAnotherFuzzer, :433-444); if !D.Empty(),
 *    corpusSignal.Merge(D); maxSignal.Merge(D) (addInputToCorpus, :446-460).
 * Deserialize (signal.go:58-71) assigns entry after entry, so D[e] is the prio
 * of the LAST entry of e inside that segment, also when an earlier one is
 * higher; prios are int8 and Merge keeps the maximum.  Max-merge commutes and
 * is idempotent, so the batch is the sequential loop exactly, for the replies
 * of any number of polls in one call.  A NULL *corpus_signal or *max_signal is
 * nil and is allocated only if a non-empty segment reaches it (signal.go:
 * 117-131): a batch of MAXSIGNAL segments leaves a nil corpusSignal nil.
 * All or nothing: the segments are checked first, and room is reserved in both
 * tables before the launches that commit; an error before them leaves both
 * sets' contents (and NULL sets NULL) as they were.  The two sets must be
 * distinct (SYZSIG_EINVAL); a kind above SYZSIG_SEG_INPUT is SYZSIG_EINVAL, a
 * segment of 2^31 or more entries or 2^32 or more segments SYZSIG_ERANGE.
 * SYZSIG_POLLRES_TILE: a segment of at most this many entries is resolved by
 * one workgroup in LDS; a longer one (a Connect reply's MaxSignal) through a
 * scratch table in the context's workspace. */
#define SYZSIG_SEG_MAXSIGNAL 0u
#define SYZSIG_SEG_INPUT 1u
#define SYZSIG_POLLRES_TILE 4096
int syzsig_fuzzer_poll_res_dev(syzsig_ctx* ctx, const uint64_t* d_seg_off, const uint8_t* d_seg_kind, uint64_t nseg,
                               const uint32_t* d_elems, const int8_t* d_prios, uint64_t n_entries,
                               syzsig_set** corpus_signal, syzsig_set** max_signal);
/* Which paths the context's last syzsig_fuzzer_poll_res_dev took (tests,
 * tuning; results never depend on them): out[0] = segments resolved in LDS,
 * out[1] = segments resolved through a scratch table, out[2] = entries that
 * lost to a later entry of their element in their segment, out[3] = bytes of
 * the scratch tables. */
int syzsig_poll_res_stats(syzsig_ctx* ctx, uint64_t out[4]);

/* ---- pkg/ipc/ipc.go:328-468 readOutCoverage over a batch of executor output regions ----
 * Program p's output region (executor.h:566-604 records, the executor's shmem
 * out file) is d_out[prog_off[p] .. prog_off[p+1]); it has the calls
 * [prog_call[p], prog_call[p+1]) (len(p.Calls)), call_num[c] = the expected
 * syscall ID (c.Meta.ID; NULL = unchecked) and call_any[c] = CallContainsAny
 * (prog/any.go:177-185).  Writes per call: the Signal range inside d_out
 * (aliasing it, ipc.go:410; call_len = 0 if the call has no record), its Errno
 * (-1 = not executed), and its signalPrio (fuzzer.go:513-521); optionally the
 * Cover range.  The result feeds syzsig_triage_batch with sigs = d_out,
 * nrec = nwords.  prog_status[p] = SYZSIG_INGEST_* (the ipc.go error branch
 * hit); a failed program gets no signal (the fuzzer retries that Exec,
 * proc.go:269-278).  *n_failed (optional) = programs with status != 0.
 * Returns SYZSIG_EINVAL if an offset or call range is out of bounds. */
#define SYZSIG_INGEST_OK 0
#define SYZSIG_INGEST_ENCMD 1      /* no ncmd word (ipc.go:356-359) */
#define SYZSIG_INGEST_EHEADER 2    /* short call header (:378-383) */
#define SYZSIG_INGEST_EINDEX 3     /* callIndex >= len(p.Calls) (:384-388) */
#define SYZSIG_INGEST_ECALLNUM 4   /* callNum != c.Meta.ID (:389-395) */
#define SYZSIG_INGEST_EDOUBLE 5    /* double coverage for a call (:396-400) */
#define SYZSIG_INGEST_ESIGNAL 6    /* signalSize past the region (:403-407) */
#define SYZSIG_INGEST_ECOVER 7     /* coverSize past the region (:411-415) */
#define SYZSIG_INGEST_ECOMPS 8     /* short comparison record (:420-445) */
#define SYZSIG_INGEST_ECOMPTYPE 9  /* comparison type > compConstMask|compSizeMask (:429-433) */
#define SYZSIG_INGEST_EBOUNDS 10   /* prog_off / prog_call out of bounds (ABI check) */
int syzsig_ingest_exec_output_dev(syzsig_ctx* ctx, const uint32_t* d_out, uint64_t nwords,
                                  const uint64_t* d_prog_off, uint64_t nprog, const uint32_t* d_prog_call,
                                  uint64_t ncalls, const uint32_t* d_call_num, const uint8_t* d_call_any,
                                  uint64_t* d_call_start, uint32_t* d_call_len, uint8_t* d_call_prio,
                                  int32_t* d_call_errno, uint64_t* d_cover_start, uint32_t* d_cover_len,
                                  int32_t* d_prog_status, uint64_t* n_failed);

/* ---- comparison hints: the executor's comps output, CompMap, shrinkExpand ----
 * SYZSIG_COMPS_TILE: a segment of at most this many keys (comparison triples,
 * map pairs, replacers: 3, 2 and 1 u64 words) is sorted in LDS by one
 * workgroup, 48 KB for the triples; longer ones are tile-sorted and
 * rank-merged through workspace buffers. */
#define SYZSIG_COMPS_TILE 2048

/* executor/executor.h:576-593 handle_completion with flag_collect_comps, per
 * call of a batch.  d_comps holds ncmp KCOV_TRACE_CMP records of four u64
 * (type, arg1, arg2, pc; executor.h:155-160); call c's are the call_len[c]
 * records from record call_start[c] on.  Per call: std::sort + std::unique on
 * (type, arg1, arg2) as full u64 words (:861-875; pc takes no part), then every
 * survivor that ignore() (executor_linux.cc:221-253, the x86_64 branch included,
 * out_start = the address of the executor's output_data, kMaxOutput = 16 MB)
 * does not drop is written as write() does (:823-859): (u32)type, then the low
 * words of the operands sign-extended from the size (3 words), or lo and hi of
 * each operand for SIZE8 (5 words).  Call c's words go to d_out[5 *
 * call_start[c] ..] (d_out holds 5 * ncmp words; words outside the written
 * ranges are left alone), their number to d_out_words[c] and the number of
 * records written -- the record's comps_size -- to d_comps_cnt[c].  A call of
 * more than 65535 records (fail("too many comparisons")) or outside the buffer
 * is SYZSIG_EINVAL, checked before anything is written. */
int syzsig_exec_comps_dev(syzsig_ctx* ctx, const uint64_t* d_comps, uint64_t ncmp, const uint64_t* d_call_start,
                          const uint32_t* d_call_len, uint64_t ncalls, uint64_t out_start, uint32_t* d_out,
                          uint32_t* d_out_words, uint32_t* d_comps_cnt);

/* pkg/ipc/ipc.go:420-465: a call's comparison records parsed into its
 * prog.CompMap (CompMap.AddComp, prog/hints.go:43-48).  d_words is a buffer of
 * nwords u32 -- the output of syzsig_exec_comps_dev, or the executor regions
 * syzsig_ingest_exec_output_dev indexed (for an executed call: comps_start =
 * cover_start + cover_len, comps_cnt = d_out[call_start - 1]); call c has
 * comps_cnt[c] records from word comps_start[c] on, inside the region that ends
 * at comps_end[c] (NULL: at nwords).  d_status[c] = SYZSIG_INGEST_OK,
 * SYZSIG_INGEST_ECOMPS or SYZSIG_INGEST_ECOMPTYPE where the Go returns an error;
 * such a call gets an empty map.  The maps come back as CSR: call c's distinct
 * (key, value) pairs -- pair i = d_pairs[2 i], d_pairs[2 i + 1] -- sorted
 * ascending by key, then value (one fixed instance of the map's iteration
 * order) at pairs d_map_off[c] .. d_map_off[c + 1]; d_map_off has ncalls + 1
 * entries; *n_out = the total.  If it exceeds cap (the capacity of d_pairs in
 * pairs) nothing is written: SYZSIG_ERANGE with the needed total in *n_out.
 * A range outside the buffer or more than 65535 records in a call is
 * SYZSIG_EINVAL. */
int syzsig_comp_map_dev(syzsig_ctx* ctx, const uint32_t* d_words, uint64_t nwords, const uint64_t* d_comps_start,
                        const uint32_t* d_comps_cnt, const uint64_t* d_comps_end, uint64_t ncalls,
                        int32_t* d_status, uint64_t* d_map_off, uint64_t* d_pairs, uint64_t cap, uint64_t* n_out);

/* prog/hints.go:164-218 shrinkExpand(v, compMap) for nq queries (q_call[q],
 * q_val[q]) against the maps of syzsig_comp_map_dev (npairs = map_off[ncalls]).
 * special_ints is a host array (prog/rand.go specialInts, at most 4096 entries;
 * copied during the call).  Query q's distinct replacers come back sorted
 * ascending at d_rep[rep_off[q] .. rep_off[q + 1]); rep_off has nq + 1 entries;
 * *n_out = the total.  If it exceeds cap nothing is written: SYZSIG_ERANGE with
 * the needed total in *n_out.  A query's call outside the maps is SYZSIG_EINVAL. */
int syzsig_shrink_expand_dev(syzsig_ctx* ctx, const uint64_t* d_map_off, const uint64_t* d_pairs, uint64_t ncalls,
                             uint64_t npairs, const uint32_t* d_q_call, const uint64_t* d_q_val, uint64_t nq,
                             const uint64_t* special_ints, uint32_t nspecial, uint64_t* d_rep_off, uint64_t* d_rep,
                             uint64_t cap, uint64_t* n_out);

/* SYZSIG_HINT_LIST: the capacity of the per-arg list of (window, replacer)
 * candidates that one workgroup of syzsig_hint_mutants_dev sorts in LDS (16 B
 * each).  An arg with more accepted candidates than this, or with one lookup
 * whose key has more values than this, takes the exact fallback through the
 * internals of syzsig_shrink_expand_dev; the results do not depend on the path.
 * SYZSIG_HINT_MAX_DATA: maxDataLength, prog/hints.go:38. */
#define SYZSIG_HINT_LIST 1024
#define SYZSIG_HINT_MAX_DATA 100

/* prog/hints.go:105-132, the inner half of generateHints (:82-103) for narg
 * args of a batch against the maps of syzsig_comp_map_dev (npairs =
 * map_off[ncalls]); the caller has applied the type filter of :83-95.  Arg a
 * is matched against the map of call arg_call[a].
 *  - arg_kind[a] = 0, a ConstArg (checkConstArg, :105-112): one window, v =
 *    arg_val[a]; every replacer of shrinkExpand(v, map) (:164-218) is a mutant
 *    (at = 0, nb = 8, rep).  Its range in arg_off must be empty.
 *  - arg_kind[a] = 1, a DataArg (checkDataArg, :114-132) whose L bytes are
 *    d_data[arg_off[a] .. arg_off[a + 1]) (no alignment asked): windows i = 0 ..
 *    min(L, 100) - 1, v = the little-endian u64 of data[i : i + 8], zero-padded
 *    past L (:122-124); every replacer is a mutant (at = i, nb = min(8, L - i),
 *    rep): the mutated arg is the original with bytes at .. at + nb set to the
 *    low nb bytes of rep, little-endian (:126-127; copy() stops at the arg's
 *    end).  rep is reported in full.
 * Replacers are a set per window (uint64Set), a replacer equal to v included;
 * the order is args as given, windows ascending, replacers ascending as
 * unsigned (the fixed instance of Go's map order that shrink_expand uses).  Arg
 * a's mutants are entries mut_off[a] .. mut_off[a + 1] of d_mut_at, d_mut_nb
 * and d_mut_rep (cap entries each); mut_off has narg + 1 entries; *n_out = the
 * total.  If it exceeds cap nothing of the caller's is written: SYZSIG_ERANGE
 * with the needed total in *n_out.  special_ints as for
 * syzsig_shrink_expand_dev.  SYZSIG_EINVAL (nothing written): a NULL argument,
 * an arg_call outside the maps, a kind other than 0 / 1, an arg_off that
 * decreases or passes nbytes, a ConstArg with a non-empty range, more than
 * 2^25 args.  narg = 0 writes mut_off[0] = 0. */
int syzsig_hint_mutants_dev(syzsig_ctx* ctx, const uint64_t* d_map_off, const uint64_t* d_pairs, uint64_t ncalls,
                            uint64_t npairs, const uint32_t* d_arg_call, const uint8_t* d_arg_kind,
                            const uint64_t* d_arg_val, const uint64_t* d_arg_off, const uint8_t* d_data,
                            uint64_t narg, uint64_t nbytes, const uint64_t* special_ints, uint32_t nspecial,
                            uint64_t* d_mut_off, uint32_t* d_mut_at, uint8_t* d_mut_nb, uint64_t* d_mut_rep,
                            uint64_t cap, uint64_t* n_out);
/* The paths of the last syzsig_hint_mutants_dev call: out[0] = args resolved
 * in LDS, out[1] = args that took the fallback, out[2] = windows examined,
 * out[3] = accepted candidates before the per-window dedup. */
int syzsig_hint_mutants_stats(syzsig_ctx* ctx, uint64_t out[4]);

/* ---- pkg/hash/hash.go:14-26: type Sig [sha1.Size]byte, Hash, over a batch ----
 * Message i is d_data[off[i] .. off[i + 1]) (d_off has nmsg + 1 entries), at any
 * byte alignment; d_sig[20 i ..] receives its Sig: the SHA-1 digest bytes in
 * order (each state word big-endian), what hash.Hash returns and Sig.String
 * prints as hex.  Hash(pieces...) is the hash of the concatenation: the caller
 * concatenates.  nmsg = 0 is SYZSIG_OK and writes nothing.
 * SYZSIG_EINVAL, nothing written: a NULL d_off or d_sig with nmsg > 0, a NULL
 * d_data with nbytes > 0, offsets that decrease, off[nmsg] > nbytes.
 * SYZSIG_ERANGE, nothing written: a message longer than SYZSIG_HASH_MAX_MSG
 * (its bit length then fits the low length word; the executor's input region
 * is 2 MB), 2^32 or more messages.  The offsets are checked on device before
 * any byte of d_data is read.
 * Reads: no byte outside the messages' ranges is ever loaded, aligned or not.
 * The 16-byte and 4-byte loads are of aligned chunks that lie wholly inside the
 * span of one wave's messages (resp. inside one message); the bytes before the
 * first and after the last such chunk are loaded one by one.  Nothing is assumed
 * about the allocation's alignment or about room past d_data + nbytes.
 * SYZSIG_HASH_STAGE: 64 consecutive messages are one wave's; when their bytes
 * together are at most this many, the wave loads them coalesced into LDS and
 * hashes from there, else each lane reads its own message from global memory.
 * SYZSIG_HASH_LONG: a message longer than this is left to a second launch
 * that takes only such messages, one per lane, so that it does not hold up the
 * 63 others of its wave. */
#define SYZSIG_SIG_BYTES 20
#define SYZSIG_HASH_MAX_MSG (1ull << 28)
#define SYZSIG_HASH_STAGE 32768
#define SYZSIG_HASH_LONG 4096
int syzsig_hash_dev(syzsig_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off, uint64_t nmsg, uint64_t nbytes,
                    uint8_t* d_sig);
/* The paths of the last syzsig_hash_dev call: out[0] = messages hashed from LDS
 * staging, out[1] = messages of the first launch read directly from global
 * memory, out[2] = messages on the long list, out[3] = 64-byte blocks
 * compressed. */
int syzsig_hash_stats(syzsig_ctx* ctx, uint64_t out[4]);

/* ---- sets keyed by hash.Sig: fuzzer.corpusHashes (syz-fuzzer/fuzzer.go:
 * 447-452), mgr.hubCorpus (syz-manager/manager.go:1110-1113, :1142-1158), the
 * keys of mgr.corpus ----
 * A syzsig_sigset is a device-resident map[hash.Sig]struct{}: its Sigs sorted
 * ascending as memcmp orders them.  NULL is the nil map: Len 0, usable wherever
 * a set is read, and allocated by the entry points that write one.  Every d_sig
 * is n Sigs of SYZSIG_SIG_BYTES bytes back to back in device memory, at any
 * alignment.  One call takes at most 2^25 Sigs and a set holds at most 2^32 - 2
 * (SYZSIG_ERANGE).  SYZSIG_SIGSET_TILE: the keys of one sort tile in LDS; a
 * longer batch is tile-sorted and rank-merged through workspace buffers. */
#define SYZSIG_SIGSET_TILE 2048
typedef struct syzsig_sigset syzsig_sigset;
int syzsig_sigset_make(syzsig_ctx* ctx, syzsig_sigset** out);
void syzsig_sigset_free(syzsig_sigset* s);
uint64_t syzsig_sigset_len(const syzsig_sigset* s);
/* addInputToCorpus's `if _, ok := fuzzer.corpusHashes[sig]; !ok` (fuzzer.go:
 * 447-452) over a batch in arrival order: is_new[i] = 1 iff Sig i is neither
 * in the set nor at an earlier row of the batch -- the rows whose programs are
 * appended to fuzzer.corpus.  Afterwards the set holds the union.  A NULL *s is
 * allocated only if n > 0.  All or nothing: the new storage is allocated
 * before d_is_new is written, and the set takes it last. */
int syzsig_sigset_add_dev(syzsig_ctx* ctx, syzsig_sigset** s, const uint8_t* d_sig, uint64_t n, uint8_t* d_is_new);
/* in[i] = 1 iff Sig i is in s (NULL: the empty set). */
int syzsig_sigset_contains_dev(syzsig_ctx* ctx, const syzsig_sigset* s, const uint8_t* d_sig, uint64_t n,
                               uint8_t* d_in);
/* The set's Sigs ascending (one fixed instance of Go's map order, as
 * Serialize's elsewhere); *n_out = Len.  cap (in Sigs) below it: SYZSIG_ERANGE,
 * nothing written. */
int syzsig_sigset_export_dev(syzsig_ctx* ctx, const syzsig_sigset* s, uint8_t* d_sig, uint64_t cap, uint64_t* n_out);
/* The dense keys syzsig_manager_new_input_batch takes for hash.String(a.Prog):
 * key[i] = the number of distinct Sigs whose first row precedes Sig i's first
 * row (dense, in order of first appearance), first[k] = key k's first row,
 * known[k] = 1 iff key k's Sig is in `known` (the keys of mgr.corpus; NULL:
 * empty): the keys whose old entry goes in as a SYZSIG_INPUT_PRESENT row.
 * *nkeys = the distinct Sigs.  d_key has n entries, d_first and d_known n
 * entries of capacity. */
int syzsig_number_sigs_dev(syzsig_ctx* ctx, const syzsig_sigset* known, const uint8_t* d_sig, uint64_t n,
                           uint32_t* d_key, uint32_t* d_first, uint8_t* d_known, uint64_t* nkeys);
/* hubSync's diff (manager.go:1142-1158) with d_sig the Sigs of mgr.corpus:
 * add[i] = 1 iff Sig i is not in hubCorpus and at no earlier row (:1146-1150);
 * d_del_sig receives, ascending, the Sigs of hubCorpus absent from the batch
 * (:1152-1157), *ndel their number; afterwards hubCorpus is the set of the
 * batch.  del_cap (in Sigs) below *ndel: SYZSIG_ERANGE with *ndel set and
 * nothing else changed.  On a NULL *hub_corpus this is the Connect branch
 * (:1110-1113): every first row is added; it stays NULL when n == 0. */
int syzsig_hub_sync_dev(syzsig_ctx* ctx, syzsig_sigset** hub_corpus, const uint8_t* d_sig, uint64_t n,
                        uint8_t* d_add, uint8_t* d_del_sig, uint64_t del_cap, uint64_t* ndel);

/* ---- pkg/db/db.go:177-265: db.Open's read side -- deserializeDB over the
 * file's bytes: corpus.db of syz-manager (manager.go:185-243), the databases of
 * syz-hub (state.go:85-91), tools/syz-db.  The write side (serializeRecord with
 * its compressor, Save / Delete's no-op rules) follows below; files, Flush and
 * compact's decisions are the caller's (syzkaller_amd/db.py restates them). ----
 * Three steps: the frames on the host, the values on the device, the map's
 * last-write-wins on the device.  (d_out, d_out_off) of the second is what
 * syzsig_hash_dev takes. */
/* deserializeHeader and the frame of every deserializeRecord (db.go:203-257) of
 * the host buffer data[0 .. nbytes); no context and no device.  The chain of
 * lengths is walked, the compressed values are not read.  *version = the user
 * version (0 for a version-1 header, the empty file, a bad header); *n = the
 * records framed whole inside the file before the walk ended; *ended = how:
 *   SYZSIG_DB_END_EOF         the file ended at a record boundary (:187-189), or is empty (:206-208)
 *   SYZSIG_DB_END_BAD_HEADER  magic != 0xbaddb, version 0 or > 2, or the file ends inside the header:
 *                             no record (:179-183)
 *   SYZSIG_DB_END_BAD_MAGIC   a record that does not start with 0xfee1bad (:234-237)
 *   SYZSIG_DB_END_TRUNCATED   the file ends inside a record: a field, a key or a value runs past it
 * Record i: its key is data[key_off[i] .. + key_len[i]), seq[i]; its value's raw
 * DEFLATE stream data[val_off[i] .. + val_len[i]), both 0 for a delete (seq ==
 * ^0, :250-252) and for an empty value (valLen == 0, :257).  Every length is
 * checked against the bytes left before it is used: a key length of 0xffffffff
 * is a truncated record.  cap = the room of the five arrays in records; below
 * *n: SYZSIG_ERANGE with *n set and nothing else written (NULL arrays with
 * cap = 0: the sizing call).  SYZSIG_EINVAL: a NULL version, n or ended, a NULL
 * data with nbytes > 0, NULL arrays with records to write. */
#define SYZSIG_DB_END_EOF 0
#define SYZSIG_DB_END_BAD_HEADER 1
#define SYZSIG_DB_END_BAD_MAGIC 2
#define SYZSIG_DB_END_TRUNCATED 3
int syzsig_db_scan(const uint8_t* data, uint64_t nbytes, uint64_t cap, uint64_t* version, uint64_t* n,
                   uint32_t* ended, uint64_t* key_off, uint32_t* key_len, uint64_t* seq, uint64_t* val_off,
                   uint32_t* val_len);
/* flate.NewReader + ioutil.ReadAll (db.go:258-259) over a batch: stream i is the
 * raw DEFLATE (RFC 1951) bytes d_src[src_off[i] .. + src_len[i]), at any byte
 * alignment; an entry of length 0 is skipped (status OK, no output: the empty
 * value).  Stream i's output is d_out[out_off[i] .. out_off[i + 1]) (d_out_off
 * has n + 1 entries, out_off[0] = 0), *out_bytes = out_off[n]; d_status[i]:
 *   SYZSIG_INFLATE_OK
 *   SYZSIG_INFLATE_TRUNCATED  the input ended before the final block's end
 *   SYZSIG_INFLATE_INVALID    block type 3; a stored LEN != ~NLEN; HLIT > 286 or HDIST > 30; an
 *                             over-subscribed code; an incomplete one other than the single one-bit
 *                             code; a repeat with nothing to repeat or past HLIT + HDIST; no
 *                             end-of-block code; literal/length symbols 286, 287; distance symbols
 *                             30, 31; a distance that reaches before this stream's output
 *   SYZSIG_INFLATE_TRAILING   bytes left after the final block.  (The reference's answer here
 *                             depends on its bufio.Reader's fill; its writer never produces one.
 *                             This class is this library's decision: DESIGN.md.)
 *   SYZSIG_INFLATE_TOO_LONG   more than SYZSIG_INFLATE_MAX_OUT bytes of output
 * the first one met in stream order; the decoder is pinned to zlib 1.2.11's
 * inflate() wherever RFC 1951 leaves a choice (csrc/inflate_core.h).  A stream
 * that is not OK has length 0 in d_out_off and disturbs no other.
 * out_cap = the room of d_out.  Below *out_bytes: SYZSIG_ERANGE with *out_bytes
 * set and nothing else written.  A NULL d_out with out_cap = 0 is the sizing
 * call: SYZSIG_OK, d_out_off and d_status written as the full call writes them,
 * no output.  n = 0 writes out_off[0] = 0.
 * SYZSIG_EINVAL, nothing written: a NULL argument, a stream's range that passes
 * nbytes (checked on device, overflow-safe, before any byte of d_src is read).
 * SYZSIG_ERANGE, nothing written: more than 2^25 streams.
 * Reads: as syzsig_hash_dev, no byte outside a stream's range is ever loaded;
 * the decoder loads single bytes.  Every loop over input is bounded by the
 * stream's length and every write by the extent the counting pass computed.
 * One lane decodes one stream (counting pass, scan, writing pass);
 * SYZSIG_INFLATE_LONG: a stream of more compressed bytes than this is left to a
 * second launch that takes only such streams, as SYZSIG_HASH_LONG. */
#define SYZSIG_INFLATE_OK 0
#define SYZSIG_INFLATE_TRUNCATED 1
#define SYZSIG_INFLATE_INVALID 2
#define SYZSIG_INFLATE_TRAILING 3
#define SYZSIG_INFLATE_TOO_LONG 4
#define SYZSIG_INFLATE_MAX_OUT SYZSIG_HASH_MAX_MSG
#define SYZSIG_INFLATE_LONG 4096
int syzsig_inflate_dev(syzsig_ctx* ctx, const uint8_t* d_src, uint64_t nbytes, const uint64_t* d_src_off,
                       const uint32_t* d_src_len, uint64_t n, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                       uint8_t* d_status, uint64_t* out_bytes);
/* The paths of the last syzsig_inflate_dev call (its counting pass): out[0] =
 * streams decoded by the first launch, out[1] = streams on the long list,
 * out[2] = stored blocks, out[3] = fixed blocks in the low and dynamic blocks
 * in the high 32 bits. */
int syzsig_inflate_stats(syzsig_ctx* ctx, uint64_t out[4]);
/* deserializeDB's loop over the records (db.go:185-200) as a map from key to
 * the last write: d_sig = the n records' keys as 20-byte Sigs (the manager and
 * the hub only write hash.String keys, 40 hex characters: the caller parses
 * them; a database with any other key is replayed by the caller), d_seq their
 * seqs, nvalid <= n = the records before the first one that failed (its value's
 * status, or the scan's end).  live[i] = 1 iff i < nvalid, no record in
 * (i, nvalid) has record i's key, and seq[i] != ^0: the records of db.Records.
 * *nlive = their number = len(db.Records); *uncompacted = nvalid (:194).
 * One sort of (Sig, index), the Sig sets' (SYZSIG_SIGSET_TILE), and the last of
 * each run.  At most 2^25 records (SYZSIG_ERANGE).  All of d_live is written,
 * after everything that can fail. */
int syzsig_db_live_dev(syzsig_ctx* ctx, const uint8_t* d_sig, const uint64_t* d_seq, uint64_t n, uint64_t nvalid,
                       uint8_t* d_live, uint64_t* nlive, uint64_t* uncompacted);

/* ---- pkg/db/db.go:55-74, :147-175: the write side -- Save, Delete and
 * serializeRecord over a batch.  What is pinned is what a reader depends on:
 * the frame around a stream, which ops reach the log, and that zlib's inflate
 * and syzsig_inflate_dev read every stream back to its value.  The stream's own
 * bytes are this library's (compress/flate's differ between Go releases). ---- */
/* The compressor of serializeRecord over a batch, the mirror image of
 * syzsig_inflate_dev: value i is d_src[src_off[i] .. + src_len[i]), at any byte
 * alignment; its raw DEFLATE (RFC 1951) stream is d_out[out_off[i] ..
 * out_off[i + 1]) (n + 1 entries, out_off[0] = 0), *out_bytes = out_off[n].  A
 * value of length 0 gets a stream of length 0 (valLen = 0, db.go:158-159).
 * A stream is greedy LZ77 (matches of 3..258 bytes at distances <= 32768, found
 * through a hash table of recent positions, every candidate verified byte by
 * byte) in one final fixed-Huffman block, or, when that is not smaller, stored
 * blocks of at most 65535 bytes, the last one final: at most
 * len + 5 * ceil(len / 65535) bytes.  No sync-flush and no empty final block.
 * A stream's bytes depend on the value's bytes alone -- not on its lane, its
 * place or neighbours in the batch, its alignment or the launch that took it --
 * and equal syzsig_deflate_host's (one shared core, csrc/deflate_core.h).
 * out_cap = the room of d_out.  Below *out_bytes: SYZSIG_ERANGE with *out_bytes
 * set and nothing else written.  A NULL d_out with out_cap = 0 is the sizing
 * call: SYZSIG_OK, d_out_off written, no output.  n = 0 writes out_off[0] = 0.
 * SYZSIG_EINVAL, nothing written: a NULL argument, a value's range that passes
 * nbytes (checked on device, overflow-safe, before any byte of d_src is read).
 * SYZSIG_ERANGE, nothing written: more than 2^25 values, or a value of more than
 * SYZSIG_INFLATE_MAX_OUT bytes (it could never be read back).
 * Reads: no byte outside a value's range is ever loaded; single bytes.  Every
 * write is bounded by the extent the counting pass computed.  One lane
 * compresses one value (counting pass, scan, writing pass), its hash table in
 * LDS; SYZSIG_DEFLATE_LONG: a value of more bytes is left to a second launch
 * that takes only such values, as SYZSIG_INFLATE_LONG. */
#define SYZSIG_DEFLATE_LONG 4096
int syzsig_deflate_dev(syzsig_ctx* ctx, const uint8_t* d_src, uint64_t nbytes, const uint64_t* d_src_off,
                       const uint32_t* d_src_len, uint64_t n, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                       uint64_t* out_bytes);
/* The paths of the last syzsig_deflate_dev call (its counting pass): out[0] =
 * values compressed by the first launch, out[1] = values on the long list,
 * out[2] = streams written stored, out[3] = streams written fixed. */
int syzsig_deflate_stats(syzsig_ctx* ctx, uint64_t out[4]);
/* The same compressor for one value in host memory; no context and no device
 * (as syzsig_db_scan).  *out_len = the stream's size; cap below it:
 * SYZSIG_ERANGE with *out_len set and nothing written (a NULL out with cap = 0:
 * the sizing call).  SYZSIG_EINVAL: a NULL out_len, a NULL src with len > 0, a
 * NULL out with cap > 0; SYZSIG_ERANGE: len above SYZSIG_INFLATE_MAX_OUT. */
int syzsig_deflate_host(const uint8_t* src, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_len);
/* serializeRecord (db.go:147-175) over n records: d_sig their keys as 20-byte
 * Sigs, d_seq their seqs, stream i = d_stream[stream_off[i] .. stream_off[i + 1])
 * (syzsig_deflate_dev's outputs).  Record i is d_out[rec_off[i] .. rec_off[i + 1])
 * (n + 1 entries), *out_bytes = rec_off[n]: u32 0xfee1bad, u32 40, the Sig as 40
 * lower-case hex characters (hash.String), u64 seq, and unless seq == ^0 (a
 * delete: 56 bytes) u32 stream length and the stream (an empty one: 60 bytes);
 * little-endian.  The 16-byte file header is the caller's.  out_cap, the sizing
 * call and SYZSIG_ERANGE as syzsig_deflate_dev.  SYZSIG_EINVAL, nothing written:
 * a NULL argument, stream offsets that decrease or pass stream_bytes, a delete
 * with a stream of non-zero length (the reference's panic, :153-155);
 * SYZSIG_ERANGE: more than 2^25 records, a stream of 2^32 bytes or more. */
int syzsig_db_records_dev(syzsig_ctx* ctx, const uint8_t* d_sig, const uint64_t* d_seq, uint64_t n,
                          const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_stream_off, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_rec_off, uint64_t* out_bytes);
/* Save and Delete (db.go:55-74) over m ops in order, against the live set of nl
 * records (db.Records: distinct keys, no seq of ^0): Sigs, seqs and values
 * (data, off) each, value i = data[off[i] .. off[i + 1]); an op with seq == ^0 is
 * a Delete.  written[j] = 1 iff op j reaches the log: a Save unless its key is
 * present with the same seq and equal bytes (:59-61), a Delete unless its key is
 * absent (:68-70), where the state an op sees is what the last earlier row of
 * its key -- op or live record -- left.  keep_live[i] / keep_op[j] = 1 for the
 * rows of the new db.Records: per key its last written row (a live record
 * counts as written), unless that is a Delete; the new Records in file order of
 * the last write are the kept live records in their order, then the kept ops in
 * theirs.  *nwritten, *nkeep_live, *nkeep_op their counts.  One sort of (Sig,
 * row) over nl + m rows, the Sig sets' (SYZSIG_SIGSET_TILE), a look at each
 * run's neighbours, and a byte compare where seq and length agree.
 * SYZSIG_EINVAL, nothing written: a NULL argument, offsets that decrease or pass
 * their nbytes, a Delete with a non-empty value, a live seq of ^0;
 * SYZSIG_ERANGE: nl + m above 2^25.  Everything is written after everything
 * that can fail. */
int syzsig_db_apply_dev(syzsig_ctx* ctx, const uint8_t* d_live_sig, const uint64_t* d_live_seq, uint64_t nl,
                        const uint8_t* d_live_data, uint64_t live_bytes, const uint64_t* d_live_off,
                        const uint8_t* d_op_sig, const uint64_t* d_op_seq, uint64_t m, const uint8_t* d_op_data,
                        uint64_t op_bytes, const uint64_t* d_op_off, uint8_t* d_written, uint8_t* d_keep_live,
                        uint8_t* d_keep_op, uint64_t* nwritten, uint64_t* nkeep_live, uint64_t* nkeep_op);

/* ---- prog/prio.go:133-245: call-to-call priorities over the whole corpus and
 * the ChoiceTable (the numeric part; the program model stays with the caller) ----
 * N = len(target.Syscalls); a matrix is N * N row-major.  Every result is what
 * the reference computes on amd64, bit for bit: float32, each operation rounded
 * on its own (no fused multiply-add), IEEE division.
 * SYZSIG_PRIO_MAX_CALLS: one row of u32 counters is static LDS.
 * SYZSIG_PRIO_SPLIT: the default of `split` below. */
#define SYZSIG_PRIO_MAX_CALLS 16384
#define SYZSIG_PRIO_SPLIT 4096
/* calcDynamicPrio and CalculatePriorities' product (prio.go:133-149, :27-36;
 * manager.go:896 on Connect).  The corpus is CSR: program p's calls are
 * d_call_id[off[p] .. off[p + 1]) (d_prog_off has nprog + 1 entries, off[0] = 0,
 * off[nprog] = total), each the call's Meta.ID.  d_prios[a * N + b] = the
 * normalised count of ordered pairs of positions (a at one, b at the other) over
 * all programs -- a cell is min(count, 2^24) as a float32 `+= 1.0` leaves it --
 * times d_static[a * N + b] when d_static is given (NULL: the dynamic matrix
 * alone).  A row whose cells are all equal and non-zero is NaN throughout, as in
 * Go.  split: a call that occurs more than `split` times has its row counted in
 * slices of `split` occurrences by workgroups of their own (0 = the default; it
 * is raised when the slices' partial rows would pass 1 GB); no result depends
 * on it.
 * SYZSIG_EINVAL: a NULL argument, N = 0, offsets that decrease or do not run
 * from 0 to total, a call id >= N (Go panics on the index).  SYZSIG_ERANGE:
 * N > SYZSIG_PRIO_MAX_CALLS; the sum of len_p^2 over the programs is 2^32 or
 * more (u32 counters are exact below it).  Both are found before any counting
 * and before d_prios is written. */
int syzsig_calc_prios_dev(syzsig_ctx* ctx, const uint64_t* d_prog_off, const uint32_t* d_call_id, uint64_t nprog,
                          uint64_t total, uint64_t N, uint64_t split, const float* d_static, float* d_prios);
/* The tail of calcStaticPriorities (prio.go:118-129) in place on the summed
 * matrix: pp[c0] = the row's max (over the row as given: the reference leaves
 * the diagonal 0 until here), then normalizePrio. */
int syzsig_static_prio_finish_dev(syzsig_ctx* ctx, float* d_prios, uint64_t N);
/* BuildChoiceTable (prio.go:198-228; syz-fuzzer/fuzzer.go:173).  d_enabled:
 * u8[N], non-zero = enabled (NULL: every call).  For an enabled row i,
 * d_run[i * N + j] = the sum over enabled j' <= j of int(prios[i][j'] * 1000)
 * (1 when d_prios is NULL, Go's nil prios); a disabled row, nil in Go, is zeros.
 * int() of a NaN, of a negative value or of one that is 2^31 / N or more is not
 * defined by Go: such a weight at an enabled row and column is SYZSIG_EINVAL,
 * syzsig_last_error names the first such row, and d_run is not written. */
int syzsig_choice_table_dev(syzsig_ctx* ctx, const float* d_prios, const uint8_t* d_enabled, uint64_t N,
                            int32_t* d_run);
/* Choose's lookup (prio.go:230-245; prog/rand.go:398) for n queries:
 * out[q] = sort.SearchInts(run[call[q]], x[q]), the smallest i with
 * run[call][i] >= x.  With x in [1, run[call][N - 1]], what r.Intn(total) + 1
 * draws, that is an enabled call of non-zero weight, so the reference's loop
 * never retries.  call < 0 or a row whose total is 0 (disabled): out[q] = N,
 * "uniform over enabledCalls", which is the caller's draw.  SYZSIG_EINVAL,
 * nothing written: a call >= N, an x outside [1, total] of an enabled row. */
int syzsig_choice_lookup_dev(syzsig_ctx* ctx, const int32_t* d_run, uint64_t N, const int32_t* d_call,
                             const int32_t* d_x, uint64_t n, int32_t* d_out);
/* The paths of the last syzsig_calc_prios_dev call: out[0] = rows counted whole,
 * out[1] = rows split, out[2] = slices, out[3] = pair increments (the sum of
 * len_p^2). */
int syzsig_prio_stats(syzsig_ctx* ctx, uint64_t out[4]);

/* ---- syz-manager/html.go, syz-manager/cover.go: the corpus-wide loops behind
 * the manager's coverage pages, their numeric part.  The text tools (objdump,
 * nm, readelf, addr2line, the source files, the HTML template) stay with the
 * caller, who interns call names to dense ids.  Every array is device memory;
 * each call is all-or-nothing on an argument error, with outputs untouched.
 *
 * collectSyscallInfo (html.go:135-149) and httpCover's selection
 * (html.go:202-212).  The corpus as CSR: input i's Cover is d_cov[d_cov_off[i]
 * .. d_cov_off[i + 1]) (offsets from 0 to total; repeats allowed within and
 * across inputs), its call d_call[i] < ncalls.  d_select: NULL = every input,
 * else input i takes part iff d_select[i] != 0.  Outputs: d_count[c] = the
 * selected inputs of call c (an input with an empty cover counts);
 * d_cover_len[c] = len(cc.cov); the unions as CSR, call c's PCs ascending and
 * distinct at d_call_cov[d_call_cov_off[c] .. d_call_cov_off[c + 1]) (ncalls +
 * 1 offsets).  d_all_cov / n_all (both or neither): the union over all
 * selected inputs, ascending, and its size -- httpCover with call == "",
 * httpRawCover; room for cover_cap PCs as well.  cover_cap below the selected
 * inputs' total PCs is SYZSIG_ERANGE (that total always suffices), a call id
 * >= ncalls or offsets that decrease or do not run from 0 to total
 * SYZSIG_EINVAL, both checked before anything is written.  total < 2^31. */
int syzsig_call_cover_dev(syzsig_ctx* ctx, const uint64_t* d_cov_off, const uint32_t* d_cov, uint64_t ninputs,
                          uint64_t total, const uint32_t* d_call, const uint8_t* d_select, uint64_t ncalls,
                          uint32_t* d_count, uint32_t* d_cover_len, uint64_t* d_call_cov_off, uint32_t* d_call_cov,
                          uint64_t cover_cap, uint32_t* d_all_cov, uint64_t* n_all);
/* cover.RestorePC (pkg/cover/cover.go:28-30), previousInstructionPC
 * (cover.go:394-411) and httpRawCover's sort (html.go:323-331) over n PCs:
 * d_out_order[i] = prev(base << 32 + d_pcs[i]) (generateCoverHTML's pcs,
 * cover.go:99-104), d_out_sorted = the same values ascending.  Repeats stay
 * (on arm two PCs can share a previous PC); with base == 0 a PC below the
 * subtrahend wraps as Go's u64 does and sorts last.  An arch other than the
 * five below is SYZSIG_EINVAL (Go panics).  n < 2^31. */
#define SYZSIG_ARCH_AMD64 0u   /* pc - 5 */
#define SYZSIG_ARCH_386 1u     /* pc - 1 */
#define SYZSIG_ARCH_ARM64 2u   /* pc - 4 */
#define SYZSIG_ARCH_ARM 3u     /* (pc - 3) & ~1 */
#define SYZSIG_ARCH_PPC64LE 4u /* pc - 4 */
int syzsig_report_pcs_dev(syzsig_ctx* ctx, const uint32_t* d_pcs, uint64_t n, uint32_t base, uint32_t arch,
                          uint64_t* d_out_order, uint64_t* d_out_sorted);
/* uncoveredPcsInFuncs (cover.go:254-304) for d_pcs in the order the loop sees
 * them.  Symbols as d_sym_start / d_sym_end (end = Addr + Size), sorted by
 * start as sort.Sort(symbols) leaves them (equal starts in the caller's
 * order); d_all_cover = allCoverPCs strictly ascending (a repeat is
 * SYZSIG_EINVAL: drop them first, the result is a map's keys).  d_out (room for
 * nall PCs) = the keys of `uncovered` ascending, *n_out their count.  nall == 0
 * gives an empty result (cover.go:268).  The device runs sort.Search's probe
 * sequence over `pc < end` (ends need not be monotone), keys handledFuncs by
 * start with the end of the alias that the first PC found, and adds a
 * function's sites at the position of its first PC, before that position's
 * delete.  npc, nsym, nall < 2^32. */
int syzsig_uncovered_pcs_dev(syzsig_ctx* ctx, const uint64_t* d_sym_start, const uint64_t* d_sym_end, uint64_t nsym,
                             const uint64_t* d_all_cover, uint64_t nall, const uint64_t* d_pcs, uint64_t npc,
                             uint64_t* d_out, uint64_t* n_out);
/* The paths of the context's last call of the three above (tests, tuning):
 * out[0] = call segments of more than SYZSIG_COVER_TILE PCs (repeats
 * included), out[1] = the rank-merge passes over them, out[2] = functions
 * handled, out[3] = those whose site range was walked by a workgroup. */
int syzsig_report_stats(syzsig_ctx* ctx, uint64_t out[4]);
/* fileSet (cover.go:162-193) and the per-file Coverage count of
 * generateCoverHTML's line walk (cover.go:129-148) over symbolized frames.  The
 * caller interns Frame.File and Frame.Func to dense ids (file < nfiles, func <
 * nfuncs; funcs is keyed by the function's name alone, so one name is one id
 * whatever its file) and passes each list as three parallel arrays; lines are
 * Frame.Line as int32, the whole range, ordered as signed.  The order of frames
 * within a list does not matter; the covered list is applied first, as in Go:
 * an uncovered frame counts only if its function has a covered frame, and a
 * line that is covered stays covered.
 * Outputs, as CSR over the files: file f's sorted list is d_line / d_covered
 * [d_off[f] .. d_off[f + 1]) (nfiles + 1 offsets from 0), lines strictly
 * ascending, covered 0 or 1.  A file without entries has an empty range (the
 * Go map has no such key).  cap = room in d_line and d_covered; a cap below the
 * entries of all lists is SYZSIG_ERANGE (ncov + nunc always suffices), a file
 * or function id out of range SYZSIG_EINVAL, both checked before anything is
 * written.
 * d_nlines (nfiles; NULL: the lists only, and then d_shown and d_coverage are
 * NULL too, else neither is): len(parseFile(f)) per file.  d_shown[f] = the
 * entries the walk consumes: 0 when the list is empty or its first line is
 * below 1 (an entry that is never consumed blocks all behind it: `?:0` of
 * addr2line), else the entries with line <= nlines; d_coverage[f] = the
 * covered ones among the first d_shown[f] = templateFile.Coverage.
 * SYZSIG_FILESET_TILE: a file with at most this many frames (covered plus
 * kept uncovered, repeats included) is sorted in LDS by one workgroup.
 * ncov + nunc < 2^31; nfiles, nfuncs < 2^32. */
#define SYZSIG_FILESET_TILE 2048
int syzsig_file_set_dev(syzsig_ctx* ctx, const uint32_t* d_cov_file, const int32_t* d_cov_line,
                        const uint32_t* d_cov_func, uint64_t ncov, const uint32_t* d_unc_file,
                        const int32_t* d_unc_line, const uint32_t* d_unc_func, uint64_t nunc, uint64_t nfiles,
                        uint64_t nfuncs, const uint32_t* d_nlines, uint64_t* d_off, int32_t* d_line,
                        uint8_t* d_covered, uint64_t cap, uint32_t* d_shown, uint32_t* d_coverage);
/* The paths of the context's last syzsig_file_set_dev call: out[0] = uncovered
 * frames kept (their function has a covered frame), out[1] = files of more
 * than SYZSIG_FILESET_TILE frames, out[2] = the rank-merge passes over them,
 * out[3] = entries written. */
int syzsig_file_set_stats(syzsig_ctx* ctx, uint64_t out[4]);

/* ---- hash-sharded maxSignal across GPUs (one process per GPU) ----
 * The batch is split by program range over G GPUs (serial order = GPU-major);
 * each element is owned by the GPU owner = syz::owner_of(elem, G).  Records
 * travel packed as
 *   elem << 32 | level << 24 | serial      (serial < 2^24, level < 4)
 * where serial is its call's position in the batch's global serial order and
 * level the rank of its call's prio in `levels` (ascending int8, <= 4 entries,
 * the union of the prios of all GPUs' calls).  A source sends only each
 * element's staircase -- for every level, the element's first local record at
 * that level if no earlier local record has a higher level, <= 4 records per
 * distinct element: records off the staircase can never be new nor raise
 * maxSignal, so the owner's triage of the staircases is checkNewSignal's exact
 * result.  The exchange is the stream-ordered step below; the owner side is
 * records mode:
 *
 * syzsig_triage_records_dev: triage records against the local shard of
 * maxSignal; d_new_flags[i] = 1 iff record i is new (checkNewSignal's DiffRaw
 * result for its call).  Serial order comes from the records' serial fields;
 * records with one serial are one call's, so they carry one level. */
int syzsig_triage_records_dev(syzsig_ctx* ctx, syzsig_set* shard, syzsig_set** new_signal,
                              const uint64_t* d_recs, uint64_t nrec, const int8_t* levels,
                              uint32_t nlevels, uint8_t* d_new_flags, syzsig_batch_stats* stats);

/* ---- the stream-ordered sharded step (one process per GPU) ----
 * The three calls below only enqueue work on the context's stream and return;
 * syzsig_step_finish is the step's one host synchronisation.  The exchange
 * uses fixed-size buckets, so no split sizes have to reach the host first:
 * each source writes, for every owner g, a bucket of cap + 1 words at
 * d_send[g * (cap + 1)]:
 *   word 0      header: records for g (the true count, even past cap)
 *               | SYZSIG_STEP_HDR_VOID (the source's run is void)
 *               | SYZSIG_STEP_HDR_OVF  (more than cap records for g)
 *   words 1..   the staircase records (elem << 32 | level << 24 | serial).
 * An equal-split all-to-all of the buckets gives each owner every source's
 * bucket for it (d_recv, same layout, bucket s from source s); the owner's
 * flags go back the same way, one byte per word (d_flags / d_back, nshards *
 * (cap + 1) bytes; byte 0 of a bucket is the owner's status).  Every owner sees
 * every header, so all ranks agree without another collective that a step is
 * void (nothing committed anywhere; redo it, with exact = 1 on a void source
 * and a larger cap after an overflow) or which owners skipped their records
 * (their records redone with syzsig_step_own_dev(exact = 1) and one more flags
 * exchange, which syzsig_step_back_dev adds to the first).
 * Reference semantics: syz-fuzzer/fuzzer.go:494-511 over the batch in global
 * serial order; the result is the unsharded checkNewSignal's. */
#define SYZSIG_STEP_HDR_VOID (1ull << 63)
#define SYZSIG_STEP_HDR_OVF (1ull << 62)
#define SYZSIG_STEP_HDR_COUNT ((1ull << 40) - 1)
typedef struct {
	uint64_t src_void;     /* this source's run was void: 1 = a cell spilled, a partition overflowed the LDS
	                          table, a call range is bad or the records exceed b->nrec (redo with exact = 1,
	                          which validates), 2 = a call's prio is not among `levels` */
	uint64_t global_void;  /* some bucket was void or over cap: nothing was committed on any rank */
	uint64_t owners_void;  /* bit g: owner g skipped its records (redo them exactly); 0 when global_void */
	uint64_t records;      /* this source's records */
	uint64_t distinct;     /* this source's distinct elements */
	uint64_t sent;         /* this source's staircase records (all owners) */
	uint64_t max_out;      /* the most records this source had for one owner (the cap it needs) */
	uint64_t received;     /* records this owner received */
	uint64_t max_in;       /* the most records one source had for this owner */
	uint64_t own_distinct; /* distinct elements among them */
	uint64_t inserted;     /* elements new to this owner's shard */
	uint64_t changed;      /* elements whose prio rose in this owner's shard */
	uint64_t new_pairs;    /* this source's DiffRaw entries (call << 32 | elem), see syzsig_batch */
	uint64_t own_parts;    /* LDS partitions of the owner's records (0 = exact path) */
	double src_ms, own_ms, back_ms; /* device time of each side (0 unless timing is on) */
} syzsig_step_status;
/* Source side: aggregate b (zeroing call_new) and write its staircase buckets.
 * cap >= 1; d_send has nshards * (cap + 1) words.  exact = 0: one run on
 * capped cells that voids itself on a spill, an LDS partition overflow or a prio
 * outside `levels` (no host round trip); exact = 1: the counted path with its
 * HBM fallback (host round trips; a prio outside `levels` is SYZSIG_EINVAL). */
int syzsig_step_send_dev(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t serial_base, const int8_t* levels,
                         uint32_t nlevels, uint32_t nshards, uint64_t cap, uint64_t* d_send, int exact);
/* Owner side: the buckets every source sent this owner (d_recv, nshards *
 * (cap + 1) words) triaged against its shard and newSignal shard (both
 * non-NULL); d_flags gets one byte per word.  exact = 0: records partitioned by
 * element hash through LDS (per partition its elements' level firsts, per
 * element one shard probe, per record checkNewSignal's verdict in closed form;
 * no sort); a partition over the LDS capacity makes this owner skip its
 * records (owners_void).
 * exact = 1: the per-record path (host round trips), for that redo.  Until
 * syzsig_step_finish, `shard` and `new_signal` take no other call. */
int syzsig_step_own_dev(syzsig_ctx* ctx, syzsig_set* shard, syzsig_set* new_signal, const uint64_t* d_recv,
                        uint32_t nshards, uint64_t cap, const int8_t* levels, uint32_t nlevels, uint8_t* d_flags,
                        int exact);
/* Source side again: the owners' flags (d_back, from the flags exchange) for
 * this source's buckets -> b->call_new, b->new_pairs (new_pairs_cap entries at
 * most; the total in the status); b->new_bits (if set; costs one host
 * synchronisation).  Adds to what an earlier call of the step set. */
int syzsig_step_back_dev(syzsig_ctx* ctx, const syzsig_batch* b, uint64_t serial_base, const uint64_t* d_send,
                         uint32_t nshards, uint64_t cap, const uint8_t* d_back);
/* The step's one host synchronisation: waits for the context's stream (which
 * the collectives' streams joined), commits the owner's table lengths and
 * returns the status of the calls since the last finish. */
int syzsig_step_finish(syzsig_ctx* ctx, syzsig_step_status* status);

/* ---- synthetic workload (deterministic; host and device give identical data) ---- */
typedef struct {
	uint64_t seed;
	uint32_t nblocks_log2, region_log2, nsys, skew, restart_log2;
	uint32_t errno_permille, any_permille, bad_pc_ppm;
	/* 1: SURVEY 8(d)'s global walk -- each call starts at a uniform block and
	 * walks b <- (4b + 1 + r%4) mod 2^nblocks_log2 with no restarts (region_log2,
	 * nsys, skew and restart_log2 then only pick the call's prio draw); M0's
	 * known elements are that walk's whole edge universe. */
	uint32_t global_walk;
} syzsig_synth_cfg;

void syzsig_synth_default(syzsig_synth_cfg* cfg);
/* Per call c of a batch (prog_base + p for program p): call_prio and the raw trace
 * of call_len[c] PCs at pcs[call_start[c]..]. */
int syzsig_synth_traces_host(const syzsig_synth_cfg* cfg, uint64_t prog_base, uint64_t nprog,
                             uint32_t calls_per_prog, const uint64_t* call_start, const uint32_t* call_len,
                             uint64_t* pcs, uint8_t* call_prio);
int syzsig_synth_traces_dev(syzsig_ctx* ctx, const syzsig_synth_cfg* cfg, uint64_t prog_base,
                            uint64_t nprog, uint32_t calls_per_prog, const uint64_t* d_call_start,
                            const uint32_t* d_call_len, uint64_t* d_pcs, uint8_t* d_call_prio);
int syzsig_synth_m0_host(const syzsig_synth_cfg* cfg, uint64_t known_sys, uint64_t n, uint32_t* elems,
                         int8_t* prios);
int syzsig_synth_m0_dev(syzsig_ctx* ctx, const syzsig_synth_cfg* cfg, uint64_t known_sys, uint64_t n,
                        uint32_t* d_elems, int8_t* d_prios);
/* The elements i < n of that M0 which shard `shard` of `nshards` owns
 * (owner_of), in index order, packed into d_elems/d_prios (capacity `cap`);
 * *n_out = how many.  A rank builds its shard of a 1B-element M0 without
 * materialising the whole. */
int syzsig_synth_m0_shard_dev(syzsig_ctx* ctx, const syzsig_synth_cfg* cfg, uint64_t known_sys, uint64_t n,
                              uint32_t nshards, uint32_t shard, uint32_t* d_elems, int8_t* d_prios, uint64_t cap,
                              uint64_t* n_out);

/* ---- program text: the calls of a batch of programs (csrc/calls.hip) ----
 *
 * The heads of the lines of program text, and nothing else of it: the ordered
 * call ids that target.Deserialize would give p.Calls[*].Meta.ID
 * (prog/encoding.go:159-180, the parser of :740-828), or prog.CallSet's set
 * (:836-869).  This does not parse arguments, it does not run validate(), and it
 * does not run SanitizeCall: a program whose heads are well-formed but whose
 * arguments are broken is reported OK here.  Deserialize stays with the caller
 * for programs that arrive from outside.
 *
 * The name table of one target: names[name_off[i] .. name_off[i + 1]) is the name
 * of call id i (host arrays, name_off[0] = 0, n + 1 offsets).  Open-addressed on
 * a 64-bit hash of the bytes; a hit is the hash, the length and then the bytes.
 * SYZSIG_EINVAL: a NULL argument, n = 0, an empty name, a duplicate name, offsets
 * that decrease.  SYZSIG_ERANGE: more than 2^24 names. */
typedef struct syzsig_calltab syzsig_calltab;
int syzsig_calltab_make(syzsig_ctx* ctx, const uint8_t* names, const uint64_t* name_off, uint64_t n,
                        syzsig_calltab** out);
void syzsig_calltab_free(syzsig_calltab* tab);
uint64_t syzsig_calltab_len(const syzsig_calltab* tab);
/* Program i is d_data[off[i] .. off[i + 1]) (d_off has nprog + 1 entries; d_data
 * is 16-byte aligned).  Lines are bufio.ScanLines': the runs between '\n' inside
 * the program, a last run without '\n' if it is not empty, one trailing '\r'
 * dropped; a line never passes off[i + 1].  A line of SYZSIG_PROGTEXT_MAX_LINE
 * bytes or more before its '\n' ('\r' counted) fails its program with
 * SYZSIG_PT_LINE_TOO_LONG.  Empty lines and lines that start with '#' are skipped.
 * d_status[i] is the status of the program's first failing line and d_err_line[i]
 * that line's 1-based number, skipped lines counted (0: no line to blame); a
 * program that is not OK has an empty range in d_call_off and flag 0.
 *   SYZSIG_PROGTEXT_DESERIALIZE  a line is I W* ( '=' W* I W* )? '(' from its first
 *     byte (W: space or tab, I: one or more of [a-zA-Z0-9_$]), the name its last I.
 *     SYZSIG_PT_BAD_IDENT: no identifier at the line's start or after the '=';
 *     SYZSIG_PT_BAD_HEAD: the line ends where '=' or '(' is expected;
 *     SYZSIG_PT_UNKNOWN_CALL: the name is not in the table (looked up before the
 *     '('); SYZSIG_PT_BAD_HEAD: the next byte is not '('.  A program without call
 *     lines is OK with no calls.  The ids are in line order; d_flag[i] = 1 when a
 *     call of the program has d_enabled[id] == 0 ("contains a disabled syscall").
 *   SYZSIG_PROGTEXT_CALLSET  the name is the line up to its first '(' -- none:
 *     SYZSIG_PT_NO_BRACKET -- restarted behind its first '=' and the spaces (not
 *     tabs) after it; empty: SYZSIG_PT_EMPTY_NAME; a program without calls:
 *     SYZSIG_PT_NO_CALLS.  The ids are the distinct names found in the table,
 *     ascending; d_flag[i] = supported | has_unknown << 1: has_unknown = some name
 *     is not in the table, supported = !has_unknown and every id enabled.
 * d_enabled: one byte per table entry, NULL = every call enabled.
 * Count-then-write: *total = d_call_off[nprog].  cap = the room of d_call_id;
 * below *total: SYZSIG_ERANGE with *total set and nothing else written.  A NULL
 * d_call_id with cap = 0 is the sizing call: SYZSIG_OK, everything but the ids
 * written.  nprog = 0 writes call_off[0] = 0.
 * SYZSIG_EINVAL, nothing written: a NULL argument or table, a mode that is neither,
 * offsets that decrease or pass nbytes.  SYZSIG_ERANGE, nothing written: more
 * than 2^25 programs, 2^32 calls or more.
 * The text is read twice (line starts counted, then parsed), 16 bytes per lane,
 * SYZSIG_PROGTEXT_TILE bytes per workgroup staged in LDS with
 * SYZSIG_PROGTEXT_WINDOW bytes behind them; a head that does not end inside the
 * window after its line's start is left to a second launch.  CallSet's dedup is
 * the shared segmented sort-unique, SYZSIG_PROGTEXT_SORT_TILE ids per tile. */
#define SYZSIG_PROGTEXT_DESERIALIZE 0
#define SYZSIG_PROGTEXT_CALLSET 1
#define SYZSIG_PROGTEXT_MAX_LINE (1u << 20)
#define SYZSIG_PROGTEXT_TILE 4096
#define SYZSIG_PROGTEXT_WINDOW 256
#define SYZSIG_PROGTEXT_SORT_TILE 2048
#define SYZSIG_PT_OK 0
#define SYZSIG_PT_LINE_TOO_LONG 1
#define SYZSIG_PT_BAD_IDENT 2
#define SYZSIG_PT_BAD_HEAD 3
#define SYZSIG_PT_UNKNOWN_CALL 4
#define SYZSIG_PT_NO_BRACKET 5
#define SYZSIG_PT_EMPTY_NAME 6
#define SYZSIG_PT_NO_CALLS 7
int syzsig_prog_calls_dev(syzsig_ctx* ctx, const syzsig_calltab* tab, const uint8_t* d_data, uint64_t nbytes,
                          const uint64_t* d_off, uint64_t nprog, uint32_t mode, const uint8_t* d_enabled,
                          uint64_t* d_call_off, uint32_t* d_call_id, uint64_t cap, uint8_t* d_status,
                          uint32_t* d_err_line, uint8_t* d_flag, uint64_t* total);
/* The paths of the last syzsig_prog_calls_dev call: out[0] = lines seen, out[1] =
 * lines skipped, out[2] = heads parsed in the window, out[3] = heads on the long
 * list. */
int syzsig_prog_calls_stats(syzsig_ctx* ctx, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SYZSIG_H */
