/*
 * sst.h -- C ABI of the MI355X mass-explanation engine (libsstgpu.so).
 *
 * Drop-in boundary for spectrseq/spectrseqtools' per-peak combinatorial
 * search.  The reference has no FFI (it is pure Python); these entry points
 * are what its hot-path functions call through ctypes in
 * spectrseqtools_amd/_native.py.  Each declaration cites the reference
 * interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain C types only; host pointers unless the name ends in _device;
 *   - every function returns 0 on success or a negative SST_E* code; the
 *     message is available from sst_last_error(ctx);
 *   - one sst_ctx per HIP device; calls on one ctx are serialised; a table
 *     belongs to the ctx that made it;
 *   - masses are f64 Da; windows are quantised exactly as the reference does
 *     (mass_explanation.py:107,110-114): target = round(mass/precision) with
 *     ties-to-even, thr = ceil((thr_abs or tolerance*mass)/precision).
 */
#ifndef SST_H
#define SST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ---------------------------------------------------- */
#define SST_OK 0
#define SST_E_ARG (-1)      /* bad argument / shape                         */
#define SST_E_HIP (-2)      /* HIP runtime error                            */
#define SST_E_NOMEM (-3)    /* device allocation failed                     */
#define SST_E_TABLE (-4)    /* packed table violates the DP recurrence      */
#define SST_E_INTERNAL (-5) /* depth/budget guard tripped                   */

/* ---- per-query status of sst_explain_batch -------------------------- */
#define SST_NONE 0          /* reference returns MassExplanations(None)      */
#define SST_EMPTY 1         /* reference returns MassExplanations(set())     */
#define SST_SOME 2          /* >= 1 candidate composition                    */
#define SST_OUT_OF_TABLE (-1) /* reference raises NotImplementedError naming */
                              /* its window value (mass_explanation.py:68-72, */
                              /* :134-138 with `value` bound at :192)        */
#define SST_OVERFLOW (-2)   /* count > cap_per_query: exact count, no payload */
#define SST_ABORTED (-4)    /* DFS node guard (2^34 nodes) exhausted: count is a lower bound */

/* ---- per-query result of sst_is_valid_batch ------------------------- */
/*  1 = True, 0 = False, -1 = reference raises NotImplementedError          */

typedef struct sst_ctx sst_ctx;
typedef struct sst_table sst_table;
typedef struct sst_result sst_result;

/* Number of visible HIP devices (0 when none). */
int sst_device_count(void);

/* One context per GPU (one process per GPU in multi-GPU runs). */
int sst_ctx_create(int device, sst_ctx** out);
void sst_ctx_destroy(sst_ctx* ctx);
const char* sst_last_error(const sst_ctx* ctx);
/* The HIP stream all work of this ctx is queued on (hipStream_t). */
void* sst_ctx_stream(sst_ctx* ctx);
/* Queue this ctx's subsequent work on `stream` (a hipStream_t of the ctx's
 * device, owned by the caller), or on the ctx's own stream again when NULL.
 * Set-stream semantics as in rocBLAS: nothing is ordered across the switch,
 * the caller orders work on different streams (events).  A result's later
 * operations (compaction, fetch, free) go to the ctx's stream at that time.  Used to overlap the A7
 * batch with the A8 chain (bench.py).  No reference equivalent (the
 * reference is single-threaded Python). */
int sst_ctx_set_stream(sst_ctx* ctx, void* stream);
/* Wait for all queued work of this ctx. */
int sst_ctx_synchronize(sst_ctx* ctx);
/* Release the ctx's cached work buffers: the first-visit frontier's
 * workspaces that sst_length_bounds_frontier_device and
 * sst_length_bound_batch keep across calls (up to min(96 GB, free / 2) and
 * 4 GB), so that later stages, other allocators or another process on the
 * same GPU get that HBM back.  Waits for the ctx's queued work first; the
 * next frontier call allocates again.  No reference equivalent (the
 * reference's memo dict is freed when compute_sequence_length_bound returns,
 * mass_table.py:361). */
int sst_ctx_trim(sst_ctx* ctx);

/* Build the packed 2-bit DP reachability table on the GPU.
 * Replaces set_up_bit_table(integer_masses, max_mass, compression_rate)
 * (spectrseqtools/mass_table.py:207-248; settings :251-289) and therefore
 * load_dp_table / _reduce_nucleotide_list (:319-340, :102-121).
 * masses: sorted unique integer masses incl. the 0 sentinel (row 0),
 * n_rows <= 120; compression in {4, 8, 16, 32}. */
int sst_table_build(sst_ctx* ctx, const int64_t* masses, int n_rows, int64_t max_mass, int compression,
                    sst_table** out);

/* Adopt an existing packed table (e.g. the reference's .npy cache,
 * load_dp_table mass_table.py:319-340): words are n_rows x n_cols elements
 * of compression/4 bytes, C order.  Fails with SST_E_TABLE if the table
 * does not satisfy the row recurrence the engine's index relies on. */
int sst_table_upload(sst_ctx* ctx, const int64_t* masses, int n_rows, const void* words, int64_t n_cols,
                     int compression, sst_table** out);

/* Prove on the device that an uploaded table is the table set_up_bit_table
 * (mass_table.py:207-248) produces for its masses, and give it the state of a
 * table built here.  An uploaded table is otherwise only known to satisfy
 * bit0(r, m) == any(r - 1, m), which involves neither the masses nor bit1
 * (the reference's cache key ignores the alphabet: a .npy written for other
 * masses with the same row count loads silently, load_dp_table :319-340), so
 * it has no pair list: its explain passes run the bitset scan, the length
 * bound has neither fast path nor frontier, and sst_step_rows_device,
 * sst_explain_pairs_alpha* and the sst_pipe_* / bins / dict / walk stages
 * refuse it.
 * Criterion, every word against words of the same table, with pair(r, m) the
 * 2-bit cell of mass m (bit0 low, bit1 the "left" bit):
 *   row 0: pair(0, 0) = 3, all other cells 0 (:215-216);
 *   row r >= 1: bit0(r, m) = [pair(r - 1, m) != 0] (:221-223),
 *               bit1(r, m) = [m >= w_r and pair(r, m - w_r) != 0] (:230-243);
 *   last column: word == expected & ((full << 2k) & full) for one k in
 *   [0, compression] shared by all rows (:246; max_mass is not known here).
 * By induction over rows, then masses, a table that passes is the built one.
 * Certifiable are alphabets whose rows r >= 1 all have w_r >= compression
 * (rows below follow the reference's literal in-place sweep, a zero row leaves
 * the fixpoint open).  One read-only streaming pass, 16 bytes of output, no
 * scratch buffer.  Takes the ctx lock and waits for the ctx's queued work.
 *   built here or certified before: *certified = 1, nothing runs;
 *   not certifiable: SST_OK, *certified = 0, the table stays as it is;
 *   violation: SST_E_TABLE, first_bad = {row, column} of the first violating
 *     word in row-major order (may be NULL; {-1, -1} otherwise), and
 *     sst_last_error names row, column and the word's mass range.  In the last
 *     column the violating row is the first at which no k fits all rows so
 *     far.  The table stays usable exactly as before the call;
 *   pass: *certified = 1; closure fast paths on, pair list, buckets and census
 *     built, the scan limits refreshed under the budgets set earlier
 *     (sst_table_set_budgets), as after sst_table_build.
 * A result created on this table before certification stays valid and keeps
 * the bitset scan it was sized for whenever it is reused on this table; new
 * results take the pair scan. */
int sst_table_certify(sst_table* t, int* certified, int64_t* first_bad /* [2] row, column; may be NULL */);

/* Row budgets the explain DFS reads from DynamicProgrammingTable.masses:
 * is_mod[r] = NucleotideMass.is_modification, cap[r] =
 * round(seq.max_len * NucleotideMass.modification_rate)
 * (mass_explanation.py:158-172, :200). */
int sst_table_set_budgets(sst_table* t, const uint8_t* is_mod, const int64_t* cap);

int sst_table_shape(const sst_table* t, int* n_rows, int64_t* n_cols, int* compression);
/* Copy the packed table to host (n_rows*n_cols*(compression/4) bytes):
 * the DynamicProgrammingTable.table ndarray (mass_table.py:54). */
int sst_table_download(sst_table* t, void* words_out);
void sst_table_destroy(sst_table* t);

/* is_valid_mass (mass_explanation.py:45-89), one result per query.
 * thr_abs may be NULL (reference default threshold = tolerance*mass). */
int sst_is_valid_batch(sst_table* t, const double* mass, const double* thr_abs, int64_t n, double tolerance,
                       double precision, int8_t* out);
/* Same on device buffers, queued on the ctx stream (no synchronisation). */
int sst_is_valid_batch_device(sst_table* t, const double* d_mass, const double* d_thr_abs, int64_t n,
                              double tolerance, double precision, int8_t* d_out);

/* is_valid_mass over peaks x breakage weights, as classify_fragments maps it
 * over its concatenated frame (fragment_classification.py:39-67): for every
 * peak p and shift k, mass = obs[p] - shifts[k] and threshold = tolerance *
 * obs[p] (shifts[k] = breakage weight x precision, computed by the caller as
 * the reference does); out[k * n_peaks + p] as sst_is_valid_batch
 * (breakage-major, the reference's row order).  Reads each peak once. */
int sst_is_valid_peaks(sst_table* t, const double* obs, int64_t n_peaks, const double* shifts, int n_shifts,
                       double tolerance, double precision, int8_t* out);
int sst_is_valid_peaks_device(sst_table* t, const double* d_obs, int64_t n_peaks, const double* shifts, int n_shifts,
                              double tolerance, double precision, int8_t* d_out);

/* is_singleton (fragment_classification.py:104-119), one result per query:
 * 1 if some value of the quantised window [round(mass/precision) -
 * ceil(thr/precision), ... + ...] is one of masses[0..n_masses) (the caller's
 * integer masses; classify_fragments passes the table's rows, :73-80), else 0.
 * n_masses <= 1024.  thr_abs may be NULL (tolerance*mass). */
int sst_is_singleton_batch(sst_ctx* ctx, const int64_t* masses, int n_masses, const double* mass,
                           const double* thr_abs, int64_t n, double tolerance, double precision, int8_t* out);
/* Same on device buffers, queued on the ctx stream (masses: host array). */
int sst_is_singleton_batch_device(sst_ctx* ctx, const int64_t* masses, int n_masses, const double* d_mass,
                                  const double* d_thr_abs, int64_t n, double tolerance, double precision,
                                  int8_t* d_out);

/* explain_mass_with_table (mass_explanation.py:92-203), batched.
 *   max_mods: per-query budget array (may be NULL) else max_mods_scalar;
 *             a negative value means np.inf (the reference default);
 *   with_memo: the reference's with_memo flag (memo semantics reproduced
 *             exactly, including budget-dependent first-visit effects);
 *   cap_per_query: candidate cap; larger sets report SST_OVERFLOW with the
 *             exact count and no payload.
 *   n <= SST_MAX_EXPLAIN_BATCH per call (the kernels address per-query
 *             arrays with 32-bit byte offsets; split larger batches).
 * Results (host copies) through sst_result_* below. */
#define SST_MAX_EXPLAIN_BATCH (1ll << 29)
int sst_explain_batch(sst_table* t, const double* mass, const double* thr_abs, int64_t n, double tolerance,
                      double precision, const int64_t* max_mods, int64_t max_mods_scalar, int with_memo,
                      uint64_t cap_per_query, sst_result** out);
/* Same with inputs already in HBM; results stay on the device.  Queued on
 * the ctx stream, no host synchronisation: on tables built here the pass is
 * one scan launch that writes the complete result (status bytes, dense hit
 * list, dense payload; see sst_result_hit_list) plus a small header into
 * host-mapped memory (uploaded tables: scan, expand, deferred and pack
 * launches).  If *out is non-NULL it must be a result of the same
 * ctx with capacity >= n: its buffers are reused (no allocation).  The inputs
 * (and the table) must stay valid and unchanged until the pass is settled
 * (sst_result_settle, or the first view / fetch, which settle implicitly):
 * settling waits for the pass and reads its header; only if the scan routed
 * windows to the deferred classes (deep, exact, no-memo and > 2-item windows;
 * the pass launches only the scan and the pack on tables with the pair list)
 * does it launch them and pack again, and only if a query outgrew a payload
 * region, the spill area or the exact path's memo does it re-run the pass
 * with larger workspaces. */
int sst_explain_batch_device(sst_table* t, const double* d_mass, const double* d_thr, int64_t n,
                             double tolerance, double precision, const int64_t* d_max_mods, int64_t max_mods_scalar,
                             int with_memo, uint64_t cap_per_query, sst_result** out);

/* sst_explain_batch_device against per-query reduced alphabets without
 * rebuilding a table: query i is answered as explain_mass_with_table on the
 * table DynamicProgrammingTable._reduce_nucleotide_list (mass_table.py:
 * 94-121) would rebuild for the rows of alphabet d_spec[i] (d_spec null: all
 * queries alphabet 0), given as a row mask over this table's rows:
 * d_alpha[2 g] rows 0..63, d_alpha[2 g + 1] rows 64..127 (row 0, the
 * sentinel, is implied).  The kept rows keep their caps (sst_table_set_budgets
 * of this table).  Every window with values goes to the deferred DFS roles,
 * which walk the alphabet's rows only (the pair scan answers none); a window
 * reaching the reduced table's extent max(kept) * 35 is SST_OUT_OF_TABLE as in
 * the reference, one inside that table's last packed word SST_ABORTED (the
 * reference's last-column mask is not modelled).  Replaces a table rebuild +
 * explain_mass_with_table per alphabet (prediction.py:207 -> :216-227,
 * skeleton_building.py:212 -> :436).  Results, reuse and settling as for
 * sst_explain_batch_device; every d_spec[i] must index d_alpha (device
 * buffers are not range-checked), and d_spec / d_alpha must stay valid until
 * the pass is settled. */
int sst_explain_alpha_batch_device(sst_table* t, const double* d_mass, const double* d_thr, const int32_t* d_spec,
                                   const uint64_t* d_alpha, int64_t n, double tolerance, double precision,
                                   const int64_t* d_max_mods, int64_t max_mods_scalar, int with_memo,
                                   uint64_t cap_per_query, sst_result** out);

/* sst_explain_alpha_batch_device with per-query budgets: query i's row caps
 * are row d_qlen[i] of caps_by_len (host, [n_lens][n_rows]: the caps
 * sst_table_set_budgets would set for that length, round(L * rate)), its
 * max_modifications d_mods[i]; the table's is_modification flags (set by
 * sst_table_set_budgets) are kept.  Every query is answered as one
 * sst_explain_alpha_batch_device call with those budgets set would answer it
 * (the exact memo path: with_memo = 1), so windows of many max_len values
 * go in one pass instead of one pass per value (skeleton_building.py:212 ->
 * :436 per spectrum, each spectrum's SequenceInformation.max_len).  Results,
 * reuse and settling as for sst_explain_batch_device; d_qlen / d_mods must
 * stay valid until the pass is settled. */
int sst_explain_alpha_lens_batch_device(sst_table* t, const double* d_mass, const double* d_thr, const int32_t* d_spec,
                                        const uint64_t* d_alpha, const int32_t* d_qlen, const int64_t* caps_by_len,
                                        int n_lens, int64_t n, double tolerance, double precision,
                                        const int64_t* d_mods, uint64_t cap_per_query, sst_result** out);

/* One step of both predicates on device buffers, as classify_fragments and
 * the explanation stage issue them: sst_is_valid_peaks_device(d_obs, n_peaks,
 * shifts, n_shifts -> d_valid_out) and sst_explain_batch_device(d_mass, ...,
 * out), with the same results.  With 4 breakage weights and a pass whose scan
 * packs its own result, both run in one launch (the pair scan's grid, the
 * is_valid workgroups behind it); otherwise as two launches.  No
 * reference equivalent (it issues the two per row). */
int sst_step_device(sst_table* t, const double* d_obs, int64_t n_peaks, const double* shifts, int n_shifts,
                    int8_t* d_valid_out, const double* d_mass, const double* d_thr, int64_t n, double tolerance,
                    double precision, const int64_t* d_max_mods, int64_t max_mods_scalar, int with_memo,
                    uint64_t cap_per_query, sst_result** out);

/* explain_mass_with_recursion (mass_explanation.py:206-284), batched: the
 * table-free enumerator (target = round(mass/precision), base case
 * |remaining| <= thr at every level, memo keyed (remaining, start) with the
 * first visit's list, per-row caps from sst_table_set_budgets).  max_mods:
 * per-query array or scalar; negative = np.inf; a fractional reference budget
 * is passed floored.  Results as for sst_explain_batch (status, count,
 * offset, payload of ascending row indices); SST_ABORTED when a query
 * exhausts the DFS node budget.  Synchronous. */
int sst_explain_recursion_batch(sst_table* t, const double* mass, const double* thr_abs, int64_t n,
                                double tolerance, double precision, const int64_t* max_mods, int64_t max_mods_scalar,
                                uint64_t cap_per_query, sst_result** out);

/* The step from the peaks: classify_fragments' is_valid and filters
 * (fragment_classification.py:17-101: A7 of every peak x breakage weight into
 * d_valid_out as sst_is_valid_peaks_device, the intensity / mass cuts and
 * filter_by_sequence_mass against d_su_seq[spectrum]) and the first
 * filter_by_explanation round's sliding-window explains of both sides
 * (prediction.py:261-329; no singletons), every producer on the device:
 * per spectrum the kept rows of each side in SU order (a merge of the
 * breakages' sorted streams), the window pairs in closed form and each pair's
 * difference and threshold formed in the kernels.  Spectrum g's peaks are
 * d_obs[d_peak_off[g] .. d_peak_off[g+1]) in any order (at most 1024; a list
 * not in mass order is ranked on the device, equal masses in their given
 * order); sides[k]: bit 0 = breakage k's rows are on the START side, bit 1 = on
 * the END side (both: the sequence-mass lower cut applies); d_intensity may
 * be NULL (every peak passes).  The result holds the explain answers in query
 * order (spectrum-major; START pairs then END pairs; the order
 * collect_diff_explanations_for_su issues them) and the number of queries
 * (sst_result_queries; at most max_queries); its hits all come from the pair
 * list (sst_result_pair_hits, n_scan_wg = 0: query order).  Every window must
 * be pair-class with budgets that cannot bind (checked: SST_E_ARG otherwise).
 * No reference equivalent (the reference issues these one row at a time). */
int sst_step_rows_device(sst_table* t, const double* d_obs, const int64_t* d_peak_off, int64_t n_spec,
                         int64_t n_peaks, const double* d_intensity, double intensity_cutoff, double mass_cutoff,
                         const double* d_su_seq, const double* shifts, const uint8_t* sides, int n_shifts,
                         double max_weight, double tolerance, double precision, int64_t max_mods_scalar,
                         uint64_t cap_per_query, int64_t max_queries, int8_t* d_valid_out, sst_result** out);
/* Number of explain queries of a result (settles it first). */
int sst_result_queries(sst_result* r, int64_t* n);

/* Wait for a result's pass and complete it (see sst_explain_batch_device);
 * reports the dense hit list's length and the dense payload's size.  Other
 * work queued on the ctx stream after the pass keeps running.  No reference
 * equivalent. */
int sst_result_settle(sst_result* r, uint64_t* n_hits, uint64_t* payload_bytes);

/* Host views of a result (valid until sst_result_free; filled by
 * sst_result_fetch, which sst_explain_batch calls):
 *   status[n] (SST_NONE..), count[n] candidates, offset[n] byte offset of the
 *   query's candidates in payload; payload = per candidate one length byte k
 *   followed by k row indices (ascending, i.e. ascending mass); a query's
 *   candidates may be followed by unused bytes (count delimits them).
 *   count[i] and offset[i] are 0 unless status[i] is SST_SOME, SST_OVERFLOW
 *   or SST_ABORTED (the host builds them from the hit list). */
int sst_result_host(sst_result* r, const int8_t** status, const uint64_t** count, const uint64_t** offset,
                    const uint8_t** payload, uint64_t* payload_bytes);
/* Ordering of a result's device buffers: they are written on the stream that
 * was the ctx's stream when the pass was queued (the pass stream); settling
 * queues any further launches (deferred classes, pack, retries) on that same
 * stream, whatever the ctx's stream is at the time.  sst_wire_pack, the views
 * and fetch wait (hipStreamWaitEvent) for the work settling queued when they
 * run on another stream; the pass's own kernels are the caller's to order
 * (e.g. an event recorded on the pass stream right after the launch). */
/* Device views (no copy; settle the result first).  d_status and d_payload
 * (the dense payload) are the pass's own output.  d_count / d_offset are
 * per-query u64 arrays built from the hit list only when asked for (pass
 * NULL to skip them: 16 B per query of extra HBM traffic); their entries are
 * undefined for queries without candidates. */
int sst_result_device(sst_result* r, int8_t** d_status, uint64_t** d_count, uint64_t** d_offset,
                      uint8_t** d_payload, uint64_t* payload_bytes);
/* The dense hit list of a result, on the device (settles it first): one
 * 16-B record {u32 query, u32 count (saturated), u32 word lo, u32 word hi}
 * per query with candidates (SOME, OVERFLOW, ABORTED), where word is the
 * byte offset of the query's candidates in the dense payload (SOME) or the
 * exact candidate count (OVERFLOW, ABORTED: no payload).  Records come in the
 * engine's order (per scan wave, then the deferred paths).  With the status
 * bytes and the payload this is the whole result in ~1 B/query + 16 B per hit
 * (the wire format bench.py --gather sends over RCCL).  Valid until the next
 * pass on this result or its free.  No reference equivalent. */
int sst_result_hit_list(sst_result* r, void** d_hits, uint64_t* n_hits);
/* The pair-path part of a device-path result (settles it first): its first
 * *n_pair_hits dense records are the hits the scan answered from the pair
 * list, and their candidates occupy the first *pair_bytes of the dense
 * payload.  d_refs (u16, one per such record): the first pair-list entry of
 * the query's candidates (entries first .. first + count - 1, records as
 * sst_table_pair_records returns them), | 0x8000 for OVERFLOW.  The records
 * come in the scan's order: workgroup b < *n_scan_wg, its wave w < 16, then
 * that wave's tiles (64 queries each; wave w of workgroup b takes tiles
 * v, v + 16 * n_scan_wg, ... with v = ((w >> 1) * n_scan_wg + b) * 2 + (w & 1)),
 * ascending query within a tile.  0 pair hits after passes that were not
 * fused (host entry points, retries, tables without the pair list).  With
 * the status codes this is the whole pair-path result in ~4 B per hit and
 * no payload (parallel.wire_pack).  No reference equivalent. */
int sst_result_pair_hits(sst_result* r, void** d_refs, uint64_t* n_pair_hits, uint64_t* pair_bytes, int* n_scan_wg);
/* Hit records each scan wave of a device-path pass on this table keeps on
 * chip (LDS) before it falls back to its worklist region in device memory:
 * the most that leaves the scan's occupancy alone for the table's pair list,
 * or what SST_SCAN_LDS_HITS forces (0 for tables without the list).  Results
 * do not depend on it.  No reference equivalent. */
int sst_table_scan_lds_hits(sst_table* t, uint32_t* per_wave);
/* The table's pair list: payload record of entry e (u32: [k][row..] in its
 * low 2-3 bytes, the bytes sst_result_host's payload holds for that
 * candidate); *n = 0 for tables without the list.  recs may be NULL (size
 * query). */
int sst_table_pair_records(sst_table* t, uint32_t* recs, int64_t cap, int64_t* n);
/* One rank's complete step result in the gather's wire format v5, packed on
 * the device by one kernel on the ctx stream (settles r first): d_valid the
 * step's n_valid is_valid codes (int8 -1 / 0 / 1), r its explain result.
 * The layout (8-B aligned sections; spectrseqtools_amd/parallel.py,
 * wire_unpack, decodes it):
 *   header   16 x u64: magic "SSTW5", n_valid, n_explain, n_pair, n_explicit,
 *            explicit payload bytes, n_scan_wg, pair key (FNV-1a of the pair
 *            records), w, n_list, list capacity, list offset, 4 x 0
 *   valid    1 bit per is_valid query: True
 *   status   1 bit per explain query: 1 = SOME / OVERFLOW / ABORTED (a hit),
 *            0 = NONE or listed
 *   first    per pair hit (sst_result_pair_hits, scan order) its first
 *            pair-list entry in w bits, w = ceil(log2(pair-list entries))
 *   codes    per pair hit 3 bits, 10 per u32: its count 1..7, 0 = listed
 *   explicit 12-B records {u32 query | kind << 30, u32 a, u32 b} of the
 *            other hits: kind 0 SOME (a = candidates, b = payload offset),
 *            1 OVERFLOW / 2 ABORTED (a, b = the exact count)
 *   payload  the explicit hits' payload
 *   list     n_list 8-B entries {u32 index | type << 30, u32 value}, in no
 *            particular order: type 0 an is_valid raise, 1 an explain status
 *            other than NONE / SOME (value: the status byte; EMPTY, raises,
 *            OVERFLOW, ABORTED), 2 a pair hit's
 *            count outside 1..7 (index: the pair hit, value: the count)
 * d_out NULL: returns the fixed part's bytes (the list's offset) and packs
 * nothing; otherwise cap (>= that) bounds the buffer and entries beyond it
 * are dropped (the header's n_list still counts them: the receiver checks).
 * d_out must be 8-byte aligned.  Returns the fixed part's bytes or a
 * negative SST_E_*.  No reference equivalent (the north star's RCCL gather of
 * candidate compositions). */
int64_t sst_wire_pack(sst_result* r, const int8_t* d_valid, int64_t n_valid, void* d_out, int64_t cap);
/* Copy device results to the host views (synchronises the ctx stream). */
int sst_result_fetch(sst_result* r);
void sst_result_free(sst_result* r);

/* Counters of the last explain launch (valid after a fetch), for measurement:
 * [0] queries run by the shallow (<= 3 item) fast path, [1] deep fast path,
 * [2] exact (budget-binding) path, [3] no-memo path, [4] index records loaded
 * (node expansions of the counting pass), [5] payload bytes written by those
 * paths, [6] queries answered from the on-chip pair list (<= 2 item windows),
 * [7] payload bytes written by the pair-list path. */
int sst_result_stats(const sst_result* r, uint64_t* stats_out /* [8] */);

/* compute_sequence_length_bound (spectrseqtools/mass_table.py:343-487),
 * batched over (su_mass, obs_mass) pairs: window = round(su/precision) +-
 * ceil(tolerance*obs/precision); max_mods = round(seq.modification_rate *
 * seq.max_len) (:351); per-row caps from sst_table_set_budgets; direction 0 =
 * "lower", 1 = "upper", optionally | SST_LB_EXACT_ONLY | SST_LB_REPLAY.
 * Windows whose budgets provably never bind come from layered reachability;
 * the others, on a table built here (a closure of its rows), from the
 * first-visit frontier (as sst_length_bounds_frontier_device, with the
 * table's own rows; a 4 GB workspace kept in the ctx), or from the replay
 * of the memoised DFS (windows in the table's last packed word, tables
 * uploaded as they are, SST_LB_REPLAY).  out[i] = the bound; status[i]: 0
 * ok, SST_OUT_OF_TABLE (the reference raises NotImplementedError),
 * SST_LB_EMPTY_WINDOW (its min([]) raises ValueError), SST_ABORTED (DFS node
 * budget exhausted: no bound).  max_len <= 253 (the frontier's u8 values);
 * a window only the replay answers needs max_len <= 120 (SST_E_ARG with a
 * message otherwise).  Synchronous, host buffers. */
#define SST_LB_EMPTY_WINDOW (-5)
/* sst_length_bound_batch on per-query reduced alphabets (the table
 * adapt_individual_modification_rates_by_alphabet_reduction would rebuild,
 * mass_table.py:94-121, as select_sequence_length_with_jaccard / _with_lp
 * call it after reducing to the skeleton's nucleotides, skeleton_building.py:
 * 212-224, 324-336): query i on alphabet spec[i] (spec NULL: alphabet 0) of
 * n_alpha row masks alpha[2 g], alpha[2 g + 1] over the table's rows; the
 * exact replay with the mask, no table rebuilt.  A window reaching the reduced
 * table's extent is SST_OUT_OF_TABLE, one in its last packed word
 * SST_ABORTED (as sst_explain_alpha_batch_device).  direction must be 0
 * ("lower"; SST_E_ARG otherwise): the reference's upper bound counts a
 * visited child that returned the default as -1 + 1 = 0, and the masked walk
 * visits children the rebuilt table would not (reachable only with dropped
 * rows), so "upper" needs the rebuilt table.  Host buffers. */
int sst_length_bound_alpha_batch(sst_table* t, const double* su_mass, const double* obs_mass, const int32_t* spec,
                                 const uint64_t* alpha, int64_t n_alpha, int64_t n, double tolerance,
                                 double precision, int max_len, int64_t max_mods, int direction, int64_t* out,
                                 int8_t* status);
#define SST_LB_EXACT_ONLY 2 /* direction flag: skip the layered fast path (tests) */
#define SST_LB_REPLAY 4     /* direction flag: the replay instead of the first-visit frontier (tests) */
int sst_length_bound_batch(sst_table* t, const double* su_mass, const double* obs_mass, int64_t n, double tolerance,
                           double precision, int max_len, int64_t max_mods, int direction, int64_t* out,
                           int8_t* status);

/* ---- per-spectrum reduced alphabets ---------------------------------- */
/* Predictor.filter_by_explanation (prediction.py:170-227) reduces every
 * spectrum's alphabet to the modifications its explanations name
 * (adapt_individual_modification_rates_by_alphabet_reduction,
 * mass_table.py:94-121) and then queries the table rebuilt for that alphabet
 * (set_up_bit_table over the kept rows, max_mass = max(kept) * 35).  Over many
 * spectra these entry points answer those rebuilt tables' queries without
 * building them: spectrum g's alphabet is a row subset of t, the bits of
 * masks[2g] (rows 0..63) and masks[2g + 1] (rows 64..119); row 0 is implied;
 * the canonical rows are never dropped by the reference, so every alphabet
 * holds t's lightest row. */

/* explain_mass_with_table (mass_explanation.py:92-203) on pair-class windows
 * (hi < 3 * the lightest row mass: every candidate has <= 2 items) of query i
 * against the table of spectrum spec[i]'s alphabet: the candidates are t's
 * pair-list entries whose rows lie in the alphabet, in the reference's order.
 * The caller guarantees the budgets cannot bind (as for any pair-class window
 * with max_modifications >= 2 and per-row caps >= 2).  Out per query: status
 * (SST_NONE / SST_EMPTY / SST_SOME; -10 for a window that is not pair-class,
 * which the caller answers otherwise), the candidate count, the union of the
 * candidates' rows (rowmask[2i], rowmask[2i + 1]) and the window's pair-list
 * entry range range[2i] .. range[2i + 1] (its candidates are the entries of
 * that range whose rows are all in the alphabet; sst_table_pair_records).
 * t must carry the pair list.  No reference equivalent (batched). */
int sst_explain_pairs_alpha_device(sst_table* t, const double* d_mass, const double* d_thr, const int32_t* d_spec,
                                   const uint64_t* d_masks, int64_t n, double tolerance, double precision,
                                   int8_t* d_status, uint32_t* d_count, uint64_t* d_rowmask, uint32_t* d_range);
int sst_explain_pairs_alpha(sst_table* t, const double* mass, const double* thr, const int32_t* spec,
                            const uint64_t* masks, int64_t n_spec, int64_t n, double tolerance, double precision,
                            int8_t* status, uint32_t* count, uint64_t* rowmask, uint32_t* range);
/* is_valid_mass (mass_explanation.py:45-89) against the table of each
 * spectrum's alphabet (its last row: reachability by the alphabet's rows,
 * the reduced table's extent and last-column mask included): spectrum g's
 * queries are mass/thr[offsets[g] .. offsets[g+1]), in ascending mass order
 * (classify_fragments' SU order).  out as sst_is_valid_batch; -10 marks a
 * query the kernel could not answer (queries out of mass order). */
int sst_is_valid_alpha_device(sst_table* t, const double* d_mass, const double* d_thr, const int64_t* d_offsets,
                              int64_t n_spec, const uint64_t* d_masks, double tolerance, double precision,
                              int8_t* d_out);
int sst_is_valid_alpha(sst_table* t, const double* mass, const double* thr, const int64_t* offsets, int64_t n_spec,
                       const uint64_t* masks, double tolerance, double precision, int8_t* out);

/* ---- query producers (host code, no device) --------------------------- */
/* The sliding window of collect_explanations_per_side
 * (spectrseqtools/prediction.py:286-329) over many sides at once: side j is
 * su[offsets[j] .. offsets[j+1]) (SU masses sorted ascending); every (start,
 * end) pair whose difference the reference explains, in its order (including
 * its quirk: once `end` reaches the last fragment, later starts pair only with
 * it until a difference exceeds max_weight), as indices into su.  cap: room in
 * start_out / end_out; the return value is the number of pairs (> cap: nothing
 * beyond cap written, call again with more room) or a negative SST_E* code. */
int64_t sst_window_pairs(const double* su, const int64_t* offsets, int64_t n_sides, double max_weight,
                         int64_t* start_out, int64_t* end_out, int64_t cap);
/* The first filter_by_explanation round's queries over many spectra
 * (spectrseqtools/prediction.py:261-329, collect_diff_explanations_for_su):
 * spectrum g's rows su/obs[offsets[g] .. offsets[g+1]) (classify_fragments'
 * rows, ascending SU mass); flags per row: 1 START side, 2 END side, 4
 * singleton.  Per spectrum, in the reference's order: the START side's
 * sliding-window pairs, the END side's, then the singletons: diff = su[end] -
 * su[start] (a singleton: its su), thr = tolerance * (obs[start] + obs[end])
 * (a singleton: tolerance * obs), spec = g, kind = 0 / 1 / 2.  Returns the
 * number of queries (> cap: nothing written) or SST_E*.  Spectra are split
 * over up to 16 host threads. */
int64_t sst_su_diff_queries(const double* su, const double* obs, const uint8_t* flags, const int64_t* offsets,
                            int64_t n_spec, double max_weight, double tolerance, double* diff, double* thr,
                            int64_t* spec, int8_t* kind, int64_t cap);
/* ---- config 5 on the device ---------------------------------------------
 * classify_fragments and the filter_by_explanation fixpoint over many spectra
 * with every array in HBM (the row slots: sst_row_slots).  Peaks in any order
 * (ranked by mass on the device, equal masses in their given order), <= 16383
 * per spectrum (above 4096 in the reserved HBM slices); shifts / sides as
 * sst_step_rows_device.  A spectrum of more than 2048 rows is held in HBM
 * slices the table's context reserves (sst_pipe_reserve_rows, before the
 * stages run); without them it is an error.  d_err collects | 1 a spectrum over 16383 peaks (or over 4096 with
 * no slices reserved), 2 over 2048 rows with no slices reserved (or over
 * the reserved rows), 4 a window outside the pair class, 8 a window past a
 * table's end (the reference raises), 16 a dict too large for its hash, 32
 * rows out of mass order; the caller checks it. */
/* The row slots: rows of spectrum g live in slots 4 * peak_off[g] + i,
 * i < cnt[g] (su / obs / meta / alive: arrays of 4 * n_peaks).
 * sst_classify_rows_device writes every array but peak_off (its input);
 * sst_fix_round_device and sst_valid_rows_alpha_device write alive (the rows a
 * round keeps); every other stage only reads.  An entry point may leave null
 * the arrays it does not take: sst_valid_rows_alpha_device needs no meta,
 * sst_fix_finish_device needs only cnt; all others need every array (with
 * n_spec > 0).  Device pointers. */
typedef struct sst_row_slots {
  int64_t n_spec;
  const int64_t* peak_off; /* [n_spec + 1] */
  double* su;              /* standard-unit mass, ascending per spectrum */
  double* obs;             /* observed mass */
  uint32_t* meta;          /* breakage | sides << 2 | is_singleton << 4 | peak position << 8 */
  uint8_t* alive;
  uint32_t* cnt;           /* [n_spec] rows per spectrum */
} sst_row_slots;
/* Reserve the context's slices for spectra of up to max_rows rows (<= 65532:
 * 4 breakages x 16383 peaks) in the row stages (classify above 4096 peaks, fix
 * rounds, final dict, bins);
 * a no-op for max_rows <= 2048 or at most what is reserved.  Synchronises the
 * context's stream when it grows. */
int sst_pipe_reserve_rows(sst_table* t, int64_t max_rows);
/* classify_fragments (fragment_classification.py:17-101): A7 into valid_out,
 * the filters, is_singleton against t's masses, SU order. */
typedef struct sst_classify_args {
  const double* obs;       /* [n_peaks] every spectrum's peaks (spectrum g: peak_off[g] .. peak_off[g + 1]) */
  int64_t n_peaks;
  const double* intensity; /* [n_peaks], may be NULL: no intensity filter */
  double intensity_cutoff, mass_cutoff;
  const double* su_seq;    /* [n_spec] SequenceInformation.su_mass */
  const double* shifts;    /* [n_shifts] host: breakage weights * precision */
  const uint8_t* sides;    /* [n_shifts] host: START = 1 | END = 2 per breakage */
  int n_shifts;            /* 1 .. 4 */
  double max_weight, tol, prec;
  int8_t* valid_out;       /* may be NULL: the A7 codes [n_shifts * n_peaks], breakage-major */
} sst_classify_args;
int sst_classify_rows_device(sst_table* t, const sst_row_slots* rows, const sst_classify_args* a, uint32_t* d_err);
/* Budget-binding ("exact mode") spectra of the device pipeline: a spectrum
 * whose max_modifications or modification caps are < 2 (a small
 * --modification_rate, or max_len <= 2: mass_explanation.py:158-172) can have
 * its budgets bind on pair-class windows, where the pair list's answers are
 * not the reference's.  With x->pair_ok[g] == 0 the stage lists the
 * spectrum's queries instead of answering them: x->xq_mass / xq_thr /
 * xq_spec / xq_single[...] in one block per spectrum (x->xq_block[g] = start
 * << 32 | count; *x->xq_count the list length, x->xq_cap its capacity, d_err
 * bit 64 on overflow); the caller answers the list with the exact masked
 * explain (sst_explain_alpha_batch_device, per max_len group) and
 * sst_result_refs_device into x->xa_st / xa_n / xa_ptr, then runs the stage's
 * second half (sst_fix_finish_device, sst_dict_build_device).  x may be NULL:
 * every spectrum's pair-class answers are exact. */
typedef struct sst_exact_io {
  const uint8_t* pair_ok;  /* [n_spec] */
  double* xq_mass;
  double* xq_thr;
  int32_t* xq_spec;
  uint8_t* xq_single;      /* 1: a singleton's query (stored in the dict even when empty) */
  uint32_t* xq_count;
  uint64_t xq_cap;
  uint64_t* xq_block;      /* [n_spec] */
  const int8_t* xa_st;
  const uint32_t* xa_n;
  const uint64_t* xa_ptr;
} sst_exact_io;

/* One filter_by_explanation round (prediction.py:170-202) of the spectra with
 * active[g]: their alive rows' window pairs and singletons explained
 * against alpha[2g..2g+1] (row masks of t; the caller keeps budgets from
 * binding, see sst_explain_pairs_alpha), the explanation dict's surviving
 * entries, alpha_next = the canonical rows | (alphabet & observed rows),
 * active_next[g] = the alphabet shrank (*n_active, zeroed by the call, counts those);
 * rounds[g] += 1, queries[g] += the round's explain queries.  Settled
 * spectra carry their alphabet over.  Device pointers. */
typedef struct sst_fix_args {
  const uint64_t* alpha; /* [2 n_spec] */
  uint64_t* alpha_next;  /* [2 n_spec] */
  const uint8_t* active; /* [n_spec] */
  uint8_t* active_next;  /* [n_spec] */
  uint32_t* rounds;      /* [n_spec] */
  uint32_t* queries;     /* [n_spec] */
  uint32_t* n_active;
  double max_weight, tol, prec; /* the round only */
} sst_fix_args;
int sst_fix_round_device(sst_table* t, const sst_row_slots* rows, const sst_fix_args* a, uint32_t* d_err,
                         const sst_exact_io* x);
/* The exact-mode spectra's half of the round, after their listed queries
 * were answered (same arrays as the round; of rows only cnt; x required). */
int sst_fix_finish_device(sst_table* t, const sst_row_slots* rows, const sst_fix_args* a, uint32_t* d_err,
                          const sst_exact_io* x);
/* SkeletonBuilder._predict_skeleton's speculative bin queries
 * (skeleton_building.py:114-160; replaces the per-bin explain calls of
 * :131-160 for every spectrum at once) over the rows a fixpoint kept
 * (rows->alive), on each spectrum's alphabet alpha: per side, bins are runs of
 * rows whose SU step is <= tol * (obs_prev + obs); the side's first bin
 * explains its rows' SU masses against 0 (threshold tol * obs), every later
 * bin each (predecessor row, row) difference (tol * (obs_p + obs_r)); a
 * side's last bin only with >= 2 rows.  Two calls: count (n_q[S] queries
 * per spectrum, q_off[S + 1] their exclusive offsets, the total last), then
 * emit into status / count [total], spectrum-major (START side, then END;
 * bins in order; a bin's pairs predecessor-row-major).  Statuses SST_NONE /
 * EMPTY / SOME, or -10 for a window outside the pair class (hi >= 3 w_min:
 * the caller's general path).  With n_def non-null (zeroed by the caller),
 * those windows are also listed, in any order, for
 * sst_explain_alpha_batch_device: def_mass / def_thr / def_spec /
 * def_q[*n_def] = window mass, threshold, spectrum and index into
 * status (capacity: the total).  d_err bit 2: a spectrum over 2048 rows
 * with no slices reserved (sst_pipe_reserve_rows).  Device pointers.
 * sst_bins_count_device reads tol and writes n_q, n_q0, q_off;
 * sst_bins_emit_device reads every field but n_q, n_q0. */
typedef struct sst_bins_args {
  const uint64_t* alpha;  /* [2 n_spec] */
  double tol, prec;
  uint32_t* n_q;          /* [n_spec] */
  uint32_t* n_q0;         /* may be NULL: the START side's count per spectrum */
  uint64_t* q_off;        /* [n_spec + 1] */
  int8_t* status;         /* [total] */
  uint32_t* count;        /* [total] */
  double* def_mass;
  double* def_thr;
  int32_t* def_spec;
  uint64_t* def_q;
  uint32_t* n_def;        /* may be NULL: the windows outside the pair class are not listed */
  const uint8_t* pair_ok; /* may be NULL; 0: list every window */
} sst_bins_args;
int sst_bins_count_device(sst_table* t, const sst_row_slots* rows, const sst_bins_args* a, uint32_t* d_err);
int sst_bins_emit_device(sst_table* t, const sst_row_slots* rows, const sst_bins_args* a, uint32_t* d_err);

/* _reduce_alphabet's filter (prediction.py:211-227): is_valid_mass of the
 * alive rows of the d_active spectra against their reduced tables (d_alpha),
 * AND-ed into rows->alive.  A spectrum whose alphabet did not change needs no
 * re-filter (its rows already passed that table), so a fixpoint passes the
 * round's changed flags (sst_fix_args.active_next).  rows->meta is not read. */
int sst_valid_rows_alpha_device(sst_table* t, const sst_row_slots* rows, const uint64_t* d_alpha,
                                const uint8_t* d_active, double tolerance, double precision, uint32_t* d_err);

/* The explanation dict collect_diff_explanations_for_su builds per spectrum
 * (prediction.py:261-284): spectrum g's queries [offsets[g], offsets[g+1])
 * in its order (START pairs, END pairs, singletons) with kind 0 / 1 / 2, their
 * dict key (the difference, or the singleton's SU mass), explain status and
 * candidate row union (2 x u64).  Side pairs are stored only with >= 1
 * explanation, singletons always; a later store of an equal key replaces the
 * earlier one.  keep[i] = 1 for the queries whose answers the finished dict
 * holds; union_out[2g..2g+1] = the rows of those answers (the observed
 * nucleotides of filter_by_explanation, :189-195).  Returns the number of
 * dict entries over all spectra, or SST_E*.  Host code, up to 16 threads. */
int64_t sst_dict_union(const int64_t* offsets, int64_t n_spec, const double* key, const int8_t* kind,
                       const int8_t* status, const uint64_t* rowmask, uint8_t* keep, uint64_t* union_out);
/* order[0..n): the row permutation that sorts by group (0 <= group < n_groups)
 * then key ascending, ties in row order -- classify_fragments' per-spectrum
 * sort by standard_unit_mass (fragment_classification.py:84), for many
 * spectra (numpy.lexsort((rows, key, group))). */
int sst_sort_rows(const int64_t* group, const double* key, int64_t n, int64_t n_groups, int64_t* order);

/* ---- config 5: SkeletonBuilder._predict_skeleton's walk --------------- */
/* One lane per (spectrum, side) walks the side's rows the fixpoint kept
 * (skeleton_building.py:114-196): bins, each closed bin explained against the
 * last bin with explanations (explain_bin_differences :372-421, the first
 * against 0) after filter_by_explanation's final dict (:423-440),
 * update_skeleton_for_given_explanations (:442-482) with CPython's set order
 * (sst_pyset_order; name hashes from the caller's interpreter), min_end /
 * max_end per bin.  Pair-class windows are answered in the lane; the others
 * come from the masked explain: stage 3's speculative queries (s_*), and
 * re-queries (a bin explained against an older bin) listed by the lane when
 * their answers are missing -- the side is then SST_WALK_SUSPENDED, and the
 * caller answers req_* (sst_explain_alpha_batch_device), adds them as round
 * n_rounds (rq_*: per side its block start << 32 | count in the round's
 * lists) and walks the suspended sides again: with resume set and the same
 * scratch slots, each resumes at the bin that suspended it (its loop state
 * is kept at the head of its slot), otherwise it replays from the start.
 * SST_WALK_BIG: a bin outgrew the lane's scratch capacities (walk that side
 * again with larger ones).  All pointers are device pointers. */
#define SST_WALK_MAX_ROUNDS 16
#define SST_WALK_DONE 0
#define SST_WALK_SUSPENDED 1
#define SST_WALK_BIG 2
#define SST_WALK_RAISE 3   /* an answer raised in the reference (window past the reduced table) */
#define SST_WALK_LIMIT 4   /* an engine limit: rows, positions, request list, OVERFLOW / ABORTED answer */
#define SST_WALK_ROUNDS 5  /* more than SST_WALK_MAX_ROUNDS re-query rounds */
#define SST_WALK_MISSING 6 /* a DFS answer was not supplied */
typedef struct sst_walk_args {
  const int64_t* peak_off;   /* [n_spec + 1]: rows of spectrum g at slots 4 peak_off[g] + i (SU order) */
  const uint32_t* cnt;       /* [n_spec] rows */
  const double* r_su;
  const double* r_ob;
  const uint32_t* r_meta;    /* breakage | sides << 2 | singleton << 4 | peak << 8 */
  const uint8_t* alive;      /* the rows the fixpoint kept */
  const uint64_t* alpha;     /* [2 n_spec] the fixpoint's alphabets (row masks) */
  const int32_t* max_len;    /* [n_spec] SequenceInformation.max_len */
  const uint8_t* pair_ok;    /* [n_spec] budgets cannot bind on pair-class windows */
  int64_t n_spec;
  int64_t slots;             /* 4 * peaks */
  double tol, prec, rprec;
  const uint64_t* d_off;     /* the final dict (sst_dict_build_device) */
  const uint32_t* d_n;
  const uint64_t* d_key;
  const double* d_thr;
  const uint64_t* q_off;     /* stage 3 (sst_bins_count_device): per spectrum its queries' offset */
  const uint32_t* q0;        /* and its START side's count */
  const uint64_t* s_ptr;     /* per stage-3 query off the pair class: first payload record (sst_result_refs_device) */
  const uint32_t* s_n;
  const int8_t* s_st;
  int n_rounds;
  const uint64_t* rq_block[SST_WALK_MAX_ROUNDS];
  const uint64_t* rq_ptr[SST_WALK_MAX_ROUNDS];
  const uint32_t* rq_n[SST_WALK_MAX_ROUNDS];
  const int8_t* rq_st[SST_WALK_MAX_ROUNDS];
  uint64_t* req_block;       /* [2 n_spec] this round's blocks (zeroed by the caller) */
  double* req_mass;
  double* req_thr;
  int32_t* req_spec;
  uint32_t* req_count;
  uint64_t req_cap;
  const int64_t* name_hash;  /* [n_rows] hash() of each row's nucleoside name */
  const uint32_t* sides;     /* side ids 2 g + (0 START, 1 END) to walk */
  uint32_t n_sides;
  uint8_t* scratch;          /* scratch_stride bytes per slot (sst_walk_scratch_bytes) */
  uint64_t scratch_stride;
  uint32_t pos_cap, len_cap, expl_cap, cand_cap, tset_cap;  /* len_cap = max max_len + 2 <= 255 */
  uint16_t* side_rows;       /* [2 slots] */
  const uint64_t* skel_off;  /* [n_spec] exclusive prefix of 2 max_len */
  uint64_t* skel;            /* spectrum g, side sd, position i: masks at 2 (skel_off[g] + sd max_len[g] + i) */
  int32_t* min_end;          /* [2 slots] per side */
  int32_t* max_end;
  uint8_t* kept;             /* [2 slots] per side: not rejected by the walk */
  uint8_t* side_status;      /* [2 n_spec] SST_WALK_* */
  uint32_t* n_suspended;
  uint32_t* n_big;
  const uint32_t* slot;      /* [n_sides] each walked side's scratch slot (NULL: its index in sides) */
  int resume;                /* a side whose slot holds its suspended state resumes there (else it
                                walks from the start; slots of a first launch hold no state) */
} sst_walk_args;
/* Scratch bytes per walked side for the given capacities (pos_cap, tset_cap:
 * powers of two >= the set tables the positions / a query's candidates need,
 * sst_pyset_table_size). */
uint64_t sst_walk_scratch_bytes(uint32_t pos_cap, uint32_t len_cap, uint32_t expl_cap, uint32_t cand_cap,
                                uint32_t tset_cap);

/* The walk's re-query answers merged over rounds (skeleton_device's round
 * loop; skeleton_building.py:114-196 issues them one explain call at a time,
 * the device walk suspends and resumes, so a side's k-th re-query answer must
 * be entry k of its merged list).  Per side sid of n_sides: the earlier
 * rounds' merged entries (o_block[sid] = start << 32 | count into o_ptr /
 * o_n / o_st; o_block NULL for the first round), then this round's
 * (block[sid] likewise into ptr / n / st) -> m_block[sid] = start << 32 |
 * count into m_ptr / m_n / m_st, sides in order.  m_* must hold the earlier
 * rounds' total plus this round's entries; tot (u32[n_sides]) and off
 * (u64[n_sides + 1]) are device scratch.  Device pointers, the ctx's stream. */
typedef struct sst_requery_merge_args {
  const int64_t* o_block;
  const uint64_t* o_ptr;
  const uint32_t* o_n;
  const int8_t* o_st;
  const int64_t* block;
  const uint64_t* ptr;
  const uint32_t* n;
  const int8_t* st;
  int64_t n_sides;
  int64_t* m_block;
  uint64_t* m_ptr;
  uint32_t* m_n;
  int8_t* m_st;
} sst_requery_merge_args;
int sst_requery_merge_device(sst_table* t, const sst_requery_merge_args* args, uint32_t* d_tot, uint64_t* d_off);
/* CPython's table size after n distinct additions to an empty set. */
uint32_t sst_pyset_table_size(uint32_t n);
int sst_skel_walk_device(sst_table* t, const sst_walk_args* a);
/* Candidate references of a result's queries (settles it first): for query
 * i, d_st[d_dst[i]] = its status, d_n[...] = its candidates (SOME) or exact
 * count (OVERFLOW / ABORTED), d_ptr[...] = the device address of its first
 * payload record (SOME; else 0).  Valid while the result lives unchanged. */
int sst_result_refs_device(sst_result* r, const int64_t* d_dst, uint64_t* d_ptr, uint32_t* d_n, int8_t* d_st);
/* filter_by_explanation's final explanation dict per spectrum
 * (prediction.py:261-329 over the final rows and alphabet).  Count pass
 * (sst_dict_count_device; reads max_weight, tol): n_q[g] = the last round's
 * queries, off = their exclusive offsets (n_spec + 1 entries, total last);
 * build pass (sst_dict_build_device; every field but n_q): keys ascending
 * (double bits) and the last writer's threshold into [off[g], + n_ent[g]).
 * sst_dict_list_device (reads max_weight, tol; x required): the exact-mode
 * spectra's final-round queries listed for the masked explain (before
 * sst_dict_build_device, which then reads x->xa_*).  Device pointers. */
typedef struct sst_dict_args {
  const uint64_t* alpha; /* [2 n_spec] */
  double max_weight, tol, prec;
  uint32_t* n_q;         /* [n_spec] */
  uint64_t* off;         /* [n_spec + 1] */
  uint64_t* key;         /* [total] */
  double* thr;           /* [total] */
  uint32_t* n_ent;       /* [n_spec] */
} sst_dict_args;
int sst_dict_count_device(sst_table* t, const sst_row_slots* rows, const sst_dict_args* a, uint32_t* d_err);
int sst_dict_build_device(sst_table* t, const sst_row_slots* rows, const sst_dict_args* a, uint32_t* d_err,
                          const sst_exact_io* x);
int sst_dict_list_device(sst_table* t, const sst_row_slots* rows, const sst_dict_args* a, uint32_t* d_err,
                         const sst_exact_io* x);

/* select_sequence_length_with_jaccard (skeleton_building.py:315-370) and
 * combine_skeleton_sequences (:494-516) per spectrum, one lane each: the
 * START skeleton and the reversed END skeleton (sst_walk_args.skel layout),
 * the two length bounds on the skeleton alphabet (sst_length_bounds_reach_
 * device) and that alphabet's row masses; validate_sequence_length_by_mass
 * (:291-313) in the reference's float order (sequential f64 sums, CPython
 * 3.10's sum()).  Outputs: seq_len[g], the combined skeleton (masks at
 * 2 (comb_off[g] + i), i < seq_len[g]; comb_off[g] + max_len[g] positions
 * reserved) and status[g]: SST_JAC_OK, SST_JAC_NO_LENGTH (the reference's
 * "No sequence length fitting ..." Exception), SST_JAC_INDEX (an IndexError
 * in combine_skeleton_sequences: seq_len > max_len), SST_JAC_BOUNDS (a
 * length bound raised: status_lb[g] != 0). */
#define SST_JAC_OK 0
#define SST_JAC_NO_LENGTH 1
#define SST_JAC_INDEX 2
#define SST_JAC_BOUNDS 3
typedef struct sst_jaccard_args {
  int64_t n_spec;
  const int32_t* max_len;     /* [n_spec] */
  const uint64_t* skel_off;   /* [n_spec] as sst_walk_args.skel_off */
  const uint64_t* skel;
  const int64_t* lower;       /* [n_spec] the length bounds */
  const int64_t* upper;
  const int8_t* status_lb;
  const double* su_mass;      /* [n_spec] SequenceInformation.su_mass */
  const double* row_mass;     /* [n_rows] integer mass * precision (nucleoside_masses) */
  const uint64_t* comb_off;   /* [n_spec] exclusive prefix of max_len */
  uint64_t* comb;             /* combined skeleton masks */
  int32_t* seq_len;
  int8_t* status;
  double max_variance;        /* fragment_classification.MAX_VARIANCE */
} sst_jaccard_args;
int sst_jaccard_device(sst_table* t, const sst_jaccard_args* a);
/* The skeleton's alphabet per spectrum (skeleton_building.py:319-326):
 * d_out[2g..2g+1] = d_alpha[2g..] & (the table's canonical rows | every row
 * either side's skeleton names at any of its max_len positions). */
int sst_skeleton_alpha_device(sst_table* t, int64_t n_spec, const int32_t* d_max_len, const uint64_t* d_skel_off,
                              const uint64_t* d_skel, const uint64_t* d_alpha, uint64_t* d_out);

/* After the skeleton (Predictor.predict, prediction.py:88-103), for the
 * spectra whose Jaccard length stands (status SST_JAC_OK; the others get
 * active 0 and no rows: predict returns Prediction.default()):
 * build_skeleton's fragments (skeleton_building.py:67-109) -- rows the START
 * walk kept (min_end - 1, max_end - 1), rows the END walk kept that START did
 * not (len - min_end, len - max_end), the alive internal rows whose peak no kept
 * terminal row shares (0, -1), every end index outside [0, len) clamped to
 * len - 1 -- in alive_out / min_end_out / max_end_out per row slot, and the
 * alphabet _reduce_alphabet sets (:99-103): alpha (the Jaccard stage's, as
 * sst_skeleton_alpha_device gives it) without the modifications the combined
 * skeleton's positions 0 .. seq_len - 1 do not name.  The caller applies the
 * reduction's is_valid filter with sst_valid_rows_alpha_device(alpha_out,
 * active, alive_out).  kept / min_end / max_end are sst_walk_args' [2][slots]
 * arrays (side-major).  err bit 0: a spectrum of more than 4096 peaks. */
typedef struct sst_post_args {
  int64_t n_spec;
  const int64_t* peak_off;   /* [n_spec + 1] */
  const uint32_t* rows;      /* [n_spec] */
  const uint32_t* meta;      /* row slots, as sst_classify_rows_device writes them */
  const uint8_t* alive;      /* the fixpoint's survivors */
  const uint8_t* kept;       /* [2][slots] */
  const int32_t* min_end;    /* [2][slots] */
  const int32_t* max_end;
  int64_t slots;
  const int32_t* seq_len;    /* [n_spec] sst_jaccard_device's */
  const int8_t* jac_status;  /* [n_spec] */
  const uint64_t* comb_off;  /* [n_spec] */
  const uint64_t* comb;
  const uint64_t* alpha;     /* [2 n_spec] the Jaccard stage's alphabets */
  uint64_t* alpha_out;       /* [2 n_spec] */
  uint8_t* active;           /* [n_spec] */
  uint8_t* alive_out;        /* row slots */
  int32_t* min_end_out;
  int32_t* max_end_out;
  uint32_t* err;
} sst_post_args;
int sst_post_skeleton_device(sst_table* t, const sst_post_args* a);

/* The dense per-spectrum hand-off to the MILP stages: what Predictor.predict
 * holds after the skeleton-based reduction (prediction.py:88-103 -- the
 * fragments build_skeleton returned, skeleton_building.py:67-109, that pass
 * the reduced alphabet's is_valid filter, with min_end / max_end; the
 * combined skeleton's seq_len positions), compacted so that one download per
 * array delivers it.  Count, then emit, as sst_bins_count_device /
 * sst_bins_emit_device:
 * sst_handoff_count_device: n_frag[g] = the row slots of spectrum g with a
 * non-zero flags byte among its cnt[g] rows from slot 4 * peak_off[g],
 * n_pos[g] = seq_len[g]; both 0 where active[g] == 0; then their exclusive
 * prefixes frag_off / pos_off (n_spec + 1 entries each, totals last).
 * sst_handoff_emit_device (after the caller sized the outputs from the
 * totals): the flagged rows of spectrum g in ascending row order from
 * frag_off[g] -- index (the row's place among the spectrum's rows: the
 * reference's SU-order `index`, prediction.py:68-72), code (meta & 0x1f:
 * breakage code, side bits << 2, singleton << 4), su, obs, out_min_end,
 * out_max_end -- and the first seq_len[g] position masks (two u64 each) of
 * comb + 2 comb_off[g] at skeleton + 2 pos_off[g].  flags / min_end / max_end
 * are row-slot arrays (sst_post_args' alive_out / min_end_out / max_end_out).
 * Device pointers, the ctx's stream. */
typedef struct sst_handoff_args {
  int64_t n_spec;
  const int64_t* peak_off;   /* [n_spec + 1] */
  const uint32_t* cnt;       /* [n_spec] rows per spectrum */
  const double* r_su;        /* row slots, as sst_classify_rows_device writes them */
  const double* r_ob;
  const uint32_t* r_meta;
  const uint8_t* flags;      /* row slots: the rows to hand off */
  const int32_t* min_end;    /* row slots */
  const int32_t* max_end;
  const uint8_t* active;     /* [n_spec] */
  const int32_t* seq_len;    /* [n_spec] */
  const uint64_t* comb_off;  /* [n_spec] as sst_jaccard_args.comb_off */
  const uint64_t* comb;
  uint32_t* n_frag;          /* [n_spec] count pass */
  uint32_t* n_pos;
  uint64_t* frag_off;        /* [n_spec + 1] count pass writes, emit pass reads */
  uint64_t* pos_off;
  int32_t* index;            /* [frag_off[n_spec]] emit pass (may be NULL for the count pass) */
  uint8_t* code;
  double* su;
  double* obs;
  int32_t* out_min_end;
  int32_t* out_max_end;
  uint64_t* skeleton;        /* [2 pos_off[n_spec]] */
} sst_handoff_args;
int sst_handoff_count_device(sst_table* t, const sst_handoff_args* a);
int sst_handoff_emit_device(sst_table* t, const sst_handoff_args* a);

/* The alignment certificate: which handed-off fragments no window of the
 * skeleton can explain.  filter_with_lp (prediction.py:229-259) builds and
 * solves one LinearProgramInstance per fragment only to ask whether the
 * fragment can sit on a contiguous run of skeleton positions with a mass error
 * <= tolerance * observed_mass.  A necessary condition is decided here without
 * a solver; the inputs are the hand-off's dense arrays.
 * Per spectrum g: L = seq_len[g]; position masks P_0 .. P_{L-1} (two u64 over
 * table rows, skeleton + 2 pos_off[g]); alphabet mask alpha + 2 g; integer row
 * masses w_r (the table's, all >= 0); fragments frag_off[g] .. frag_off[g + 1].
 * Position sets (linear_program.py:109-134): A_i = P_i & alpha if P_i != 0,
 *   else alpha; row 0 and rows the table does not have are excluded.  If any
 *   A_i is empty the program has no feasible y: every fragment of the
 *   spectrum gets SST_ALIGN_INFEASIBLE.
 * Window of a fragment: target = rint(su / prec) (ties to even), W =
 *   ceil(tol * obs / prec); an integer sum s fits iff |s - target| <= W
 *   (W < 0: nothing fits).  su and obs are finite (values beyond +-2^61 after
 *   the division are clamped there).
 * Admissible intervals: the contiguous sets of positions with x = 1 under the
 *   fixings of _set_x (linear_program.py:74-102; later fixings override
 *   earlier ones) and the contiguity constraints (:206-217), selected by the
 *   side bits of frag_code (START = bit 2, END = bit 3), mn = frag_min_end,
 *   mx = frag_max_end:
 *     START and END ("START_END")  [0, L-1] only (the empty interval if L == 0)
 *     START only                   [0, r] for r in [min(mn, mx), mx]
 *     END only                     [l, L-1] for l in [min(mx, mn), mn]
 *     neither (internal)           every [l, r], 0 <= l <= r < L, and the
 *                                  empty interval
 *   The empty interval has sum 0, is written (l, r) = (0xFF, 0xFF), and is
 *   counted and reported like any other; it fits iff |target| <= W.
 *   A START-only or END-only fragment with mn or mx outside [0, L-1] is not
 *   modelled: SST_ALIGN_SKIPPED.  So is every fragment of a spectrum with
 *   L < 0, L > 253 (sums fit u32 and (l, r) two bytes up to there) or
 *   pos_off[g + 1] - pos_off[g] != L; an empty A_i takes precedence only
 *   among modelled spectra.
 * Achievable sums: S(l, r) = { one w_a per position i in [l, r], a in A_i,
 *   summed }, LO(l, r) / HI(l, r) the sums of the positions' minima / maxima.
 * Capacity K = sst_align_capacity() (a build constant >= 1024): [l, r] is
 *   closed if |S(l, r)| <= K, else open.  |S| never shrinks when an interval
 *   grows, so this does not depend on the sweep direction.
 * Outputs per fragment:
 *   status    SST_ALIGN_NONE: no admissible interval has [target - W,
 *             target + W] meeting [LO, HI], or every one that does is closed
 *             and holds no fitting sum; SST_ALIGN_FIT: a closed admissible
 *             interval holds a fitting sum; SST_ALIGN_OPEN: no closed fit, but
 *             an open admissible interval's [LO, HI] meets the window
 *             (undecided); SST_ALIGN_INFEASIBLE, SST_ALIGN_SKIPPED as above.
 *   alignable 1 for FIT, OPEN, SKIPPED; 0 for NONE, INFEASIBLE.
 *   n_fit     closed admissible intervals that hold a fitting sum (at most
 *             253 * 254 / 2 + 1, so the saturating count never saturates).
 *   first     l << 8 | r of the smallest such (l, r) in (l, r) order (the
 *             empty interval last, 0xFFFF); 0xFFFE when n_fit == 0.
 * alignable == 0 is safe: dropping the modification-rate constraints
 * (linear_program.py:180-196) only enlarges the feasible set, and if no
 * achievable s has |s - target| <= W then every s has |su / prec - s| >=
 * W + 1 - 0.5 >= tol * obs / prec + 0.5, so the true error exceeds the
 * threshold by >= prec / 2, far above the float sums' and a solver's
 * tolerances; an incumbent is feasible, hence >= the optimum (None becomes
 * inf, :236), so minimize_error > tol * obs and filter_with_lp removes the
 * fragment.  This equivalence is proven, not run: no solver is part of this
 * project's tests.  alignable == 1 promises nothing.
 * One kernel (k_align_windows, sst_align.hip) queued on the ctx stream; device
 * pointers; no scratch buffer beyond the outputs.  Fragments of a spectrum in
 * ascending su order (as the hand-off emits them) run fastest; any order is
 * answered exactly.  SST_E_ARG: a NULL array with n_spec > 0, n_spec < 0, a
 * non-positive or non-finite prec, a non-finite tol, a table of more than
 * SST_MAX_ROWS rows or with a row mass < 0 or >= 2^32 / 253. */
#define SST_ALIGN_CAPACITY 1024u
#define SST_ALIGN_NONE 0
#define SST_ALIGN_FIT 1
#define SST_ALIGN_OPEN 2
#define SST_ALIGN_INFEASIBLE 3
#define SST_ALIGN_SKIPPED 4
typedef struct sst_align_args {
  int64_t n_spec;
  const int32_t* seq_len;       /* [n_spec] */
  const int64_t* pos_off;       /* [n_spec + 1] */
  const uint64_t* skeleton;     /* [2 pos_off[n_spec]] */
  const uint64_t* alpha;        /* [2 n_spec] */
  const int64_t* frag_off;      /* [n_spec + 1] */
  const uint8_t* frag_code;     /* [frag_off[n_spec]] each, as sst_handoff_emit_device's code */
  const double* frag_su;
  const double* frag_obs;
  const int32_t* frag_min_end;
  const int32_t* frag_max_end;
  double tol, prec;
  uint8_t* status;              /* outputs, [frag_off[n_spec]] each */
  uint8_t* alignable;
  uint32_t* n_fit;
  uint16_t* first;
} sst_align_args;
uint32_t sst_align_capacity(void);
int sst_align_windows_device(sst_table* t, const sst_align_args* a);

/* The two-list split of the certificate's open intervals (an exact
 * meet-in-the-middle).  Everything of sst_align_windows_device's definition
 * stays; for an open interval [l, r]:
 *   [l, r] is split-closed iff there is an m in [l, r - 1] with S(l, m) and
 *   S(m + 1, r) both closed.  |S| never shrinks when an interval grows, so
 *   this holds iff it holds for the greedy split from the left (m* the largest
 *   m with S(l, m) closed) and iff it holds for the greedy split from the
 *   right: it does not depend on the sweep direction.
 *   A split-closed interval holds a fitting sum iff some a in S(l, m) and b in
 *   S(m + 1, r) have |a + b - target| <= W (exact for any valid m, since
 *   S(l, r) = S(l, m) + S(m + 1, r)).
 *   An interval that is neither closed nor split-closed is undecided.
 * Precondition: a's four output arrays hold the result of
 * sst_align_windows_device for the same a.  Only fragments whose status there
 * is SST_ALIGN_OPEN are recomputed:
 *   status    SST_ALIGN_FIT if a split-closed admissible interval holds a
 *             fitting sum; else SST_ALIGN_OPEN if an undecided admissible
 *             interval has [LO, HI] meeting [target - W, target + W]; else
 *             SST_ALIGN_NONE.
 *   n_fit     the split-closed admissible intervals that hold a fitting sum
 *             (the fragment's closed intervals hold none, or it would not have
 *             been OPEN).
 *   first     l << 8 | r of the smallest of them, else 0xFFFE.
 *   alignable 0 for NONE, else 1.
 * Every other fragment keeps all four outputs bit for bit; in particular the
 * n_fit of a fragment that was FIT before still counts closed intervals only.
 * The call is idempotent on its own output.  A split NONE is as safe as a
 * base NONE: no achievable sum of any admissible interval fits, and that was
 * enumerated exactly.
 * One kernel (k_align_split, sst_align.hip) queued on the ctx stream, so it
 * follows sst_align_windows_device without a host round trip; spectra without
 * an OPEN fragment cost one read of their status bytes; no scratch buffer, no
 * global atomics.  Argument checks and errors as sst_align_windows_device. */
int sst_align_split_device(sst_table* t, const sst_align_args* a);

/* The certificate under the program's universal modification cap
 * (linear_program.py:180-188: the y of rows whose name is not in
 * UNMODIFIED_BASES sum to at most ceil(modification_rate * L)).  Everything of
 * sst_align_windows_device's definition stays, except:
 *   row_mod[r]  one byte per table row: 1 iff the row's first name (the name
 *     the program's y variable carries) is not in UNMODIFIED_BASES.  This is
 *     not the table's is_modification ("any name").
 *   mod_cap[g]  int(ceil(modification_rate * L)) of spectrum g, computed by the
 *     caller in f64 as the reference does; the kernels see integers only.
 *   Position i is forced iff every row of A_i is modified; F is the number of
 *   forced positions of the spectrum.  If F > mod_cap[g] (so also for a
 *   negative mod_cap) no y is feasible: every fragment of the spectrum gets
 *   SST_ALIGN_INFEASIBLE, with the precedence of an empty A_i (among modelled
 *   spectra only).  Else the budget is E = mod_cap[g] - F >= 0.
 *   Capped sums: S_E(l, r) = the sums of one w_a per position i in [l, r], a in
 *   A_i, for which some choice has excess <= E, the excess of a choice being
 *   (modified rows chosen) - (forced positions in [l, r]).  Positions outside
 *   [l, r] cost at least their forced count and can be chosen to cost exactly
 *   that, so S_E(l, r) is exactly what the y that satisfy the cap over the
 *   whole sequence can place on [l, r].  Per distinct sum the smallest excess
 *   is kept; extending by position p maps (s, e) to (s + w_a, e + row_mod[a] -
 *   forced_p), a in A_p; excess never falls along a sweep, so an entry above E
 *   leaves for good.  The empty interval has sum 0 and excess 0.
 *   [l, r] is closed iff |S_E(l, r)| <= K.  Every position has a row of cost
 *   0, so |S_E| never shrinks when an interval grows at either end, and the
 *   set does not depend on the sweep direction.  LO / HI stay the uncapped sums
 *   of minima / maxima: a conservative cut only (the meets test of open
 *   intervals, the early exit); they need not be achievable under the cap.
 *   status, n_fit, first, alignable: as defined there, with S_E for S.
 * With row_mod all zero, or mod_cap[g] >= L, all four outputs equal
 * sst_align_windows_device's bit for bit.  alignable here <= alignable there;
 * an interval closed there is closed here; a FIT there may be NONE or OPEN
 * here, a NONE there stays NONE (or INFEASIBLE).
 * alignable == 0 stays safe by the argument above with "dropping the per-row
 * caps (linear_program.py:190-196)" for "dropping the modification-rate
 * constraints": those caps are not a function of one scalar per sum and stay
 * dropped, so the certificate remains a necessary condition and alignable == 1
 * still promises nothing.
 * One kernel (k_align_windows_caps, sst_align.hip: one u8 excess beside every
 * u32 list entry) on the ctx stream; no scratch buffer, no global atomics.
 * Both members of caps are device pointers.  Argument checks and errors as
 * sst_align_windows_device, plus SST_E_ARG for a NULL caps or, with n_spec >
 * 0, a NULL member (with a message). */
typedef struct sst_align_caps {
  const uint8_t* row_mod; /* [table rows] */
  const int32_t* mod_cap; /* [n_spec] */
} sst_align_caps;
int sst_align_windows_caps_device(sst_table* t, const sst_align_args* a, const sst_align_caps* caps);

/* The two-list split under the cap.  sst_align_split_device's definition with:
 *   m* the largest m with S_E(l, m) closed; the second list is S_E(m* + 1, r),
 *   its excess counted against its own forced positions; [l, r] is
 *   split-closed while both lists are closed (by monotonicity this is again
 *   the "exists m" rule and direction-free).  It holds a fitting sum iff some
 *   a, b of the two lists have |a + b - target| <= W and e_a + e_b <= E (excess
 *   adds over disjoint intervals).  Every b inside the window is tried, not
 *   only the first one >= target - W - a.
 * Precondition: a's four output arrays hold sst_align_windows_caps_device's
 * result for the same a and caps; only its SST_ALIGN_OPEN fragments are
 * recomputed, every other keeps all four outputs bit for bit, and the call is
 * idempotent on its own output.  One kernel (k_align_split_caps) on the ctx
 * stream.  Argument checks as sst_align_windows_caps_device. */
int sst_align_split_caps_device(sst_table* t, const sst_align_args* a, const sst_align_caps* caps);

/* Keep mode: the certificate's second side.  Everything of
 * sst_align_windows_caps_device's definition stays; status, alignable, n_fit
 * and first equal its outputs bit for bit.  Keep mode adds, per fragment, a
 * proof that the program HAS a feasible point within the threshold (KEEP), so
 * that the three answers are DROP (alignable == 0), KEEP (keep == 1) and
 * SOLVE (the rest).
 *   Inner window: with q = tol * obs / prec in f64 (the quotient W takes the
 *     ceiling of), W_in = floor(q) - 1 if q is finite and >= 1, else -1
 *     (nothing fits inside); clamped like W.  An integer sum s fits inside iff
 *     |s - target| <= W_in.  Since |su / prec - target| <= 0.5, a sum that fits
 *     inside has a true error <= (W_in + 0.5) prec <= tol * obs - prec / 2: the
 *     margin is half a precision unit, the mirror image of the DROP side's.
 *     W - W_in is 1 where q is an integer and 2 otherwise (q >= 1).
 *   Per-row caps (linear_program.py:190-196): row_cap[L * n_rows + r] =
 *     int(ceil(rate_r * L)) for L in [0, 253] and every table row r (n_rows the
 *     table's), rate_r the modification_rate of the row of the explanation
 *     masses that holds row r's first name; the caller computes it in f64 as
 *     the reference does, the kernels see integers only.  n_r is the number of
 *     positions i with r in A_i.  Row r of the spectrum's alphabet is free iff
 *     row_cap >= n_r, or row_mod[r] != 0 and row_cap >= mod_cap[g] (all
 *     modified rows together appear at most mod_cap times).  A spectrum is
 *     row-free iff every row of alpha except row 0 (and rows the table does
 *     not have) is free.  In a row-free spectrum every y within the universal
 *     cap is within every per-row cap, so S_E(l, r) is exactly the program's
 *     set of sums on [l, r].
 *   Outputs:
 *     keep        1 iff the spectrum is modelled, feasible and row-free, the
 *                 fragment is not SKIPPED, and some closed admissible interval's
 *                 S_E holds a sum that fits inside (the empty interval counts:
 *                 it fits inside iff |target| <= W_in); else 0.
 *     keep_first  l << 8 | r of the smallest such interval in (l, r) order (the
 *                 empty one last, 0xFFFF); 0xFFFE if there is none.
 *     spec_free   per spectrum: 1 iff it is modelled, feasible and row-free; 0
 *                 else, and 0 for a spectrum without fragments (nothing is
 *                 computed for it).
 *   keep == 1 implies status == SST_ALIGN_FIT.
 * What KEEP means: the program has a feasible point (y the choice behind the
 * sum, x the interval) with error <= tol * obs - prec / 2, so a solve that
 * runs to optimality returns a value within the threshold and filter_with_lp
 * keeps the fragment.  A solver stopped by its time limit may return a worse
 * incumbent, or none, and the reference then removes the fragment: KEEP equals
 * the reference under completed solves only, while DROP holds under every
 * outcome.  No solver runs in this project: the claim is proven and held to a
 * brute force over every y and x, not solved.  keep == 0 promises nothing.
 * One kernel (k_align_windows_keep: k_align_windows_caps with one more u32
 * per fragment record, W - W_in in the record's spare bits, and the row test
 * once per spectrum) on the ctx stream; no scratch buffer, no global atomics.
 * All four members of keep are device pointers.  Argument checks and errors as
 * sst_align_windows_caps_device, plus SST_E_ARG with a message for a NULL keep
 * or, with n_spec > 0, a NULL member. */
typedef struct sst_align_keep {
  const int32_t* row_cap; /* [254 * table rows] */
  uint8_t* keep;          /* outputs: [frag_off[n_spec]] */
  uint16_t* keep_first;   /*          [frag_off[n_spec]] */
  uint8_t* spec_free;     /*          [n_spec] */
} sst_align_keep;
int sst_align_windows_keep_device(sst_table* t, const sst_align_args* a, const sst_align_caps* caps,
                                  const sst_align_keep* keep);

/* The two-list split in keep mode: sst_align_split_caps_device's contract (a's
 * outputs and keep's hold sst_align_windows_keep_device's result for the same
 * arguments; only its SST_ALIGN_OPEN fragments are recomputed, every other
 * keeps all six outputs bit for bit; idempotent on its own output; spec_free is
 * read, not written).  For the recomputed fragments keep and keep_first come
 * from the split-closed intervals of a row-free spectrum: some a, b of the two
 * lists with |a + b - target| <= W_in and e_a + e_b <= E.  A fragment that was
 * FIT at base keeps its keep and keep_first even where an inner fit exists only
 * in an open interval: that incompleteness is documented, not fixed (keep == 0
 * promises nothing).  One kernel (k_align_split_keep) on the ctx stream. */
int sst_align_split_keep_device(sst_table* t, const sst_align_args* a, const sst_align_caps* caps,
                                const sst_align_keep* keep);

/* The final program: the optimal sequence by exact enumeration.  After
 * filter_with_lp, Predictor.predict builds one LinearProgramInstance over the
 * fragments that are left and reads the prediction from its solution
 * (prediction.py:158-166; linear_program.py:164-225 the program, :238-313
 * evaluate).  Here that program is enumerated, not solved.
 * Per spectrum everything is as sst_align_windows_keep_device defines it: L,
 * the position sets A_i (row 0 excluded), row_mod, mod_cap, row_cap, the
 * admissible intervals per fragment class, the row-free test.
 *   Used fragments: frag_use, one byte per fragment, NULL = all.  Only used
 *     fragments enter the program.
 *   Assignments: y takes one row of A_i per position.  y is feasible iff at
 *     most mod_cap[g] of its rows have row_mod == 1.  combos = prod |A_i|,
 *     saturating at UINT64_MAX; n_feas is the number of feasible y.  Order:
 *     the index of y in mixed radix, position 0 most significant, rows
 *     ascending within a position: index order is lexicographic order.
 *   Fixed-point mass: u = su / prec in f64, qfix = (int64) rint(u * 65536.0),
 *     ties to even.
 *   Cost: c_j(y) = min over the admissible (l, r) of |qfix_j - 65536 S_y(l, r)|,
 *     S_y the sum of w_{y_i} over [l, r] and 0 for the empty interval;
 *     obj(y) = sum of c_j(y) over the used fragments, as u64.
 *   Status per spectrum:
 *     SST_FINAL_NONE        no fragments (a default spectrum): nothing computed
 *     SST_FINAL_SKIPPED     not modelled: L outside [0, 253]; pos_off[g + 1] -
 *                           pos_off[g] != L; a used START-only or END-only
 *                           fragment with mn or mx outside [0, L - 1]; a used
 *                           fragment whose u is not finite or has |u| >= 2^32;
 *                           more than 16 384 used fragments (below these limits
 *                           every total stays below 2^63)
 *     SST_FINAL_INFEASIBLE  an empty A_i, or n_feas == 0
 *     SST_FINAL_NOT_FREE    not row-free: the per-row caps may bind, and they
 *                           are not enumerated
 *     SST_FINAL_TOO_LARGE   combos > max_combos (1 <= max_combos <=
 *                           SST_FINAL_MAX_COMBOS = sst_final_max_combos())
 *     SST_FINAL_SOLVED      the optimum was found
 *     Precedence: NONE, SKIPPED, an empty A_i, NOT_FREE, TOO_LARGE, n_feas == 0.
 *   Outputs per spectrum: status; combos (0 for NONE and SKIPPED); and, all 0
 *     (gap: UINT64_MAX) unless SOLVED: n_feas; best = min obj over the feasible
 *     y; n_opt, the feasible y with obj == best (u32, saturating); gap, the
 *     smallest obj above best minus best, UINT64_MAX if there is none.
 *   Per position (seq, [pos_off[n_spec]]): the row of the first optimal y in
 *     the order above; 0 unless SOLVED.
 *   Per fragment: iv, under that y the smallest l << 8 | r among the
 *     minimisers of c_j, the empty interval last as 0xFFFF; 0xFFFE for an
 *     unused fragment or a spectrum that is not SOLVED.  sum: that interval's
 *     S_y (0 where iv is 0xFFFE).
 *   Every output element is written on every call.
 * What SOLVED proves.  In a row-free spectrum the feasible y are exactly the
 * program's y (keep mode's argument).  For a fixed y the x_j are independent:
 * contiguity plus _set_x's fixings give exactly the admissible intervals.
 * |qfix / 65536 - su / prec| < 2^-16 per fragment (rint, and one f64 division
 * at |u| < 2^32), so obj / 65536 * prec is within n_used * 2^-16 * prec of the
 * real objective of y's best x.  Hence if n_opt == 1 and gap > 2 n_used, the
 * program's optimal y is unique in real arithmetic and is seq.  The claim holds
 * for a solve run to optimality; a time-limited solve may return anything.  iv
 * is AN optimal x: where two intervals tie, the reference's left / right and
 * the sign of predicted_diff are the solver's choice.  n_opt > 1 (rows of equal
 * mass, positions no fragment's best interval covers) is reported, not
 * resolved.  No solver runs in this project: the claim is proven and held to a
 * brute force, not solved.
 * One kernel (k_final_program, sst_final.hip: one spectrum per workgroup, lanes
 * over the indices of y) on the ctx stream; device pointers; no scratch buffer
 * beyond the outputs, no global atomics.  SST_E_ARG with a message for a NULL
 * struct or, with n_spec > 0, a NULL member (frag_use excepted); max_combos of
 * 0 or above the limit; a non-positive or non-finite prec; and the row-mass
 * limits of the align calls.  n_spec == 0 is SST_OK. */
#define SST_FINAL_MAX_COMBOS (1ull << 22)
#define SST_FINAL_NONE 0
#define SST_FINAL_SOLVED 1
#define SST_FINAL_TOO_LARGE 2
#define SST_FINAL_INFEASIBLE 3
#define SST_FINAL_SKIPPED 4
#define SST_FINAL_NOT_FREE 5
typedef struct sst_final_args {
  int64_t n_spec;
  const int32_t* seq_len;       /* [n_spec] */
  const int64_t* pos_off;       /* [n_spec + 1] */
  const uint64_t* skeleton;     /* [2 pos_off[n_spec]] */
  const uint64_t* alpha;        /* [2 n_spec] */
  const int64_t* frag_off;      /* [n_spec + 1] */
  const uint8_t* frag_code;     /* [frag_off[n_spec]] each */
  const double* frag_su;
  const int32_t* frag_min_end;
  const int32_t* frag_max_end;
  const uint8_t* frag_use;      /* NULL: every fragment is used */
  double prec;
  const uint8_t* row_mod;       /* [table rows] */
  const int32_t* mod_cap;       /* [n_spec] */
  const int32_t* row_cap;       /* [254 * table rows] */
  uint64_t max_combos;
  uint8_t* status;              /* outputs, [n_spec] each */
  uint64_t* combos;
  uint64_t* n_feas;
  uint64_t* best;
  uint32_t* n_opt;
  uint64_t* gap;
  uint8_t* seq;                 /* [pos_off[n_spec]] */
  uint16_t* iv;                 /* [frag_off[n_spec]] */
  uint32_t* sum;                /* [frag_off[n_spec]] */
} sst_final_args;
uint64_t sst_final_max_combos(void);
int sst_final_program_device(sst_table* t, const sst_final_args* a);

/* The robust final program: the optimal sequence whatever subset of the
 * optional fragments enters the program.  After filter_with_lp the final
 * program runs over the fragments keep mode proves kept (R, required) plus the
 * subset T the solver keeps of those it still has to decide (O, optional;
 * prediction.py:126-166); the fragment set enters the program nowhere else.
 * Everything not listed here is sst_final_program_device's definition.
 *   frag_use: 0 unused, 1 required, 2 optional; NULL = all required; any other
 *     value is treated as 1.
 *   SKIPPED: its conditions apply to required and optional fragments alike;
 *     the 16 384 limit counts both, so every total stays below 2^63.
 *   The nine outputs of base: what sst_final_program_device writes for
 *     frag_use' = (frag_use == 1), except that an optional fragment of a SOLVED
 *     spectrum has iv and sum, its interval and sum under seq by the rule for
 *     used fragments (smallest (l, r) among the minimisers, the empty one last).
 *   With y* the first optimal y over R (seq), c*_j = c_j(y*) and
 *     cap(y) = sum over R of c_j(y) + sum over O of min(c_j(y), c*_j),
 *   five more outputs per spectrum, all 0 and rgap UINT64_MAX unless SOLVED:
 *     n_optional (u32); cstar = sum over O of c*_j; rbest = min cap(y) over the
 *     feasible y; rn_opt, the feasible y with cap(y) == rbest (u32,
 *     saturating); rgap, the smallest cap above rbest minus rbest, UINT64_MAX
 *     if there is none.  Without optional fragments cap == obj: cstar = 0,
 *     rbest = best, rn_opt = n_opt, rgap = gap.
 *   No limit on the number of optional fragments and no further status.  Every
 *   output element is written on every call.
 * What it proves.  With obj_T(y) = sum over R + T of c_j(y), for any y
 *     min over T in O of [obj_T(y) - obj_T(y*)]
 *       = sum_R (c_j(y) - c*_j) + sum_O min(0, c_j(y) - c*_j) = cap(y) - cap(y*),
 *   and cap(y*) = best + cstar.  So y* is the unique minimiser of every obj_T
 *   with margin m iff it is the unique minimiser of cap with margin m.  The
 *   rounding argument of sst_final_program_device moves each objective by less
 *   than one unit per fragment in the sum.  Hence if rbest == best + cstar,
 *   rn_opt == 1 and rgap > 2 (n_used + n_optional), n_used the required
 *   fragments, then for every T the program over R + T has the unique optimum
 *   seq in real arithmetic (rn_opt == 1 with rbest == best + cstar already
 *   implies n_opt == 1).  The caveats stay: completed solves only, for the
 *   final solve and for the solves KEEP speaks about; iv is AN optimal x; no
 *   solver runs here.  The criterion is sufficient, not necessary: it
 *   quantifies over subsets a solver would never return.
 * One kernel (k_final_robust, sst_final.hip: k_final_program's body with a
 * second enumeration where a spectrum holds optional fragments) on the ctx
 * stream; no scratch buffer, no global atomics.  Errors as
 * sst_final_program_device; with n_spec > 0 the five pointers are non-NULL. */
typedef struct sst_final_robust_args {
  sst_final_args base;
  uint32_t* n_optional;         /* outputs, [n_spec] each */
  uint64_t* cstar;
  uint64_t* rbest;
  uint32_t* rn_opt;
  uint64_t* rgap;
} sst_final_robust_args;
int sst_final_robust_device(sst_table* t, const sst_final_robust_args* a);

/* The robust final program with the bounded search: spectra above max_combos
 * are searched, not given up.  Everything not listed here is
 * sst_final_robust_device's definition.
 *   Arguments: robust (sst_final_robust_args); horizon H <= 2^62; max_width in
 *     [1, SST_FINAL_SEARCH_MAX_WIDTH = sst_final_search_max_width()] (2^16: a
 *     workgroup's two frontiers take 112 bytes of workspace per node of width);
 *     three more outputs per spectrum: mode (u8), rounds (u32), nodes (u64).
 *     robust.base.max_combos may be 0 here and only here: every modelled
 *     spectrum is searched.  Otherwise it is within the existing limit.
 *   Which path.  Precedence NONE, SKIPPED, an empty A_i, NOT_FREE as before.
 *     Then a spectrum with combos <= max_combos is ENUMERATED: all fourteen
 *     arrays are what sst_final_robust_device writes, mode = 1, rounds = nodes
 *     = 0.  Otherwise it is SEARCHED, mode = 2 where SOLVED: more than
 *     SST_FINAL_SEARCH_MAX_FREE = 48 free positions (|A_i| > 1) give TOO_LARGE;
 *     then n_feas == 0 gives INFEASIBLE; a sweep that overflows (below) gives
 *     TOO_LARGE.  A spectrum that is not SOLVED has mode = rounds = nodes = 0
 *     and the unsolved defaults elsewhere.  combos is written as before.
 *   n_feas of a searched spectrum: the number of feasible y, saturating at
 *     UINT64_MAX, counted over the number of modified rows per position.
 *   Nodes.  The free positions in position order are f_0 < ... < f_{n-1}.  A
 *     node of depth d fixes one row at each of f_0 .. f_{d-1}.  It is
 *     live-feasible iff the modified rows at the one-row positions, plus those
 *     it fixed, plus one for every later free position all of whose rows are
 *     modified, is at most mod_cap.  Children in ascending row order.  A leaf
 *     (d = n) is a y; its index is the mixed-radix index of the definition.
 *   Bound.  For a node, wmin_i = wmax_i = the row's mass at a fixed or one-row
 *     position, the smallest and largest mass over A_i at an open one; Pmin,
 *     Pmax their prefix sums.  For an interval [l, r]: Smin = Pmin(r + 1) -
 *     Pmin(l), Smax likewise, d(l, r) = max(0, 65536 Smin - qfix_j, qfix_j -
 *     65536 Smax); the empty interval: |qfix_j|.  lb_j(node) = min of d over
 *     fragment j's admissible intervals; lb(node) = the sum over the required
 *     fragments (pass 1), plus min(lb_j, c*_j) over the optional ones (pass
 *     2).  Integers throughout.  lb(leaf) = obj(y) (cap(y) in pass 2); lb
 *     never decreases from a node to its child; lb(node) is at most the
 *     objective of every leaf below it.
 *   Sweep(T).  S_0 = {root}; S_{d+1} = the live-feasible children c of S_d
 *     with lb(c) <= T.  It OVERFLOWS iff some |S_d| > max_width.  Otherwise it
 *     returns the leaves S_n: the feasible y with objective <= T (with n = 0
 *     the root is the one leaf, whatever T).  Its node count: sum over d = 1 ..
 *     n of |S_d|.
 *   Pass 1 (required fragments).  T = max(H, 65536); run Sweep(T), and while it
 *     returns no leaf T = 4 T, saturating at 2^63 - 1 (objectives stay below
 *     2^63).  b = the smallest leaf objective; if b + H > T, one more
 *     Sweep(b + H).  best = b; n_opt = the leaves with objective b, saturating
 *     u32; seq = the one of them with the smallest index; gap = the smallest
 *     leaf objective in (b, b + H] minus b, or H + 1 if there is none: gap =
 *     min(true gap, H + 1), the only place a searched spectrum's outputs leave
 *     the robust program's definition.  iv, sum, c*_j, cstar from seq as before.
 *   Pass 2 (only where n_optional > 0): one Sweep(best + cstar + H) with the
 *     capped bound (y* is a leaf of it).  rbest = the smallest leaf cap; rn_opt
 *     = the leaves at rbest; rgap = the smallest leaf cap in (rbest, rbest + H]
 *     minus rbest, or H + 1.  Without optional fragments the three copy best,
 *     n_opt, gap.
 *   rounds = the sweeps run in both passes, nodes = the sum of their counts; an
 *     overflow in either pass makes the spectrum TOO_LARGE.  Every output is a
 *     function of the inputs alone: S_d does not depend on an order of
 *     evaluation, so identical calls give identical arrays, nodes included.
 * Why the decisions stay sound.  A truncated gap never exceeds the true one, so
 * final_decisions / robust_decisions read it unchanged: they say TAKE only
 * where the true gap meets the need (at most 2 * 16 384 + 1 units or half a
 * precision unit, below H + 1 at H = 2^17).
 * Three launches on the ctx stream: k_final_robust (the enumerated spectra; the
 * others come out TOO_LARGE), k_final_search_list (one workgroup: the list of
 * those, and the three outputs' defaults), k_final_search (one workgroup per
 * listed spectrum, a level's frontier ping-ponged in the context's workspace:
 * cached across calls, freed by sst_ctx_trim).  Plain vector stores, no global
 * atomics.  Errors as sst_final_robust_device, and SST_E_ARG with a message for
 * max_width of 0 or above the limit, horizon > 2^62, a NULL mode / rounds /
 * nodes with n_spec > 0; SST_E_NOMEM where the workspace cannot be had. */
#define SST_FINAL_SEARCH_MAX_WIDTH (1u << 16)
#define SST_FINAL_SEARCH_MAX_FREE 48
typedef struct sst_final_search_args {
  sst_final_robust_args robust;
  uint64_t horizon;
  uint32_t max_width;
  uint8_t* mode;                /* outputs, [n_spec] each */
  uint32_t* rounds;
  uint64_t* nodes;
} sst_final_search_args;
uint32_t sst_final_search_max_width(void);
int sst_final_search_device(sst_table* t, const sst_final_search_args* a);

/* The length program: the optimum of the program determine_lp_score builds, per
 * candidate sequence length.  SkeletonBuilder.build_skeleton chooses the length
 * with select_sequence_length_with_lp first (skeleton_building.py:198-289): for
 * every c in [lower, upper] it combines the two skeletons at c, builds one
 * LinearProgramInstance over the terminal fragments and reads only the optimal
 * objective value (minimize_error, linear_program.py:227-236); the smallest
 * value among the lengths validate_sequence_length_by_mass accepts wins, and a
 * result below 1 hands the choice to the Jaccard selection (:44-57).  Here that
 * value is enumerated, not solved.
 * Per spectrum g (what build_skeleton holds at :45): M = max_len[g], the walk's
 *   length; the START skeleton S_0 .. S_{M-1} and the REVERSED END skeleton
 *   E_0 .. E_{M-1} (:41), two u64 over table rows each, at skeleton +
 *   2 skel_off[g] and skeleton + 2 (skel_off[g] + M); the skeleton alphabet
 *   alpha + 2 g; the terminal fragments frag_off[g] .. frag_off[g + 1]: the START
 *   walk's kept rows, then the END walk's kept rows whose index no START row has
 *   (:262-264; this does not depend on c), each with frag_code (side bits as
 *   everywhere: START = bit 2, END = bit 3), su, and the walk's RAW min_end /
 *   max_end.  Its candidates cand_off[g] .. cand_off[g + 1], each with its length
 *   cand_len[k] = c (the caller lists lower .. upper, or nothing where the bounds
 *   raised), valid[k] and mod_cap[k].
 * Candidate c, n = max(c, 0) the number of positions of its program:
 *   Combined skeleton (:494-516): position i takes S_i & E_{M-c+i} if that is
 *     non-zero, else S_i | E_{M-c+i}.  A_i from it as sst_align_windows_device
 *     defines the position sets (alpha where the position is empty, row 0
 *     excluded).  mod_cap[k] = int(ceil(modification_rate * c)), row caps
 *     row_cap[c * n_rows + r], row_mod: all as keep mode's inputs, computed by the
 *     caller.  The row-free test is keep mode's, at length c.
 *   Ends (:267-276, no clamping): a START row has mn = min_end - 1, mx =
 *     max_end - 1; an END row mn = n - min_end, mx = n - max_end.
 *   Shape: the contiguous runs of positions, the empty one included, that agree
 *     with what _set_x leaves (linear_program.py:74-102; later fixings override
 *     earlier ones, Python's negative indices wrap, an index outside [-n, n - 1]
 *     raises and determine_lp_score returns inf, :279-286):
 *       START and END ("START_END")  WHOLE, [0, n - 1]
 *       START only  RAISES iff mn >= n or mx + 1 < -n.  Else, if mx + 1 <= 0:
 *                   EMPTY (every x is 0; the empty interval only).  Else, if
 *                   mn < 0: not modelled (no x is fixed to 1).  Else PREFIX
 *                   [0, e], e in [min(mn, mx), min(mx, n - 1)].
 *       END only    RAISES iff mx > n or mn < -n.  Else, if mn < 0: WHOLE (the
 *                   wrapped range fixes every x to 1).  Else, if mn >= n: EMPTY
 *                   if mx == n, otherwise not modelled.  Else SUFFIX [s, n - 1],
 *                   s in [max(0, min(mx, mn)), mn].
 *       neither     not modelled (no terminal fragment).
 *     Inside [0, n - 1] this is sst_align_windows_device's rule.
 *   Cost and objective: the final program's.  qfix_j = rint(su_j / prec *
 *     65536) (ties to even; |su_j / prec| < 2^32, at most 16 384 fragments),
 *     c_j(y) = min over the fragment's shape of |qfix_j - 65536 S_y(l, r)| (the
 *     empty interval: |qfix_j|), obj(y) = the sum over ALL terminal fragments, y
 *     feasible iff at most mod_cap[k] of its rows are modified; combos, n_feas as
 *     there.
 *   Status (u8), in precedence order:
 *     SST_LEN_INVALID       valid[k] == 0: validate_sequence_length_by_mass
 *                           (:291-313) rejects c, so c is never chosen and never
 *                           updates best_val (:244-250).  Nothing is computed.
 *                           valid is the caller's: the f64 sums in the
 *                           reference's order.
 *     SST_LEN_RAISES        some fragment raises: the value is exactly +inf
 *     SST_LEN_NOT_MODELLED  c < 1, c > 253 or c > M (combine_skeleton_sequences
 *                           raises there); no terminal fragment (what the solver
 *                           layer returns for an empty objective is not pinned
 *                           here); more than 16 384 fragments or one outside the
 *                           fixed-point limits; a shape that is not modelled
 *     SST_LEN_INFEASIBLE    an empty A_i, or n_feas == 0.  The reference reads
 *                           objective.value() without looking at the solve
 *                           status: the value is the solver's and is not claimed.
 *     SST_LEN_NOT_FREE      not row-free: the per-row caps may bind
 *     SST_LEN_TOO_LARGE     combos > max_combos (1 <= max_combos <=
 *                           SST_FINAL_MAX_COMBOS)
 *     SST_LEN_SOLVED        best = min obj over the feasible y
 *   Outputs per candidate: status; combos (0 unless the status is INFEASIBLE,
 *     NOT_FREE, TOO_LARGE or SOLVED; 0 for an empty A_i); n_feas and best (0
 *     unless SOLVED).  Every element is written on every call.
 * What SOLVED proves: as sst_final_program_device's "What SOLVED proves", points
 * one to three -- in a row-free candidate the feasible y are the program's; for a
 * fixed y the x_j are independent and take exactly the shape's intervals; best /
 * 65536 * prec is within n_frag * 2^-16 * prec of the program's real optimum.  So
 * two SOLVED candidates whose best differ by more than 2 n_frag units are ordered
 * as their real optima are.  The claim is for solves run to optimality
 * (timeLimit(short) may cut one off); no solver runs in this project: the claim
 * is proven and held to a brute force.
 * One kernel (k_length_program, sst_length_program.hip: one candidate per
 * workgroup, lanes over the indices of y) on the ctx stream; device pointers; no
 * scratch buffer beyond the outputs, no global atomics.  SST_E_ARG with a message
 * for a NULL struct or, with n_spec > 0, a NULL member; n_spec or n_cand < 0;
 * max_combos of 0 or above the limit; a non-positive or non-finite prec; and the
 * row-mass limits of the align calls.  n_spec == 0 is SST_OK, and so is n_cand
 * == 0 (nothing is written). */
#define SST_LEN_INVALID 0
#define SST_LEN_RAISES 1
#define SST_LEN_NOT_MODELLED 2
#define SST_LEN_INFEASIBLE 3
#define SST_LEN_NOT_FREE 4
#define SST_LEN_TOO_LARGE 5
#define SST_LEN_SOLVED 6
typedef struct sst_length_program_args {
  int64_t n_spec;
  int64_t n_cand;               /* cand_off[n_spec] */
  const int32_t* max_len;       /* [n_spec] M */
  const int64_t* skel_off;      /* [n_spec + 1] in positions: spectrum g holds 2 M */
  const uint64_t* skeleton;     /* [2 skel_off[n_spec]] two u64 per position */
  const uint64_t* alpha;        /* [2 n_spec] */
  const int64_t* frag_off;      /* [n_spec + 1] */
  const uint8_t* frag_code;     /* [frag_off[n_spec]] each */
  const double* frag_su;
  const int32_t* frag_min_end;  /* the walk's raw ends */
  const int32_t* frag_max_end;
  const int64_t* cand_off;      /* [n_spec + 1] */
  const int32_t* cand_len;      /* [n_cand] each */
  const uint8_t* valid;
  const int32_t* mod_cap;
  double prec;
  const uint8_t* row_mod;       /* [table rows] */
  const int32_t* row_cap;       /* [254 * table rows] */
  uint64_t max_combos;
  uint8_t* status;              /* outputs, [n_cand] each */
  uint64_t* combos;
  uint64_t* n_feas;
  uint64_t* best;
} sst_length_program_args;
int sst_length_program_device(sst_table* t, const sst_length_program_args* a);

/* compute_sequence_length_bound (mass_table.py:343-487) after the skeleton's
 * alphabet reduction (skeleton_building.py:315-336), both directions, for
 * queries on per-spectrum reduced alphabets, exact without a table rebuild:
 * sst_reach_rows_device writes, per spectrum g, the reachability bitset of
 * each kept row k (row 0 excluded, ascending): bit m of u32 word
 * d_bits[d_off[g] + k * d_words[g] + m / 32] <=> m is a sum of kept rows up
 * to that one (the rebuilt table's pair(r_k, m) != 0), for m < 32 d_words[g]
 * (>= the highest window value + 1).  sst_length_bounds_reach_device then
 * replays the reference's memoised DFS once per query (sst_length_queries)
 * on those pairs and derives both bounds from it.  soft_nodes > 0: a query
 * whose replay passes that many nodes stops with status SST_LB_HEAVY (the
 * caller replays such queries together later, with soft_nodes 0), so that a
 * few heavy spectra do not hold up a batch.  memo_first: the first attempt's
 * memo masses per query (0: 2^16; a power of two).  fuse: both bounds'
 * values computed inside the replay, in dense per-mass slots (allowed when
 * every alphabet has <= 64 kept rows; 0: the separate value passes).
 * Device pointers. */
#define SST_MAX_ROWS 120
#define SST_LB_HEAVY (-7)
/* The queries of both length-bound engines: query i is the window of su[i],
 * obs[i] on the alphabet of spectrum spec[i].  Budgets: max_len, max_mods and
 * the table's caps (sst_table_set_budgets) as in sst_length_bound_batch -- or,
 * with qlen non-NULL, per query: max_len qlen[i], caps caps_len[qlen[i] *
 * SST_MAX_ROWS + r] and max_mods a0_len[qlen[i]] (the caller's round(L *
 * rate)), so spectra of every max_len share one launch (the table's
 * is_modification flags still come from sst_table_set_budgets). */
typedef struct sst_length_queries {
  const double* su;        /* [n] */
  const double* obs;       /* [n] */
  const int32_t* spec;     /* [n] */
  const uint64_t* alpha;   /* [2 n_spec] row masks */
  int64_t n;
  double tol, prec;
  int max_len;
  int64_t max_mods;
  int64_t* lower;          /* [n] out: the bounds */
  int64_t* upper;
  int8_t* status;          /* [n] out: 0 ok, SST_OUT_OF_TABLE (the reference raises), SST_ABORTED (a window in the
                              reduced table's masked last word, or a guard), SST_LB_EMPTY_WINDOW */
  const int32_t* qlen;     /* [n] or NULL */
  const int32_t* caps_len; /* required with qlen */
  const int32_t* a0_len;   /* required with qlen */
  uint64_t* nodes;         /* may be NULL; zeroed by the caller: per query, the replay's visited nodes summed
                              over its attempts, or the memo entries the frontier creates */
} sst_length_queries;
int sst_reach_rows_device(sst_table* t, const uint64_t* d_alpha, const int64_t* d_words, const uint64_t* d_off,
                          int64_t n_spec, uint32_t* d_bits);
int sst_length_bounds_reach_device(sst_table* t, const sst_length_queries* q, const uint32_t* d_reach_bits,
                                   const uint64_t* d_reach_off, const int64_t* d_reach_words, int64_t soft_nodes,
                                   uint32_t memo_first, int fuse);

/* The same bounds WITHOUT replaying the DFS (sst_frontier.hip, DESIGN §3
 * "first-visit frontier"): the reference's memo is keyed by (mass, row) and
 * ignores the budgets, so each node's memoised value is fixed by its first
 * visit; which visit comes first is the lexicographic minimum over the node's
 * up and left parents (mass_table.py:373-457: up before left, window values
 * ascending), computed in bands of the lightest row mass over descending
 * masses, then the values by a DP over ascending masses.  Same result as the
 * replay for every query, in time linear in the memo's size and independent of
 * any one spectrum's depth.
 * sst_reach_lowest_device first turns sst_reach_rows_device's bitsets into one
 * byte per mass: d_lr[d_lr_off[g] + m] = the lowest kept rank k with m in
 * R_k (0xFF: none), m < 32 d_words[g] (d_lr_off[g] a multiple of 32).
 * sst_length_bounds_frontier_device: the same queries (d_lr / d_lr_off instead
 * of the bitsets); q->nodes = per query, the memo entries (distinct (mass, row)
 * nodes) its DFS creates.  workspace_bytes: the device workspace (0: half the free memory, at
 * most 48 GB); queries are processed in chunks sized from the memo entries
 * per query seen so far (a chunk that overflows is split; a single query
 * beyond the workspace gets SST_ABORTED).
 * stats may be NULL. */
typedef struct sst_lbf_stats {
  int64_t live;            /* queries the list pass handed to the frontier */
  int64_t nodes;           /* memo entries created */
  int64_t chunks;          /* chunks run to completion */
  int64_t splits;          /* chunks that overflowed the workspace and were split */
  int64_t aborted;         /* single queries beyond the workspace (SST_ABORTED) */
  int64_t bands;           /* mass bands of the largest chunk */
  int64_t key_words;       /* 64-bit words per first-visit key (1, 2 or 4) */
  int64_t max_band_groups; /* (query, mass) groups of the fullest band */
  int64_t max_band_nodes;  /* memo entries of the fullest band */
  int64_t table_slots;     /* slots per hash table of the ring */
  int64_t node_cap;        /* node capacity per chunk */
  int64_t overflow_bits;   /* why chunks were split: 1 nodes / a band's records, 2 a hash table, 4 a band list */
  int64_t groups;          /* (query, mass) groups of the completed chunks (the memo's distinct masses) */
  int64_t edges;           /* left moves onto a mass > 0 of the completed chunks (candidate inserts) */
} sst_lbf_stats;
int sst_reach_lowest_device(sst_table* t, const uint64_t* d_alpha, const int64_t* d_words, const uint64_t* d_off,
                            int64_t n_spec, const uint32_t* d_bits, const uint64_t* d_lr_off, uint8_t* d_lr);
int sst_length_bounds_frontier_device(sst_table* t, const sst_length_queries* q, const uint8_t* d_lr,
                                      const uint64_t* d_lr_off, uint64_t workspace_bytes, sst_lbf_stats* stats);

/* ---- CPython set order (the skeleton walk's emulation, sst_pyset.h) ---- */
/* hash(tuple) of a tuple whose items hash to item_hashes[0..n) (CPython
 * 3.8+ tuplehash, 64-bit): the hash of an explanation's name tuple
 * (mass_explanation.py:302-318) from the names' str hashes. */
int64_t sst_py_tuple_hash(const int64_t* item_hashes, int64_t n);
/* The iteration order of a set built by adding elements keys[0..n) (distinct
 * keys = distinct elements, hashes[i] = hash(element i)) in that order to an
 * empty set (CPython 3.7-3.12 setobject.c): order[0..m) receives the keys in
 * iteration order; returns m (the distinct elements) or SST_E*.  Host code:
 * it exists so that tests can pin the walk's emulation to the interpreter. */
int64_t sst_pyset_order(const int32_t* keys, const int64_t* hashes, int64_t n, int32_t* order);

/* ---- measurement ------------------------------------------------------ */
/* Kernel ids for sst_profile_read. */
#define SST_K_IS_VALID 0
#define SST_K_EXPLAIN_MAIN 1
#define SST_K_EXPLAIN_DEFERRED 2 /* deep, no-memo and exact roles share one launch */
#define SST_K_EXPLAIN_DEEP SST_K_EXPLAIN_DEFERRED
#define SST_K_EXPLAIN_NOMEMO 3 /* reserved (merged into SST_K_EXPLAIN_DEFERRED) */
#define SST_K_EXPLAIN_EXACT 4  /* reserved (merged into SST_K_EXPLAIN_DEFERRED) */
#define SST_K_EXPLAIN_EXPAND 5
#define SST_K_RESULT_PACK 6 /* k_result_pack: dense hit list + payload of a pass */
/* config 5 (the device-resident pipeline stages) */
#define SST_K_CLASSIFY_ROWS 7 /* k_classify_rows (sst_classify_rows_device) */
#define SST_K_FIX_ROUND 8     /* k_fix_round (sst_fix_round_device) */
#define SST_K_VALID_ALPHA 9   /* k_valid_alpha (sst_valid_rows_alpha_device, sst_is_valid_alpha*) */
#define SST_K_BINS_COUNT 10   /* k_bins_count + k_scan_u32 (sst_bins_count_device) */
#define SST_K_BINS_EMIT 11    /* k_bins_emit (sst_bins_emit_device) */
#define SST_K_DICT 12         /* k_dict_count / k_dict_build (sst_dict_final_device) */
#define SST_K_SKEL_WALK 13    /* k_skel_walk (sst_skeleton_walk_device) */
#define SST_K_REACH_ROWS 14   /* k_reach_rows (sst_reach_rows_device) */
#define SST_K_LENGTH_BOUND 15 /* k_length_fast / k_length_exact (length-bound batches) */
#define SST_K_JACCARD 16      /* k_jaccard (sst_jaccard_device) */
#define SST_K_PAIRS_ALPHA 17  /* k_pairs_alpha (sst_explain_pairs_alpha*) */
#define SST_K_REQUERY_MERGE 18 /* k_requery_count + k_scan_u32 + k_requery_copy (sst_requery_merge_device) */
#define SST_K_HANDOFF 19 /* k_handoff_count + k_scan_u32, k_handoff_emit (sst_handoff_*_device) */
#define SST_K_TABLE_CERTIFY 20 /* k_table_certify (sst_table_certify) */
#define SST_K_ALIGN 21 /* k_align_windows (sst_align_windows_device) */
#define SST_K_ALIGN_SPLIT 22 /* k_align_split (sst_align_split_device) */
#define SST_K_ALIGN_CAPS 23 /* k_align_windows_caps (sst_align_windows_caps_device) */
#define SST_K_ALIGN_SPLIT_CAPS 24 /* k_align_split_caps (sst_align_split_caps_device) */
#define SST_K_ALIGN_KEEP 25 /* k_align_windows_keep (sst_align_windows_keep_device) */
#define SST_K_ALIGN_SPLIT_KEEP 26 /* k_align_split_keep (sst_align_split_keep_device) */
#define SST_K_FINAL 27 /* k_final_program (sst_final_program_device) */
#define SST_K_FINAL_ROBUST 28 /* k_final_robust (sst_final_robust_device) */
#define SST_K_FINAL_SEARCH 29 /* k_final_search_list / k_final_search (sst_final_search_device) */
#define SST_K_LENGTH_PROGRAM 30 /* k_length_program (sst_length_program_device) */
#define SST_K_COUNT 31
/* When enabled, every kernel launch of this ctx is bracketed by hipEvents
 * recorded on the ctx stream; sst_profile_read synchronises and returns the
 * summed milliseconds and launch counts per kernel id since the last read
 * (or enable), then resets them. */
int sst_profile_enable(sst_ctx* ctx, int on);
/* Same, restricted to the kernel ids set in kernel_mask (bit k = id k): each
 * bracketed launch costs two event records on the stream, so a benchmark
 * brackets only the kernels it reports. */
int sst_profile_select(sst_ctx* ctx, uint32_t kernel_mask);
/* Bracket only every `every`-th launch of each selected kernel (default 1):
 * the events' own cost on the stream is then spread over `every` launches
 * while the durations are still sampled from the live launch stream. */
int sst_profile_sample(sst_ctx* ctx, uint32_t every);
int sst_profile_read(sst_ctx* ctx, double* ms_total /* [SST_K_COUNT] */, int64_t* launches /* [SST_K_COUNT] */);

#ifdef __cplusplus
}
#endif
#endif /* SST_H */
