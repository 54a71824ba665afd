/*
 * hpgq.h — C-ABI of the MI355X FASTQ QC engine (libhpgq.so).
 *
 * This is the drop-in boundary for the per-read hot path of hpg-fastq
 * (SURVEY.md §8b).  Every entry point replaces one bioinfo-libs call made by
 * the reference's workflow workers, or the serial consumer merge that follows
 * them:
 *
 *   fastq_filter(reads, passed, failed, opts)     src/stats_fastq.c:224,
 *                                                 src/filter_fastq.c:148,
 *                                                 src/edit_fastq.c:166
 *   fastq_reads_stats(reads, rs_opts, fq_stats)   src/stats_fastq.c:230,244
 *   fastq_stats_consumer per-read + per-base merge src/stats_fastq.c:257-417
 *   fastq_edit(reads, opts)                       src/edit_fastq.c:154
 *   chaos_game_fill_tables(cg_data, batch, mode)  old/chaos_game.c:165-267
 *
 * The batch layout mirrors the SoA `fastq_batch_t` the old GPU path used
 * (fields evidenced at old/chaos_game.c:174-193): concatenated `seq` and
 * `quality` byte buffers plus `data_indices` with read i occupying
 * [data_indices[i], data_indices[i+1]).
 *
 * All functions return 0 on success or a negative HPGQ_E* code; no function
 * exits the process (the reference calls exit()/LOG_FATAL instead).
 * Plain pointers and sizes only — no C++ or framework types cross this line.
 */
#ifndef HPGQ_H
#define HPGQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------- */
/* constants                                                              */
/* ---------------------------------------------------------------------- */

/* src/commons_fastq.h:21-23 */
#define HPGQ_NO_VALUE   (-1)
#define HPGQ_MIN_VALUE  0
#define HPGQ_MAX_VALUE  100000

/* quality encodings (stats/edit --quality-encoding, src/stats_options.c:124-137) */
#define HPGQ_PHRED33 33
#define HPGQ_PHRED64 64

/* largest lmax: the dense per-position counters a ctx keeps on chip.
 * Reads of ANY length are merged: positions >= lmax of a longer read go to the
 * ctx's long-read tail (hpgq_read_counters_ext), like the reference's khash
 * maps, which have no length cap (src/stats_fastq.c:289-382). */
#define HPGQ_LMAX_LIMIT 1024
/* longest edit window (edit_left_length / edit_right_length): trims are
 * returned as two 16-bit fields (trim_out, hpgq_run_device) */
#define HPGQ_MAX_EDIT_LENGTH 65535
/* Device sequence / quality buffers must stay readable for this many bytes
 * past their last read (seq + data_indices[num_reads]): the engine fetches
 * unaligned 8-byte windows.  The bytes are never used. */
#define HPGQ_DEVICE_SLACK 8

/* error codes */
#define HPGQ_OK                  0
#define HPGQ_E_INVALID         (-1)   /* bad argument / parameter            */
#define HPGQ_E_HIP             (-2)   /* HIP runtime error                    */
#define HPGQ_E_NOMEM           (-3)   /* device or host allocation failed     */
#define HPGQ_E_READ_TOO_LONG   (-4)   /* hpgq_qdist_ / hpgq_adapt_sync / _read only: a counted read
                                         longer than the reserved rows (the engine
                                         and k-mers merge reads of any length)  */
#define HPGQ_E_NO_DEVICE       (-5)   /* no HIP device                        */
#define HPGQ_E_RCCL            (-6)   /* RCCL communicator / collective error */
#define HPGQ_E_STATE           (-7)   /* call not valid in this ctx state     */
#define HPGQ_E_FORMAT          (-8)   /* malformed FASTQ text                 */
#define HPGQ_E_IO              (-9)   /* file open / read / write failed      */
#define HPGQ_E_PAIRING        (-10)   /* mate pairs out of step: unequal or odd
                                         record counts, or a name mismatch    */

/* ---------------------------------------------------------------------- */
/* batch                                                                  */
/* ---------------------------------------------------------------------- */

/*
 * SoA read batch (fastq_batch_t, old/chaos_game.c:176-193).  Read i is
 * seq[data_indices[i] .. data_indices[i+1]) and the same range of quality.
 * data_indices has num_reads+1 entries, is non-decreasing and is `int` like
 * the reference's, so one batch holds < 2 GiB of bases.  Offsets are
 * absolute into seq/quality (data_indices[0] need not be 0).
 */
typedef struct hpgq_batch {
  int64_t        num_reads;
  const char    *seq;
  const char    *quality;
  const int32_t *data_indices;
} hpgq_batch_t;

/* ---------------------------------------------------------------------- */
/* parameters                                                             */
/* ---------------------------------------------------------------------- */

/*
 * Engine parameters.  Filter fields follow fastq_filter_options_new's
 * argument order (src/filter_fastq.c:140-145); edit fields follow
 * fastq_edit_options_new (src/edit_fastq.c:148-151).  Values are already
 * defaulted the way the reference drivers do it (NO_VALUE -> MIN/MAX_VALUE,
 * src/filter_fastq.c:195-206); hpgq_params_init() gives those defaults.
 * Quality thresholds are Phred scores; the engine compares them with
 * (quality_char - phred).
 */
typedef struct hpgq_params {
  int32_t phred;              /* 33 or 64                                    */
  int32_t lmax;               /* dense per-position length, 1..HPGQ_LMAX_LIMIT
                                 (longer reads: the long-read tail)          */

  int32_t stats_on;           /* accumulate stats counters                   */
  int32_t filter_on;          /* apply the filter (else every read passes)   */
  int32_t edit_on;            /* 5'/3' trim before filter and stats          */
  int32_t paired;             /* batches are mate pairs; pair passes iff both */

  /* fastq_filter_options_new(...) */
  int32_t min_read_length, max_read_length;
  int32_t min_read_quality, max_read_quality;
  int32_t max_out_of_quality;
  int32_t left_length, min_left_quality, max_left_quality;
  int32_t right_length, min_right_quality, max_right_quality;
  int32_t max_N;

  /* fastq_edit_options_new(left_len, minL, maxL, right_len, minR, maxR, 0,0,0);
   * the lengths are at most HPGQ_MAX_EDIT_LENGTH (hpgq_open: HPGQ_E_INVALID) */
  int32_t edit_left_length, edit_min_left_quality, edit_max_left_quality;
  int32_t edit_right_length, edit_min_right_quality, edit_max_right_quality;
} hpgq_params_t;

/* Defaults: phred33, lmax 256, stats on, filter/edit off, ranges open. */
void hpgq_params_init(hpgq_params_t *p);

/* ---------------------------------------------------------------------- */
/* packed counters (what the stats consumer merges; RCCL all-reduces)     */
/* ---------------------------------------------------------------------- */

/*
 * One counter set is a flat uint64_t array.  Offsets depend on lmax:
 *
 *   [0 .. 8)                 scalars, HPGQ_S_*
 *   hist_len   [lmax+1]      reads per length               (kh_length_histogram)
 *   hist_meanq [256]         reads per round(mean raw Q)     (kh_quality_histogram)
 *   hist_gc    [101]         reads per 100*(G+C)/len         (kh_gc_histogram)
 *   pos_qsum   [lmax]        sum of raw quality per position (kh_acc_quality_per_nt)
 *   pos_base   [5][lmax]     A, C, G, T, N per position      (kh_num_*_per_nt)
 *
 * kh_count_quality_per_nt[j] = sum_{L>j} hist_len[L] and the scalar totals of
 * stats_counters_t (src/stats_fastq.h:35-73) are derived from these by
 * hpgq_counters_summary().  A paired ctx holds two sets back to back
 * (mate 1, mate 2).  Everything is an exact integer sum, so shards merge by
 * plain addition.
 *
 * Reads longer than lmax.  The reference merges every position of every read
 * (src/stats_fastq.c:338-382, khash keyed by j < read_length).  A merged read
 * of length L > lmax adds its positions < lmax, its mean-quality and GC bins
 * and every scalar to the set above (hpgq_read_counters) and counts in
 * HPGQ_S_LONG_READS; its positions >= lmax and its length go to the ctx's
 * long-read tail.  hpgq_read_counters_ext returns both as ONE set in the
 * layout above for lmax_ext = max(lmax, longest merged read) -- the set an
 * lmax of lmax_ext would have held (HPGQ_S_LONG_READS 0).
 */
#define HPGQ_S_NUM_INPUT      0  /* reads seen                                 */
#define HPGQ_S_NUM_PASSED     1  /* reads that passed (== input if no filter)  */
#define HPGQ_S_NUM_FAILED     2
#define HPGQ_S_NUM_EDITED     3  /* reads whose trim removed >= 1 base         */
#define HPGQ_S_NUM_STATS      4  /* reads merged into stats (counters->num_reads) */
#define HPGQ_S_ACC_MEANQ_FX16 5  /* sum of floor(65536*sumQraw/len) (acc_quality) */
#define HPGQ_S_LONG_READS     6  /* merged reads longer than lmax: their positions
                                    >= lmax and length are in the long-read tail
                                    (0 in an extended set)                    */
#define HPGQ_S_RESERVED       7
#define HPGQ_NUM_SCALARS      8

#define HPGQ_MEANQ_BINS 256
#define HPGQ_GC_BINS    101

static inline size_t hpgq_off_hist_len(int lmax)   { (void)lmax; return HPGQ_NUM_SCALARS; }
static inline size_t hpgq_off_hist_meanq(int lmax) { return HPGQ_NUM_SCALARS + (size_t)lmax + 1; }
static inline size_t hpgq_off_hist_gc(int lmax)    { return hpgq_off_hist_meanq(lmax) + HPGQ_MEANQ_BINS; }
static inline size_t hpgq_off_pos_qsum(int lmax)   { return hpgq_off_hist_gc(lmax) + HPGQ_GC_BINS; }
static inline size_t hpgq_off_pos_base(int lmax, int b) {
  return hpgq_off_pos_qsum(lmax) + (size_t)lmax * (size_t)(1 + b);
}
static inline size_t hpgq_counters_len(int lmax)   { return hpgq_off_pos_base(lmax, 5); }

/* base order inside pos_base */
#define HPGQ_BASE_A 0
#define HPGQ_BASE_C 1
#define HPGQ_BASE_G 2
#define HPGQ_BASE_T 3
#define HPGQ_BASE_N 4

/* Derived view of one counter set (stats_counters_t, src/stats_fastq.h:35-73). */
typedef struct hpgq_summary {
  uint64_t num_reads;        /* reads merged into stats                       */
  uint64_t num_passed, num_failed, num_edited, num_input;
  int32_t  min_length, max_length;   /* 100000 / 0 when no reads (stats_counters_new) */
  uint64_t acc_length;
  double   mean_length;
  double   mean_quality_raw; /* acc_quality/num_reads, raw units (fx16 exact sum) */
  uint64_t num_A, num_C, num_G, num_T, num_N;
} hpgq_summary_t;

int hpgq_counters_summary(const uint64_t *set, int lmax, hpgq_summary_t *out);

/* ---------------------------------------------------------------------- */
/* engine context                                                         */
/* ---------------------------------------------------------------------- */

typedef struct hpgq_ctx hpgq_ctx_t;

/* Open a ctx on HIP device `device` (its own stream, counters zeroed). */
int  hpgq_open(hpgq_ctx_t **ctx, int device, const hpgq_params_t *p);
/* The same on the caller's HIP stream (hipStream_t, not NULL: HPGQ_E_INVALID),
 * which the ctx borrows and never destroys: a second ctx on hpgq_stream() of
 * the first runs in the first one's order (the CLI's single-end ctx for the
 * merged reads).  The stream must outlive the ctx. */
int  hpgq_open_on_stream(hpgq_ctx_t **ctx, int device, const hpgq_params_t *p, void *stream);
void hpgq_close(hpgq_ctx_t *ctx);

/*
 * Resident path: all pointers are DEVICE pointers (HBM).  Runs the fused
 * edit -> filter -> stats kernel asynchronously on the ctx stream and
 * accumulates into the ctx counters.  mask_out[i] = 1 if read (pair) i
 * passed, 0 otherwise; trim_out[i] = trim_start | trim_end << 16 when edit
 * is on (for pairs: mate 1 in trim_out[i], mate 2 in trim_out[num_reads+i]);
 * without edit trim_out is not touched, on this path and on the host path.
 * Either output may be NULL.  For paired ctxs b2 is mate 2 (same num_reads),
 * else it must be NULL.  seq / quality must be readable HPGQ_DEVICE_SLACK bytes
 * past the data end (hpgq_run_host pads its own staging copy).
 */
int  hpgq_run_device(hpgq_ctx_t *ctx, const hpgq_batch_t *b, const hpgq_batch_t *b2,
                     uint8_t *mask_out, uint32_t *trim_out);

/*
 * Host path: pointers are HOST memory (any: malloc'd is fine).  The batch is
 * copied into one of the ctx's two page-locked staging slots (1 MB pieces,
 * each piece's H2D queued as soon as it is copied) and the call returns once
 * the caller's buffers have been read: they are reusable on return.  The
 * copies run on a second stream, so this batch's H2D overlaps the previous
 * batch's kernels.  mask_out / trim_out are filled by hpgq_sync() or
 * hpgq_read_counters() (or when the slot is reused two calls later), not
 * before: synchronising hpgq_stream() yourself does not fill them, and the
 * arrays must stay allocated until one of those calls.  hpgq_close() drops
 * the outputs of calls not delivered by then (it never writes them).
 * A stats-only caller passes NULL for both and needs no hpgq_sync per batch.
 */
int  hpgq_run_host(hpgq_ctx_t *ctx, const hpgq_batch_t *b, const hpgq_batch_t *b2,
                   uint8_t *mask_out, uint32_t *trim_out);

/*
 * Host path without the staging copy: reserve the ctx's next page-locked
 * staging slot for a batch of num_reads reads holding nbytes sequence bytes
 * (and as many quality bytes; nbytes2 for mate 2 of a paired ctx, else 0 and
 * b2 NULL).  On return b (b2) point into the slot: the caller writes
 * data_indices[0..num_reads] (starting at 0, ending at <= nbytes), the
 * sequence and the quality bytes there -- e.g. while packing its reads -- and
 * calls hpgq_run_host with exactly that batch, which then only queues the DMA
 * (no host copy; the reference worker's pack becomes the only one).  The
 * pointers are valid until that hpgq_run_host, or the next hpgq_host_batch /
 * hpgq_run_host on the ctx (which abandons the reservation); waiting for the
 * slot's previous batch, as hpgq_run_host does, may deliver that batch's
 * outputs.  Replaces the worker's malloc of the SoA batch
 * (fastq_stats_worker; src/stats_fastq.c:202-250).
 */
int  hpgq_host_batch(hpgq_ctx_t *ctx, int64_t num_reads, size_t nbytes, size_t nbytes2,
                     hpgq_batch_t *b, hpgq_batch_t *b2);

/* Wait for all work on the ctx stream (and deliver hpgq_run_host outputs).
 * Reads of any length are filtered, trimmed and merged.  The long-read tail
 * grows on the host: hpgq_run_host sizes it from the batch's own offsets before
 * the launch; hpgq_run_device cannot see them, so a device batch holding a
 * merged read longer than lmax + the tail reserved so far has that read's
 * excess positions merged HERE, by a second pass over the batch -- such a
 * device batch must stay valid until the next hpgq_sync / hpgq_read_counters /
 * hpgq_read_counters_ext / hpgq_reset (hpgq_reserve_length avoids the second
 * pass).  Never HPGQ_E_READ_TOO_LONG. */
int  hpgq_sync(hpgq_ctx_t *ctx);

/* Reserve the long-read tail for merged reads up to max_len bases (no-op when
 * max_len <= lmax or already reserved; waits for the ctx stream when it
 * grows the tail).  The CLI calls it with each parse unit's longest record
 * (hpgq_parser_max_length). */
int  hpgq_reserve_length(hpgq_ctx_t *ctx, int64_t max_len);

/* The counters of every merged read at full length: nm sets in the layout of
 * hpgq_counters_len(*lmax_ext), lmax_ext = max(lmax, longest merged read)
 * (HPGQ_S_LONG_READS 0; every other entry as an lmax of lmax_ext would give).
 * out == NULL: only *lmax_ext (size query).  Synchronises like
 * hpgq_read_counters.  After hpgq_allreduce the sum over the ranks, and then it
 * is COLLECTIVE: every rank of the communicator calls it (the ranks agree on
 * lmax_ext and sum their tails with two RCCL all-reduces). */
int  hpgq_read_counters_ext(hpgq_ctx_t *ctx, uint64_t *out, size_t n, int32_t *lmax_ext);

/* Zero the ctx counters (async on the ctx stream). */
int  hpgq_reset(hpgq_ctx_t *ctx);

/* Number of uint64 in this ctx's counter buffer (1 or 2 sets). */
size_t hpgq_counters_size(const hpgq_ctx_t *ctx);

/* Copy the counters to host memory (synchronises the ctx; like hpgq_sync it
 * also delivers pending hpgq_run_host masks / trims). */
int  hpgq_read_counters(hpgq_ctx_t *ctx, uint64_t *out, size_t n);

/* DEPRECATED no-op, kept only so that round-1 callers still link: the kernels
 * add their workgroup partials into the counters themselves (global
 * atomics), so the counter buffer holds the totals as soon as the ctx stream
 * has run the batch.  New code does not call it. */
int  hpgq_fold(hpgq_ctx_t *ctx);

/* Device pointer of this ctx's own counter buffer (for an external
 * all-reduce); holds the totals once the ctx stream has run the batches. */
uint64_t *hpgq_counters_device(hpgq_ctx_t *ctx);

/* HIP stream (hipStream_t) the ctx runs on.  Synchronising it waits for the
 * kernels but does not deliver hpgq_run_host outputs (hpgq_sync does). */
void *hpgq_stream(hpgq_ctx_t *ctx);

/* ---------------------------------------------------------------------- */
/* multi-GPU: RCCL over xGMI (one process per GPU)                        */
/* ---------------------------------------------------------------------- */

#define HPGQ_COMM_ID_BYTES 128

/* rank 0 creates the id and ships it to the other ranks out of band */
int  hpgq_comm_unique_id(char id[HPGQ_COMM_ID_BYTES]);
int  hpgq_comm_init(hpgq_ctx_t *ctx, int nranks, int rank, const char id[HPGQ_COMM_ID_BYTES]);
/* ncclAllReduce(sum, uint64) of the packed counters on the ctx stream, OUT OF
 * PLACE: the ctx keeps accumulating its own reads, the sum over the ranks goes
 * to a second buffer that hpgq_read_counters returns until the next run or
 * reset (so calling it twice, or after more batches, never double-counts). */
int  hpgq_allreduce(hpgq_ctx_t *ctx);
/* device pointer of the all-reduced counters */
uint64_t *hpgq_global_counters_device(hpgq_ctx_t *ctx);
/* ranks in the ctx's communicator (ncclCommCount); HPGQ_E_STATE without one.
 * The multi-GPU bench reports it next to its own world size
 * (the old tool's --gpu-num-devices, old/main_hpg_fastq_old.c:113,161). */
int  hpgq_comm_count(hpgq_ctx_t *ctx, int *count);

/*
 * Kernel routing for tests and A/B measurements only.  The
 * library never reads routing choices from the environment: a ctx runs the
 * automatic chain unless this is called.  It waits for the ctx stream and
 * re-plans the chain; counters are kept.
 *   AUTO        segmented kernel first (hex, or wide for lmax 157..252),
 *               adaptive hex/wide first stage, catch-all for the rest
 *   CATCH_ALL   the one-read-per-wave catch-all kernel alone
 *   FIRST_TRI / FIRST_HEX / FIRST_WIDE   that geometry first (not adaptive)
 * | NO_ADAPTIVE  (with AUTO) keep the first choice for every call
 */
#define HPGQ_ROUTE_AUTO        0
#define HPGQ_ROUTE_CATCH_ALL   1
#define HPGQ_ROUTE_FIRST_TRI   2
#define HPGQ_ROUTE_FIRST_HEX   3
#define HPGQ_ROUTE_FIRST_WIDE  4
#define HPGQ_ROUTE_NO_ADAPTIVE 0x10
int  hpgq_debug_set_route(hpgq_ctx_t *ctx, int route);
/*
 * Tests only: launch at most max_wg workgroups per stage (0, the default: no
 * limit), the long-read tail's second pass included, so that a small batch
 * gives every wave of a stage several units.  Never read from the
 * environment; kept across hpgq_debug_set_route and hpgq_reset.
 * HPGQ_E_INVALID for a NULL ctx or a negative value.
 */
int  hpgq_debug_set_max_workgroups(hpgq_ctx_t *ctx, int max_wg);
/*
 * The waves stage `stage` of chain `chain` launches at most (its persistent
 * grid under the limit above, times the waves per workgroup) and the reads
 * per unit it iterates over.  chain: 0, or 1 for the adaptive wide-first
 * chain; stage: 1 (its own block), 2 and 3 (the follow-up stages: the first
 * stage's block), 4 (the long-read tail's second pass: 64).  HPGQ_E_INVALID
 * for a chain or stage the ctx does not have.
 */
int  hpgq_debug_stage_waves(const hpgq_ctx_t *ctx, int chain, int stage, int *waves, int *unit_reads);

/* ---------------------------------------------------------------------- */
/* chaos-game (CGR) accumulator, old/chaos_game.c:165-267                 */
/* ---------------------------------------------------------------------- */

#define HPGQ_CGR_ALL_READS        0
#define HPGQ_CGR_ONLY_VALID_READS 1   /* mode == ONLY_VALID_READS (:188) */

typedef struct hpgq_cgr hpgq_cgr_t;

/*
 * k: word size (dim = 2^k, tables dim x dim, 1 <= k <= 12);
 * base_quality: subtracted k times per word (chaos_game_data_init :97).
 */
int  hpgq_cgr_open(hpgq_cgr_t **cg, int device, int k, int base_quality);
void hpgq_cgr_close(hpgq_cgr_t *cg);

/*
 * One chaos_game_fill_tables() call over a DEVICE batch.  The double CGR
 * state starts at (dim/2, dim/2) for every call and is carried across the
 * reads of the batch exactly as the reference does.  status (device, may be
 * NULL) is read_status[]; in ONLY_VALID_READS mode reads with status[i] != 1
 * (VALID_READ) are skipped.
 */
int  hpgq_cgr_fill_device(hpgq_cgr_t *cg, const hpgq_batch_t *b, const uint8_t *status, int mode);
int  hpgq_cgr_sync(hpgq_cgr_t *cg);
int  hpgq_cgr_reset(hpgq_cgr_t *cg);
/* table_seq, table_q: dim*dim uint32 each, row-major [co_x][co_y]; word_count: fq_word_count */
int  hpgq_cgr_read(hpgq_cgr_t *cg, uint32_t *table_seq, uint32_t *table_q, uint32_t *word_count);
void *hpgq_cgr_stream(hpgq_cgr_t *cg);
/* reads the last fill call had to replay sequentially (diagnostic) */
int64_t hpgq_cgr_last_replays(hpgq_cgr_t *cg);

/*
 * Multi-GPU (read-sharded fills, one process per GPU): RCCL communicator
 * from a unique id (hpgq_comm_unique_id), then one all-reduce of
 * [table_seq | table_q | word_count] as uint32 sums, which wrap like the
 * reference's unsigned tables (old/chaos_game.c:253-258).  Out of place:
 * hpgq_cgr_read returns the sums until the next fill or reset.
 */
int  hpgq_cgr_comm_init(hpgq_cgr_t *cg, int nranks, int rank, const char id[HPGQ_COMM_ID_BYTES]);
int  hpgq_cgr_allreduce(hpgq_cgr_t *cg);
/* ranks in the chaos-game communicator (ncclCommCount); HPGQ_E_STATE without one */
int  hpgq_cgr_comm_count(hpgq_cgr_t *cg, int *count);
/* device pointer of the all-reduced [table_seq | table_q | word_count] */
uint32_t *hpgq_cgr_global_device(hpgq_cgr_t *cg);

/*
 * Path selection.  AUTO (default): for k <= 7 (either mode) a coalesced
 * integer pass computes each word's cell from its own k bases, which is
 * provably the reference's (int)f cell unless some axis sees a run of
 * >= 48-k toward-dim moves or a counted read holds bytes other than A/C/G/T/N
 * or qualities >= 128; such a call is redone by the exact double simulation
 * on the device.  In ONLY_VALID_READS mode the skipped reads' bytes count as
 * absent (they move nothing, :188).  EXACT: always the exact simulation.
 * Both are bit-identical to old/chaos_game.c:165-267.
 */
#define HPGQ_CGR_PATH_AUTO  0
#define HPGQ_CGR_PATH_EXACT 1
int  hpgq_cgr_set_path(hpgq_cgr_t *cg, int path);
/* 1 if a fill since the previous sync ran the exact simulation, 0 if the
 * stream pass sufficed for all of them (read after hpgq_cgr_sync).  A
 * streamed fill whose gate is set is simulated exactly inside the next
 * hpgq_cgr_sync / hpgq_cgr_read / hpgq_cgr_reset, so its batch must stay
 * valid until then (as for any asynchronous fill). */
int  hpgq_cgr_last_exact(hpgq_cgr_t *cg);

/*
 * CGR post-processing on the host (O(4^k), old/chaos_game.c:269-593); tables
 * are row-major [co_x][co_y] of dim*dim cells as hpgq_cgr_read returns them.
 *   genomic-signature (GS) file = header_gs_t (old/chaos_game.h:65-70: char
 *   gs_filename[180], u32 word_size_k, dim_x, dim_y, ref_word_count) + the
 *   dim*dim u32 table.
 */
#define HPGQ_GS_HEADER_BYTES 196
/* chaos_game_load_table_gs_direct (:297-318) */
int  hpgq_cgr_load_gs(const char *path, int k, uint32_t *table_gs, uint32_t *ref_word_count);
/* header_gs_init (:43-50) + the table: writes a GS file for a reference */
int  hpgq_cgr_write_gs(const char *path, int k, const uint32_t *table, uint32_t word_count);
/* chaos_game_calculate_table_dif (:320-373): int table_dif = seq*128/(fq/4^k) - gs*128/(ref/4^k) */
int  hpgq_cgr_table_dif(int k, const uint32_t *table_seq, uint32_t fq_word_count,
                        const uint32_t *table_gs, uint32_t ref_word_count, int32_t *table_dif,
                        int32_t *highest, int32_t *lowest);
/* chaos_game_validate_table_dif (:375-408): mean and standard deviation of table_dif */
int  hpgq_cgr_dif_stats(int k, const int32_t *table_dif, double *mean, double *std_dev);
/* chaos_game_normalize_quality_table_ (:487-502), in place */
int  hpgq_cgr_normalize_quality(int k, const uint32_t *table_seq, uint32_t *table_q);
/* chaos_game_generate_pgm_file_ (:521-593) */
int  hpgq_cgr_write_pgm(const char *path, int k, const uint32_t *table, double norm);
/* chaos_game_write_table_images (:410-472): <dir>/<fq file>_k=<k>_FG.pgm, _QQ.pgm
 * (normalises table_q in place) and, when table_dif is given, _FG_dif.pgm */
int  hpgq_cgr_write_images(const char *report_dir, const char *fq_path, int k,
                           const uint32_t *table_seq, uint32_t *table_q, uint32_t fq_word_count,
                           const int32_t *table_dif);

/* ---------------------------------------------------------------------- */
/* genomic signature of a FASTA (what --gs-filename reads)                  */
/* ---------------------------------------------------------------------- */

/*
 * Build-defined (the reference's generator is absent; lut_table_init,
 * old/chaos_game.c:51-72, is what is left of it).  The text is
 * a FASTA byte stream cut anywhere between calls.  '>' outside a header starts
 * a header, which runs up to and including the next '\n', is ignored byte for
 * byte, ends the current word and counts one sequence.  Outside headers
 * A/C/G/T in either case are bases, N/n ends the current word, every other
 * byte is skipped and does not end the word.  Every window of k consecutive
 * bases is a word and adds 1 to table[co_x][co_y]: bit i of co_x (co_y) is dx
 * (dy) of the window's i-th oldest base, dx = 1 for A/T, dy = 1 for G/T --
 * the integer (int)f cell of old/chaos_game.c:201-251, not the carried double
 * recurrence.  Cells are u32 and wrap; no cell exceeds info.words, so
 * words < 2^32 means nothing wrapped.
 */
typedef struct hpgq_gs hpgq_gs_t;
typedef struct hpgq_gs_info { uint64_t words, bases, ns, sequences; } hpgq_gs_info_t;

/* 1 <= k <= 12 (else HPGQ_E_INVALID, before any device call); stream: the HIP
 * stream to run on, or NULL for a stream of its own */
int  hpgq_gs_open(hpgq_gs_t **gs, int device, int k, void *stream);
void hpgq_gs_close(hpgq_gs_t *gs);
/* Add n bytes (0 <= n < 2^31) of DEVICE text, async on the stream: the header
 * flag, the word counter and the last k-1 bases live on the device, so no call
 * waits for the GPU.  The text must stay valid until the stream has run it;
 * any alignment. */
int  hpgq_gs_add_device(hpgq_gs_t *gs, const char *text_dev, int64_t n);
/* Add n bytes of HOST text (any n >= 0) through two page-locked 8 MB slots;
 * the caller's buffer is reusable on return. */
int  hpgq_gs_add_host(hpgq_gs_t *gs, const char *text, int64_t n);
int  hpgq_gs_sync(hpgq_gs_t *gs);
/* zero the table and the counts and forget the carried state (async) */
int  hpgq_gs_reset(hpgq_gs_t *gs);
/* table: dim*dim u32, row-major [co_x][co_y]; either output may be NULL (not
 * both).  Synchronises the stream. */
int  hpgq_gs_read(hpgq_gs_t *gs, uint32_t *table, hpgq_gs_info_t *info);
/* Tests only: at most max_wg workgroups per kernel (0, the default: no limit),
 * so that a small text gives every workgroup several tiles. */
int  hpgq_gs_debug_set_max_workgroups(hpgq_gs_t *gs, int max_wg);

/* ---------------------------------------------------------------------- */
/* stats --kmers: 5-mer counts (src/stats_options.c:274, merge              */
/* src/stats_fastq.c:384-410, report src/stats_report.c:492-563)            */
/* ---------------------------------------------------------------------- */

#define HPGQ_KMER_K    5
#define HPGQ_NUM_KMERS 1024   /* NUM_KMERS, src/stats_fastq.h:58 */

/*
 * Build-defined (the per-read k-mer code is in the absent bioinfo-libs;
 * DESIGN.md §2.5): 5-mers of exact uppercase A/C/G/T, id = sum code_i *
 * 4^(4-i) with A=0 C=1 G=2 T=3, counted at every start position
 * p <= len-5 of every counted read.  by_pos is [HPGQ_NUM_KMERS][npos] u64
 * (counter_by_pos); a k-mer's counter is its row sum.  hpgq_kmers_read gives
 * the dense starts p < npos = lmax-4; starts >= npos of longer reads (the
 * reference's counter_by_pos grows with the read, src/stats_fastq.c:394-407)
 * are in the tail, and hpgq_kmers_read_ext returns all of them as
 * [HPGQ_NUM_KMERS][npos_ext], npos_ext = max(lmax, longest counted read) - 4.
 * The tail's reservation and second pass work as the engine's (hpgq_sync).
 */
typedef struct hpgq_kmers hpgq_kmers_t;

/* stream: run on this HIP stream (e.g. hpgq_stream(ctx), so counting sees the
 * engine's mask of the same batch), or NULL for an own stream */
int  hpgq_kmers_open(hpgq_kmers_t **km, int device, int lmax, void *stream);
void hpgq_kmers_close(hpgq_kmers_t *km);
/* Count a DEVICE batch, async; mask (device, may be NULL): only reads with
 * mask[i] == 1 (the engine's mask_out: passed) are counted. */
int  hpgq_kmers_count_device(hpgq_kmers_t *km, const hpgq_batch_t *b, const uint8_t *mask);
int  hpgq_kmers_sync(hpgq_kmers_t *km);
int  hpgq_kmers_reset(hpgq_kmers_t *km);
/* HPGQ_NUM_KMERS * (lmax-4) (0 when lmax < 5) */
size_t hpgq_kmers_size(const hpgq_kmers_t *km);
/* copy by_pos to host (synchronises); n >= hpgq_kmers_size() */
int  hpgq_kmers_read(hpgq_kmers_t *km, uint64_t *by_pos, size_t n);
/* device pointer of by_pos (for an external all-reduce) */
uint64_t *hpgq_kmers_device(hpgq_kmers_t *km);
/* tail for counted reads up to max_len bases (cf. hpgq_reserve_length) */
int  hpgq_kmers_reserve_length(hpgq_kmers_t *km, int64_t max_len);
/* every start: [HPGQ_NUM_KMERS][*npos_ext] (by_pos == NULL: size query) */
int  hpgq_kmers_read_ext(hpgq_kmers_t *km, uint64_t *by_pos, size_t n, int32_t *npos_ext);

/* ---------------------------------------------------------------------- */
/* stats --quality-dist: bases per (read position, quality byte)            */
/* ---------------------------------------------------------------------- */

/*
 * Build-defined (the reference reports a mean per position only; DESIGN.md
 * §2.8).  Every base j of every counted read adds 1 to hist[j][b], b its RAW
 * quality byte as an unsigned index: hist is [npos][HPGQ_QDIST_VALUES] u64,
 * positions from the read's first base, no lmax cap.  The table knows nothing
 * of phred; hpgq_qdist_quantiles reads it as qualities Q = (signed char)b -
 * phred (quirk Q13).
 *
 * The table has `rows` rows.  A counted read longer than the rows has only its
 * positions below them counted and makes hpgq_qdist_sync and hpgq_qdist_read
 * return HPGQ_E_READ_TOO_LONG until hpgq_qdist_reset: call
 * hpgq_qdist_reserve_length first; the parser gives the longest record
 * (hpgq_parser_max_length).  There is no second pass and no tail.
 */
typedef struct hpgq_qdist hpgq_qdist_t;
#define HPGQ_QDIST_VALUES 256
typedef struct hpgq_qdist_row { uint64_t count; int32_t min, p10, q1, median, q3, p90, max; } hpgq_qdist_row_t;

/* rows >= 1; 0 <= base <= 192: the 64 byte values [base, base + 64) are
 * counted on chip, the others by a slower path -- a speed hint (pass phred),
 * the table is exact for all 256 values whatever it is.  stream: as
 * hpgq_kmers_open.  HPGQ_E_INVALID before any device call. */
int  hpgq_qdist_open(hpgq_qdist_t **qd, int device, int rows, int base, void *stream);
void hpgq_qdist_close(hpgq_qdist_t *qd);
/* grow the table to >= max_len rows (counts kept; async on the stream; never shrinks) */
int  hpgq_qdist_reserve_length(hpgq_qdist_t *qd, int64_t max_len);
/* Count a DEVICE batch, async; only `quality` and `data_indices` are read
 * (quality readable HPGQ_DEVICE_SLACK bytes past the data end); mask (device,
 * may be NULL): only reads with mask[i] == 1 are counted. */
int  hpgq_qdist_count_device(hpgq_qdist_t *qd, const hpgq_batch_t *b, const uint8_t *mask);
int  hpgq_qdist_sync(hpgq_qdist_t *qd);
/* zero the table, the longest read and the too-long state (async) */
int  hpgq_qdist_reset(hpgq_qdist_t *qd);
/* hist[p * 256 + b], p < *npos = the longest counted read; n >= *npos * 256
 * (hist == NULL: size query).  Synchronises. */
int  hpgq_qdist_read(hpgq_qdist_t *qd, uint64_t *hist, size_t n, int32_t *npos);
/* Tests only: at most max_wg workgroups (0, the default: no limit), so that a
 * small batch gives every workgroup several read groups. */
int  hpgq_qdist_debug_set_max_workgroups(hpgq_qdist_t *qd, int max_wg);
/* Host only, no device (csrc/hpgq_qdist_post.cpp).
 * dst[p][b] += src[p][b] for p < npos_src: merges shards' tables
 * (HPGQ_E_INVALID if npos_src > npos_dst). */
int  hpgq_qdist_add(uint64_t *dst, int npos_dst, const uint64_t *src, int npos_src);
/* Per position p: c = the row sum; the num/den quantile is the smallest Q, in
 * ascending signed order (bytes 128..255 before 0..127), whose cumulative
 * count reaches the rank max(1, ceil(num c / den)), exact for every u64 c;
 * rows[p] = {c, min, 1/10, 1/4, 1/2, 3/4, 9/10, max}, all zeros when c == 0. */
int  hpgq_qdist_quantiles(const uint64_t *hist, int npos, int phred, hpgq_qdist_row_t *rows);

/* ---------------------------------------------------------------------- */
/* stats --duplication: exact sequence duplication levels                   */
/* ---------------------------------------------------------------------- */

/*
 * Build-defined.  Every counted read adds 1 to the count of
 * its sequence's 64-bit fingerprint (hpgq_dup_fingerprint; never 0) in an
 * open-addressing table in device memory: the multiset {fingerprint -> count},
 * count u64.  Two reads are the same sequence iff their fingerprints are
 * equal; the bytes are compared as they stand.  The levels are read from the
 * table; shards are merged through hpgq_dup_export / hpgq_dup_import, never by
 * adding levels (one sequence may be in both).
 *
 * The table has 2^log2_slots slots of 16 bytes and doubles as often as needed
 * to stay at most half full, up to 2^log2_max_slots; a call that would need
 * more returns HPGQ_E_NOMEM and leaves the table as it was.
 */
typedef struct hpgq_dup hpgq_dup_t;
#define HPGQ_DUP_LEVELS 16
/* lower bounds 1..10, 50, 100, 500, 1000, 5000, 10000: level i holds the
 * counts in [lo_i, lo_{i+1}), the last one unbounded (hpgq_dup_level_bound) */
typedef struct hpgq_dup_levels {
  uint64_t reads;                          /* sum of the counts                     */
  uint64_t distinct;                       /* sequences (occupied slots)            */
  uint64_t max_count;                      /* the highest count                     */
  uint64_t distinct_at[HPGQ_DUP_LEVELS];   /* sequences at each level               */
  uint64_t reads_at[HPGQ_DUP_LEVELS];      /* the reads they account for            */
} hpgq_dup_levels_t;

/* 4 <= log2_slots <= log2_max_slots <= 34; stream: as hpgq_kmers_open.
 * HPGQ_E_INVALID before any device call. */
int  hpgq_dup_open(hpgq_dup_t **d, int device, int log2_slots, int log2_max_slots, void *stream);
void hpgq_dup_close(hpgq_dup_t *d);
/* empty the table and clear the error word (async; the slots stay allocated) */
int  hpgq_dup_reset(hpgq_dup_t *d);
/* Count a DEVICE batch, async; only `seq` and `data_indices` are read (seq
 * readable HPGQ_DEVICE_SLACK bytes past the data end, any alignment, absolute
 * offsets); reads of any length, 0 included.  mask (device, may be NULL): only
 * reads with mask[i] == 1 are counted.  Synchronises only when the table may
 * have to grow.  HPGQ_E_NOMEM past log2_max_slots (nothing of the batch is
 * counted). */
int  hpgq_dup_count_device(hpgq_dup_t *d, const hpgq_batch_t *b, const uint8_t *mask);
/* waits for the stream; HPGQ_E_STATE if a kernel found the table full (sticky
 * until hpgq_dup_reset; the host's load bound makes it unreachable) */
int  hpgq_dup_sync(hpgq_dup_t *d);
/* the levels of the table, binned on the device.  Synchronises. */
int  hpgq_dup_levels(hpgq_dup_t *d, hpgq_dup_levels_t *out);
/* The occupied slots, compacted on the device, in no particular order: *n
 * pairs (keys == NULL or counts == NULL: size query; cap < *n:
 * HPGQ_E_INVALID).  Synchronises. */
int  hpgq_dup_export(hpgq_dup_t *d, uint64_t *keys, uint64_t *counts, size_t cap, size_t *n);
/* Add n HOST pairs to the table (counts[i] to the count of keys[i]): the merge
 * of workers, GPUs and ranks.  A key or a count of 0 is HPGQ_E_INVALID. */
int  hpgq_dup_import(hpgq_dup_t *d, const uint64_t *keys, const uint64_t *counts, size_t n);
/* Tests only: at most max_wg workgroups per kernel (0, the default: no limit). */
int  hpgq_dup_debug_set_max_workgroups(hpgq_dup_t *d, int max_wg);
/* Tests only: the fingerprint of every read of a device batch (no mask, no
 * insertion) to out_host[num_reads].  Synchronises. */
int  hpgq_dup_debug_fingerprints(hpgq_dup_t *d, const hpgq_batch_t *b, uint64_t *out_host);
/* Measurement only (tools/dup_rate.py): with on != 0 every hpgq_dup_count_device
 * records HIP events around its two kernels; hpgq_dup_debug_last_times waits
 * for them and gives the fingerprint and the insert kernel's time of the last
 * call's last launch in microseconds (HPGQ_E_STATE when none was recorded). */
int  hpgq_dup_debug_set_timing(hpgq_dup_t *d, int on);
int  hpgq_dup_debug_last_times(hpgq_dup_t *d, float *fp_us, float *insert_us);
/* Tests only: the table's size now and how often it has grown since it was opened. */
int  hpgq_dup_debug_info(hpgq_dup_t *d, int *log2_slots, int64_t *rehashes);
/* Host only, no device (csrc/hpgq_dup_post.cpp). */
uint64_t hpgq_dup_fingerprint(const void *s, size_t n);
uint64_t hpgq_dup_level_bound(int level);   /* 0 outside 0 .. HPGQ_DUP_LEVELS - 1 */
/* the levels of n counts (zeros are no sequence; sums mod 2^64) */
int  hpgq_dup_levels_of(const uint64_t *counts, size_t n, hpgq_dup_levels_t *out);

/*
 * stats --overrepresented: the most frequent sequences (build-defined,
 * DESIGN.md §2.10).  A table in keeping mode copies, after each batch's insert,
 * the bytes of every counted read of that batch whose key's count in THIS
 * table is now >= min_count and that has no representative yet, once, into a
 * device arena of the table.  After hpgq_dup_sync every key whose count here
 * is >= min_count and that was counted from reads at least once after reaching
 * it has a representative; hpgq_dup_import makes none.  A representative takes
 * 16 bytes + its length rounded up to 16 bytes of the arena; one that does not
 * fit is not kept and hpgq_dup_sync / hpgq_dup_sequence return HPGQ_E_NOMEM
 * until hpgq_dup_reset (counts, levels, export and top are unaffected).
 */
/* Only on an empty table (after open or reset, before any count or import):
 * otherwise HPGQ_E_STATE.  min_count == 0 turns keeping off and frees the arena.
 * 1 <= arena_bytes <= 2^40.  Settings survive hpgq_dup_reset, which drops every
 * representative and empties the arena. */
int  hpgq_dup_keep_sequences(hpgq_dup_t *d, uint64_t min_count, uint64_t arena_bytes);
/* The entries with count >= min_count (>= 1), count descending, ties by key
 * ascending: the first min(cap, *total) of them to keys[] / counts[];
 * *total = how many qualify (keys == NULL: query only).  Only the qualifying
 * pairs leave the device.  Synchronises.  Works with keeping off. */
int  hpgq_dup_top(hpgq_dup_t *d, uint64_t min_count, uint64_t *keys, uint64_t *counts, size_t cap, size_t *total);
/* The representative of key in THIS table: *len = its length, bytes to buf
 * (buf == NULL: length query; cap < *len: HPGQ_E_INVALID with *len set).
 * *len = -1 and HPGQ_OK when the key is absent or has no representative here.
 * Synchronises.  HPGQ_E_STATE with keeping off. */
int  hpgq_dup_sequence(hpgq_dup_t *d, uint64_t key, void *buf, size_t cap, int64_t *len);
/* Tests only: representatives held and the sum of their lengths. */
int  hpgq_dup_debug_kept(hpgq_dup_t *d, uint64_t *sequences, uint64_t *bytes);
/* Measurement only: with hpgq_dup_debug_set_timing on and keeping on, the time
 * of the last launch's keep kernel in microseconds (else HPGQ_E_STATE). */
int  hpgq_dup_debug_last_keep_time(hpgq_dup_t *d, float *keep_us);
/* Host only, no device: the same selection over n (key, count) pairs. */
int  hpgq_dup_top_of(const uint64_t *keys, const uint64_t *counts, size_t n, uint64_t min_count,
                     uint64_t *out_keys, uint64_t *out_counts, size_t cap, size_t *total);

/* ---------------------------------------------------------------------- */
/* stats --adapters: adapter content per read position                      */
/* ---------------------------------------------------------------------- */

/*
 * Build-defined.  A probe is a string of HPGQ_ADAPT_MIN_LEN
 * .. HPGQ_ADAPT_MAX_LEN bytes, each one of A C G T (upper case); a set holds 1
 * .. HPGQ_ADAPT_MAX_PROBES of them (identical probes give identical rows).
 * Probe a occurs at position j of a read of n bytes iff j + K <= n and the
 * read's bytes [j, j + K) equal the probe's: bytes.find, nothing else; N,
 * lower case and every other byte value never match, and a window never
 * reaches past the read's last byte.  For every counted read and every probe
 * that occurs in it, first[a][p] += 1 at the LOWEST such position p (u64).
 * reads: the counted reads; with_any: those in which at least one probe
 * occurs; npos: the longest counted read.
 *
 * The table has `rows` positions.  A counted read longer than the rows makes
 * hpgq_adapt_sync and hpgq_adapt_read return HPGQ_E_READ_TOO_LONG until
 * hpgq_adapt_reset (the table's contents are unspecified until then): call
 * hpgq_adapt_reserve_length first.  There is no second pass and no tail.
 */
typedef struct hpgq_adapt hpgq_adapt_t;
#define HPGQ_ADAPT_MAX_PROBES 32
#define HPGQ_ADAPT_MIN_LEN 8
#define HPGQ_ADAPT_MAX_LEN 32
typedef struct hpgq_adapt_info { uint64_t reads, with_any; int32_t nprobes, npos; } hpgq_adapt_info_t;

/* probes: nprobes NUL-terminated strings, copied; rows >= 1; stream: as
 * hpgq_kmers_open.  HPGQ_E_INVALID before any device call. */
int  hpgq_adapt_open(hpgq_adapt_t **ad, int device, const char *const *probes, int nprobes, int rows, void *stream);
void hpgq_adapt_close(hpgq_adapt_t *ad);
/* grow the table to >= max_len rows (counts kept; async on the stream; never shrinks) */
int  hpgq_adapt_reserve_length(hpgq_adapt_t *ad, int64_t max_len);
/* Count a DEVICE batch, async; only `seq` and `data_indices` are read (seq
 * readable HPGQ_DEVICE_SLACK bytes past the data end, any alignment, absolute
 * offsets); reads of any length, 0 included, and an empty batch.  mask (device,
 * may be NULL): only reads with mask[i] == 1 are counted. */
int  hpgq_adapt_count_device(hpgq_adapt_t *ad, const hpgq_batch_t *b, const uint8_t *mask);
int  hpgq_adapt_sync(hpgq_adapt_t *ad);
/* zero the table, both scalars, the longest read and the too-long state
 * (async); the probes and the rows stay */
int  hpgq_adapt_reset(hpgq_adapt_t *ad);
/* first[a * npos + p]; n >= nprobes * npos (first == NULL: size query, info
 * only; info may be NULL if first is not).  Synchronises. */
int  hpgq_adapt_read(hpgq_adapt_t *ad, uint64_t *first, size_t n, hpgq_adapt_info_t *info);
/* Tests only: at most max_wg workgroups (0, the default: no limit). */
int  hpgq_adapt_debug_set_max_workgroups(hpgq_adapt_t *ad, int max_wg);
/* Host only, no device (csrc/hpgq_adapt_post.cpp).
 * dst[a][p] += src[a][p] for p < npos_src, dst's rows npos_dst long and src's
 * npos_src: merges shards' tables (HPGQ_E_INVALID if npos_src > npos_dst). */
int  hpgq_adapt_add(uint64_t *dst, int npos_dst, const uint64_t *src, int npos_src, int nprobes);
/* the lowest position at which probe occurs in s[0, n), -1 if none, -2 for a
 * probe that breaks the rules above */
int64_t hpgq_adapt_find(const void *s, size_t n, const char *probe);
/* the number of default probes (6); for 0 <= i < 6 *name and *probe (either
 * may be NULL) are set to static strings */
int  hpgq_adapt_default(int i, const char **name, const char **probe);

/* ---------------------------------------------------------------------- */
/* edit --clip-adapters: cut reads at the adapter                           */
/* ---------------------------------------------------------------------- */

/*
 * Build-defined.  The probes are those of hpgq_adapt (same
 * rules, same default set); min_overlap is 1 .. HPGQ_ADAPT_MAX_LEN (the CLI's
 * default: HPGQ_ADAPT_MIN_LEN).  Probe a of K bytes matches at position j of a
 * read of n bytes iff, with m = min(K, n - j), the read's bytes [j, j + m)
 * equal the probe's first m as they stand and m == K (a whole occurrence) or
 * m >= min_overlap (the read ends inside the adapter).  N, lower case and every
 * other byte value never match, and nothing behind the read's last byte counts.
 * c is the lowest j at which any probe matches, n if none does; the kept read
 * is bytes [0, c) of sequence and quality (c == 0: an empty read); the winner
 * is the lowest probe that matches at c (0xFF when c == n).  The scalars are
 * plain u64 sums over every batch since open or reset.
 *
 * Input as hpgq_adapt_count_device: device pointers, seq and quality readable
 * HPGQ_DEVICE_SLACK bytes past the data end, any alignment, absolute offsets,
 * reads of any length, 0 included, and an empty batch.  The inputs are never
 * written.  Everything runs on the handle's stream.
 */
typedef struct hpgq_clip hpgq_clip_t;
typedef struct hpgq_clip_info {
  uint64_t reads, clipped, bases_removed, by_probe[HPGQ_ADAPT_MAX_PROBES];
  int32_t nprobes, min_overlap;
} hpgq_clip_info_t;

/* probes: nprobes NUL-terminated strings, copied; stream: as hpgq_kmers_open.
 * HPGQ_E_INVALID before any device call. */
int  hpgq_clip_open(hpgq_clip_t **cl, int device, const char *const *probes, int nprobes,
                    int min_overlap, void *stream);
void hpgq_clip_close(hpgq_clip_t *cl);
/* positions only (async): pos_out[i] = c, probe_out[i] = the winner; device
 * pointers of num_reads elements; probe_out may be NULL */
int  hpgq_clip_find_device(hpgq_clip_t *cl, const hpgq_batch_t *in,
                           uint32_t *pos_out, uint8_t *probe_out);
/* find, then the kept reads back to back into the CALLER's device buffers
 * (async): seq_out / qual_out hold at least the input's bytes, idx_out
 * num_reads + 1 offsets from 0; pos_out / probe_out may be NULL.  Nothing is
 * written behind idx_out[num_reads] bytes of either output. */
int  hpgq_clip_device(hpgq_clip_t *cl, const hpgq_batch_t *in, char *seq_out, char *qual_out,
                      int32_t *idx_out, uint32_t *pos_out, uint8_t *probe_out);
/* The same into buffers the handle owns (grown as needed, HPGQ_DEVICE_SLACK
 * readable bytes behind the data).  *out is valid until the next
 * hpgq_clip_batch_device on this handle or its close; in and out may be the
 * same struct.  Waits for the stream once (the input's size is on the device);
 * the clip itself is async. */
int  hpgq_clip_batch_device(hpgq_clip_t *cl, const hpgq_batch_t *in, hpgq_batch_t *out);
int  hpgq_clip_sync(hpgq_clip_t *cl);
/* zero the scalars (async); the probes stay */
int  hpgq_clip_reset(hpgq_clip_t *cl);
/* the scalars since open or reset.  Synchronises. */
int  hpgq_clip_read(hpgq_clip_t *cl, hpgq_clip_info_t *info);
/* Tests only: at most max_wg workgroups per kernel (0, the default: no limit). */
int  hpgq_clip_debug_set_max_workgroups(hpgq_clip_t *cl, int max_wg);
/* Host only, no device (csrc/hpgq_clip_post.cpp): the rule above on one read.
 * Returns c (n: no match) and sets *probe (may be NULL) to the winner or -1;
 * -2 for a set or a min_overlap that breaks the rules. */
int64_t hpgq_clip_find(const void *s, size_t n, const char *const *probes, int nprobes,
                       int min_overlap, int *probe);

/* ---------------------------------------------------------------------- */
/* edit --clip-overlap: cut paired reads at the insert end                  */
/* ---------------------------------------------------------------------- */

/*
 * Build-defined.  A pair is mate 1 s1[0, n1) and mate 2
 * s2[0, n2); comp maps A<->T and C<->G, upper case only.  min_overlap is
 * 8 .. HPGQ_OVL_MAX_LEN, max_mismatches M is 0 .. 255 and below min_overlap.
 * A pair with a mate longer than HPGQ_OVL_MAX_LEN is skipped: result -1,
 * nothing cut.  For a candidate insert length F, lo = max(0, F - n2),
 * hi = min(n1, F), ov(F) = hi - lo, and for k in [lo, hi) byte s1[k] faces
 * s2[F - 1 - k]; mism(F) counts the k for which it is not true that both bytes
 * are one of A C G T and s2[F - 1 - k] == comp(s1[k]) (N, lower case and every
 * other byte value mismatch, also against themselves).  F is admissible iff
 * ov(F) >= min_overlap and mism(F) <= M; F* is the greatest admissible F, 0 if
 * there is none.  With F* > 0 mate 1 keeps min(n1, F*) bytes of sequence and
 * quality and mate 2 min(n2, F*); otherwise both keep everything.  Nothing
 * behind a read's last byte counts.  The scalars are plain u64 sums over every
 * batch since open or reset.
 *
 * Input as hpgq_clip_device, two batches of the same num_reads.  The inputs
 * are never written.  Everything runs on the handle's stream.
 */
#define HPGQ_OVL_MAX_LEN 512
typedef struct hpgq_ovl hpgq_ovl_t;
typedef struct hpgq_ovl_info {
  uint64_t pairs, skipped, overlapping, clipped, bases_removed[2];
  int32_t min_overlap, max_mismatches;
} hpgq_ovl_info_t;

/* stream: as hpgq_kmers_open.  HPGQ_E_INVALID before any device call. */
int  hpgq_ovl_open(hpgq_ovl_t **ov, int device, int min_overlap, int max_mismatches, void *stream);
void hpgq_ovl_close(hpgq_ovl_t *ov);
/* results only (async): insert_out[i] = F*, 0 or -1 (int32), pos1_out[i] /
 * pos2_out[i] = the bytes mate 1 / mate 2 keeps (uint32); device pointers of
 * num_reads elements, each may be NULL */
int  hpgq_ovl_find_device(hpgq_ovl_t *ov, const hpgq_batch_t *m1, const hpgq_batch_t *m2,
                          int32_t *insert_out, uint32_t *pos1_out, uint32_t *pos2_out);
/* find, then both mates' kept reads back to back into buffers the handle owns
 * (the contract of hpgq_clip_batch_device: valid until the next call on this
 * handle or its close; out1 / out2 may be m1 / m2; waits for the stream for
 * the inputs' sizes, the cut itself is async) */
int  hpgq_ovl_batch_device(hpgq_ovl_t *ov, const hpgq_batch_t *m1, const hpgq_batch_t *m2,
                           hpgq_batch_t *out1, hpgq_batch_t *out2);
int  hpgq_ovl_sync(hpgq_ovl_t *ov);
/* zero the scalars (async); the parameters stay */
int  hpgq_ovl_reset(hpgq_ovl_t *ov);
/* the scalars since open or reset.  Synchronises. */
int  hpgq_ovl_read(hpgq_ovl_t *ov, hpgq_ovl_info_t *info);
/* Tests only: at most max_wg workgroups per kernel (0, the default: no limit). */
int  hpgq_ovl_debug_set_max_workgroups(hpgq_ovl_t *ov, int max_wg);
/* Host only, no device (csrc/hpgq_ovl_post.cpp): the rule above on one pair.
 * Returns F*, 0, -1 (skipped) or -2 (parameters that break the rules, or a
 * NULL mate with bytes). */
int64_t hpgq_ovl_find(const void *s1, size_t n1, const void *s2, size_t n2, int min_overlap,
                      int max_mismatches);

/*
 * edit --correct-overlap and --insert-size (build-defined).
 * Both are switches of an ovl handle, off after hpgq_ovl_open; while both are
 * off the handle allocates and launches nothing for them.
 *
 * Correction.  Q1, Q2 are the mates' quality bytes (unsigned, 0 .. 255), phred
 * is 0 .. 255 as for hpgq_open, 0 <= low < high <= 93.  With F = F* > 0 and k
 * in [lo, hi), j = F - 1 - k, q1 = (int)Q1[k] - phred, q2 = (int)Q2[j] - phred:
 * at a position that does not match (the rule above),
 *   1. if s1[k] is one of A C G T, q1 >= high and q2 <= low:
 *      s2[j] := comp(s1[k]), Q2[j] := Q1[k]  (one corrected base of mate 2);
 *   2. else if s2[j] is one of A C G T, q2 >= high and q1 <= low:
 *      s1[k] := comp(s2[j]), Q1[k] := Q2[j]  (one corrected base of mate 1);
 *   3. else nothing.
 * F*, the cuts and the scalars of hpgq_ovl_info_t come from the uncorrected
 * bytes; every facing position lies inside the kept reads, which are what
 * hpgq_ovl_batch_device corrects, after the cut, in the handle's buffers.  The
 * inputs are never written, hpgq_ovl_find_device never corrects.
 *
 * Insert sizes.  hist[F*] counts every analysed pair of every find pass
 * (hpgq_ovl_find_device and hpgq_ovl_batch_device) while counting is on: bin 0
 * the pairs without an admissible F, skipped pairs in no bin.
 */
#define HPGQ_OVL_INSERT_BINS 1025   /* F* <= 2 HPGQ_OVL_MAX_LEN - 8 */
typedef struct hpgq_ovl_correct_info {
  uint64_t corrected_pairs, corrected_bases[2];   /* pairs with a corrected base; bases per mate */
  int32_t on, phred, high, low;
} hpgq_ovl_correct_info_t;
/* on != 0: hpgq_ovl_batch_device corrects from now on, with these parameters
 * (HPGQ_E_INVALID for ones that break the rules, before any device call);
 * on == 0: it does not, and the parameters given are ignored.  Between any two
 * calls on the handle. */
int  hpgq_ovl_set_correct(hpgq_ovl_t *ov, int on, int phred, int high, int low);
/* on != 0: every find pass counts its F* from now on */
int  hpgq_ovl_count_inserts(hpgq_ovl_t *ov, int on);
/* the correction's scalars since open or reset (hpgq_ovl_reset zeroes them and
 * the histogram; the switches and parameters stay).  Synchronises. */
int  hpgq_ovl_read_correct(hpgq_ovl_t *ov, hpgq_ovl_correct_info_t *info);
/* the histogram since open or reset, all zeros if counting was never on.  Synchronises. */
int  hpgq_ovl_read_inserts(hpgq_ovl_t *ov, uint64_t hist[HPGQ_OVL_INSERT_BINS]);
/* *inserts: the DEVICE array of the F* (int32, num_reads of them) that the last
 * hpgq_ovl_batch_device found, kept while either switch was on during that
 * call; NULL otherwise, and after hpgq_ovl_find_device.  Valid until the next
 * call on the handle; written on its stream.  For a consumer that assembles its
 * output from text of its own: with these and hpgq_ovl_correct it applies the
 * same correction there. */
int  hpgq_ovl_last_inserts(hpgq_ovl_t *ov, const int32_t **inserts);
/* Host only, no device (csrc/hpgq_ovl_post.cpp): the correction above, in
 * place, on one pair whose F* is F.  Returns the bases changed and sets
 * changed[0] / changed[1] (may be NULL) to those of mate 1 / mate 2; 0 and
 * nothing changed for F <= 0; -2 for parameters that break the rules, a NULL
 * array with bytes, or an F > 0 that the rule above cannot return for these
 * lengths (a mate longer than HPGQ_OVL_MAX_LEN, fewer than 8 facing bytes). */
int64_t hpgq_ovl_correct(void *s1, void *q1, size_t n1, void *s2, void *q2, size_t n2, int64_t F,
                         int phred, int high, int low, uint32_t changed[2]);

/*
 * edit --merge-overlap (build-defined): a pair with F = F* > 0
 * becomes one read m[0, F), QM[0, F); every other pair passes through uncut
 * and unchanged.  rc(b) is comp(b) for A C G T and b itself for every other
 * byte.  With lo, hi as above and j = F - 1 - p:
 *   p <  lo: m[p] = s1[p],      QM[p] = Q1[p];
 *   p >= hi: m[p] = rc(s2[j]),  QM[p] = Q2[j];
 *   lo <= p < hi (a facing position):
 *     1. a match (the rule above): m[p] = s1[p], QM[p] = max(Q1[p], Q2[j]);
 *     2. else, with a1 / a2 = "s1[p] / s2[j] is one of A C G T", mate 2 wins iff
 *        a2 && (!a1 || Q2[j] > Q1[p]) (unsigned bytes, a tie goes to mate 1):
 *        m[p] = comp(s2[j]), QM[p] = Q2[j], one base resolved by mate 2;
 *     3. else m[p] = s1[p], QM[p] = Q1[p], one base resolved by mate 1.
 * The merge reads the inputs: it never corrects, never counts §2.14's scalars
 * and ignores the correction switch (merging a corrected pair gives the same
 * bytes).  The find pass of a merge call counts §2.13's scalars and, while
 * counting is on, the histogram, as hpgq_ovl_batch_device's does.
 */
typedef struct hpgq_ovl_merge_info {
  uint64_t merged_pairs, merged_bases, resolved[2];   /* pairs with F* > 0; the sum of their F*; bases per winning mate */
} hpgq_ovl_merge_info_t;
/* find, then three compacted batches in buffers the handle owns (the contract
 * of hpgq_ovl_batch_device): out1 / out2 the pairs that do not merge, uncut,
 * in input order; merged the merged reads in input order.  out1 / out2 may be
 * m1 / m2; the inputs are never written.  hpgq_ovl_last_inserts is valid after
 * this call whatever the switches: pair i merged iff F*[i] > 0.  Waits for the
 * stream three times, once more than hpgq_ovl_batch_device: for each input's
 * size, and for the number of merged pairs.
 * HPGQ_E_INVALID before any device work for the argument errors of
 * hpgq_ovl_batch_device and a NULL merged; for inputs of more than INT32_MAX
 * bytes together (the merged offsets are int32) after the two waits that
 * fetch the inputs' sizes, before anything is allocated or launched. */
int  hpgq_ovl_merge_device(hpgq_ovl_t *ov, const hpgq_batch_t *m1, const hpgq_batch_t *m2,
                           hpgq_batch_t *out1, hpgq_batch_t *out2, hpgq_batch_t *merged);
/* the merge's scalars since open or reset (hpgq_ovl_reset zeroes them).  Synchronises. */
int  hpgq_ovl_read_merge(hpgq_ovl_t *ov, hpgq_ovl_merge_info_t *info);
/* Host only, no device (csrc/hpgq_ovl_post.cpp): the merged read of one pair
 * whose F* is F, F bytes each into seq_out and qual_out.  Returns F and sets
 * resolved[0] / resolved[1] (may be NULL) to the bases mate 1 / mate 2 won; 0
 * and nothing written for F <= 0; -2 for a NULL array with bytes or an F > 0
 * that the rule above cannot return for these lengths. */
int64_t hpgq_ovl_merge(const void *s1, const void *q1, size_t n1, const void *s2, const void *q2, size_t n2,
                       int64_t F, void *seq_out, void *qual_out, uint32_t resolved[2]);

/* ---------------------------------------------------------------------- */
/* FASTQ text -> device batch (the parsing half of the producer's          */
/* fastq_fread_se, src/stats_fastq.c:183, moved onto the GPU)              */
/* ---------------------------------------------------------------------- */

/*
 * Records are 4 lines: "@header", sequence, "+[header]", quality (as long as
 * the sequence); "\n" or "\r\n" line ends.  A parse unit is whole records,
 * the last one ending in a newline.
 */
typedef struct hpgq_parser hpgq_parser_t;

/* Bytes of buf[0, n) that form whole records; the rest starts the next unit.
 * at_eof: the data ends at n (returns n; the caller appends a final newline
 * when the file lacks one).  0: no complete record yet.  Host-only. */
int64_t hpgq_fastq_complete_prefix(const char *buf, int64_t n, int at_eof);

/* stream: the stream to parse on (e.g. hpgq_stream(ctx), so the engine runs
 * after it), or NULL for a stream of its own */
int  hpgq_parser_open(hpgq_parser_t **ps, int device, void *stream);
void hpgq_parser_close(hpgq_parser_t *ps);
/* Parse text[0, n) (n < 2^31) into a device batch owned by the parser, valid
 * until its next parse; `out` gets device pointers and num_reads.  _host
 * copies the text to the device first.  HPGQ_E_FORMAT on malformed records. */
int  hpgq_parse_host(hpgq_parser_t *ps, const char *text, int64_t n, hpgq_batch_t *out);
int  hpgq_parse_device(hpgq_parser_t *ps, const char *text_dev, int64_t n, hpgq_batch_t *out);
/* offsets into the last parsed text, num_reads u32 each (any may be NULL):
 * record start ('@'), sequence, '+' line, quality */
int  hpgq_parse_records(hpgq_parser_t *ps, uint32_t *rec_start, uint32_t *seq_start,
                        uint32_t *plus_start, uint32_t *qual_start);
void *hpgq_parser_stream(hpgq_parser_t *ps);
/* the longest record of the last parse (0 when empty): the engine's and the
 * k-mer counter's hpgq_*reserve_length before they run the batch */
int64_t hpgq_parser_max_length(hpgq_parser_t *ps);

/*
 * Mate pairs.  Pair i is record i of two texts, or records 2i
 * and 2i+1 of one interleaved text; the mates may differ in length.
 *
 * The mate name of a record is its header line's bytes after '@' up to, not
 * including, the first space, tab, CR or LF.  If mate 1's name ends in "/1"
 * and mate 2's in "/2" those two bytes are dropped from both (no other suffix
 * pair is).  A pair is in step iff the two names then have the same length and
 * bytes; two empty names are equal.
 */

/* Host only, HIP-free (csrc/hpgq_fastq_text.c).  A record is four
 * '\n'-terminated lines counted from buf[0], which is a record start: the byte
 * length of the first min(max_records, whole records present) records, their
 * number in *records (may be NULL).  Nothing is validated: the GPU parser
 * does that. */
int64_t hpgq_fastq_record_prefix(const char *buf, int64_t n, int64_t max_records, int64_t *records);
/* '\n' bytes in buf[0, n): the lines a reader's piece ends (host only) */
int64_t hpgq_fastq_count_lines(const char *buf, int64_t n);

/* Interleaved text: record 2i becomes read i of out1, record 2i+1 read i of
 * out2, each with contiguous seq / quality of its own, data_indices starting
 * at 0 and HPGQ_DEVICE_SLACK readable bytes past its end; both owned by the
 * parser until its next parse.  One parse: the per-record lengths are scanned
 * over the even and over the odd records and one copy pass routes each record
 * to its mate.  An odd record count is HPGQ_E_PAIRING.  hpgq_parse_records then
 * returns all 2 num_reads records in text order; hpgq_parser_max_length is the
 * maximum over both mates. */
int  hpgq_parse_host_interleaved(hpgq_parser_t *ps, const char *text, int64_t n, hpgq_batch_t *out1, hpgq_batch_t *out2);
int  hpgq_parse_device_interleaved(hpgq_parser_t *ps, const char *text_dev, int64_t n, hpgq_batch_t *out1, hpgq_batch_t *out2);
/* The mate-name rule over the last parses of ps1 and ps2 (record i of each),
 * or with ps2 NULL over records 2i / 2i+1 of ps1's last, interleaved, parse
 * (HPGQ_E_STATE when it was not).  HPGQ_OK with *first_bad = -1, or
 * HPGQ_E_PAIRING with the lowest pair whose names differ, or min(n1, n2) when
 * the names up to there agree and the record counts differ.  Both parsers
 * are on one device, and the texts of their last parses must still be valid
 * (the device text of hpgq_parse_device*; hpgq_parse_host* keeps its own copy
 * until the next parse), as device batches must for hpgq_sync.  Runs on ps1's
 * stream after waiting for ps2's, and synchronises it, as the parses do. */
int  hpgq_parse_pair_check(hpgq_parser_t *ps1, hpgq_parser_t *ps2, int64_t *first_bad);
/* Tests only: at most max_wg workgroups for the de-interleaving copy and the
 * name check (0, the default: no limit), so that a small text gives every
 * workgroup several iterations. */
int  hpgq_parser_debug_set_max_workgroups(hpgq_parser_t *ps, int max_wg);

/* ---------------------------------------------------------------------- */
/* synthetic input (bench / tests): counter-based, identical on host & GPU */
/* ---------------------------------------------------------------------- */

typedef struct hpgq_synth {
  uint64_t seed;
  int32_t  read_length;      /* L                                            */
  int32_t  trunc_pct;        /* % of reads truncated to U[20, L]            */
  int32_t  bad_pct;          /* % of reads with Q centred at 12             */
  int32_t  n_per_1024;       /* 'N' probability x 1024                      */
  int32_t  phred;            /* quality offset                              */
  int32_t  mate;             /* 0 or 1 (mate 2 reuses mate 1's lengths)     */
} hpgq_synth_t;

/* read length of read `idx` (host, no device needed) */
int32_t hpgq_synth_length(const hpgq_synth_t *s, int64_t idx);
/* data_indices (n+1 entries, starting at 0) of reads [first, first+n) */
int  hpgq_synth_indices_host(const hpgq_synth_t *s, int64_t first, int64_t n, int32_t *idx_host);
/* Fill seq/quality of reads [first, first+n) on the device; idx_dev must
 * already hold hpgq_synth_indices_host()'s output. Async on `stream`. */
int  hpgq_synth_device(const hpgq_synth_t *s, int64_t first, int64_t n,
                       char *seq_dev, char *qual_dev, const int32_t *idx_dev, void *stream);

/* number of visible HIP devices (0 when none or the runtime fails) */
int  hpgq_device_count(void);
/* NUMA node of HIP device `device` (its PCI function's numa_node in sysfs),
 * -1 when unknown: host threads and buffers that feed it belong there */
int  hpgq_device_numa_node(int device);

const char *hpgq_strerror(int code);
const char *hpgq_version(void);
/* the first engine kernel instance of a ctx's chain (for profiles / bench
 * reports) and the whole chain ("first -> follow-up -> ..."); DESIGN.md §4.0 */
const char *hpgq_kernel_name(const hpgq_ctx_t *ctx);
const char *hpgq_kernel_chain(const hpgq_ctx_t *ctx);

/* memory helpers for HIP-free hosts (the C CLI): page-locked host buffers
 * (fast, asynchronous H2D), device buffers, and a device -> host copy queued
 * on a ctx stream (complete after hpgq_sync) */
int  hpgq_host_alloc(void **ptr, size_t bytes);
void hpgq_host_free(void *ptr);
int  hpgq_device_alloc(int device, void **ptr, size_t bytes);
void hpgq_device_free(void *ptr);
int  hpgq_copy_to_host(hpgq_ctx_t *ctx, void *dst, const void *src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* HPGQ_H */
