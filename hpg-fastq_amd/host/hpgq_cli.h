/*
 * hpgq_cli.h — the C host side of hpg-fastq on libhpgq (stats | filter | edit).
 *
 * Mirrors the reference's command line (src/hpg-fastq.c; options
 * src/stats_options.c:260-300, src/filter_options.c:235-258,
 * src/edit_options.c:267-290), its producer -> worker -> consumer pipeline
 * (src/stats_fastq.c:174-250, src/filter_fastq.c:106-174,
 * src/edit_fastq.c:113-206) and its outputs (passed.fq / failed.fq,
 * edit.fq, <in>.summary.txt + data files, src/stats_report.c), with the
 * worker's bioinfo-libs calls replaced by the libhpgq C-ABI (include/hpgq.h)
 * and the reader's parsing moved onto the GPU (hpgq_parse_*).
 */
#ifndef HPGQ_CLI_H
#define HPGQ_CLI_H

#include <stddef.h>
#include <stdint.h>

#include "hpgq.h"

enum { CMD_STATS = 0, CMD_FILTER = 1, CMD_EDIT = 2 };
#define CLI_ADAPTER_NAME_MAX 64   /* bytes of an adapter's name in --adapter-file */

typedef struct {
  int command;
  const char *command_name;
  const char *exec_name;
  char *in_filename;        /* -f, or --fq1 */
  char *in_filename2;       /* --fq2 (NULL: one input) */
  int interleaved;          /* --interleaved: the mates alternate in -f */
  int paired;               /* two mates per pair, either way */
  char *out_dirname;
  int num_threads;          /* reader threads */
  int batch_size;           /* accepted for compatibility; chunks are sized in bytes */
  char *quality_encoding_name;
  int quality_encoding_value;
  int kmers_on;
  int quality_dist_on;      /* stats --quality-dist */
  int duplication_on;       /* stats --duplication */
  int overrep_on;           /* stats --overrepresented */
  uint64_t overrep_min_count;   /* K: the merged count a listed sequence has at least */
  int overrep_top;          /* N: sequences listed at most */
  uint64_t overrep_bytes;   /* the arena of every worker's table */
  int adapters_on;          /* stats --adapters */
  char *adapter_file;       /* --adapter-file: replaces the default set */
  int adapter_n;            /* the probe set in order (cli_adapters_load): 1 .. HPGQ_ADAPT_MAX_PROBES */
  char adapter_names[HPGQ_ADAPT_MAX_PROBES][CLI_ADAPTER_NAME_MAX + 1];
  char adapter_probes[HPGQ_ADAPT_MAX_PROBES][HPGQ_ADAPT_MAX_LEN + 1];
  int clip_on;              /* edit --clip-adapters: the set above, from --clip-adapter-file or the default */
  int clip_min_overlap;     /* --clip-min-overlap: 1 .. HPGQ_ADAPT_MAX_LEN */
  int ovl_on;               /* edit --clip-overlap: paired input only */
  int ovl_min_overlap;      /* --clip-overlap-min: 8 .. HPGQ_OVL_MAX_LEN */
  int ovl_max_mismatches;   /* --clip-overlap-mismatches: 0 .. 255, below the minimum overlap */
  int ovl_fix_on;           /* --correct-overlap: needs --clip-overlap */
  int ovl_fix_high;         /* --correct-overlap-high: 1 .. 93 */
  int ovl_fix_low;          /* --correct-overlap-low: 0 .. 92, below the high quality */
  int ovl_insert_on;        /* --insert-size (§2.14): needs --clip-overlap */
  int ovl_merge_on;         /* --merge-overlap (§2.15): needs --clip-overlap, excludes --correct-overlap */
  /* chaos game (old/main_hpg_fastq_old.c:185-189: --cg | --chaos-game, --k, --gs-filename) */
  int cg_on, k_cg;
  char *gs_filename;
  /* filter / trim options, NO_VALUE (-1) when unset (src/stats_options.c:18-40) */
  char *read_length_range, *read_quality_range, *left_quality_range, *right_quality_range;
  int min_read_length, max_read_length, min_read_quality, max_read_quality;
  int left_length, min_left_quality, max_left_quality;
  int right_length, min_right_quality, max_right_quality;
  int max_N, max_out_of_quality;
  int filter_on;
  /* MI355X build options */
  int device;               /* first GPU */
  int num_gpus;             /* devices (0: every visible one) */
  int gpu_workers;          /* worker threads per device (2: copy-in beside compute) */
  int64_t cg_batch_size;    /* --cg: FASTQ text bytes per chaos-game call */
  int lmax;                 /* per-position arrays (longest read kept) */
  int chunk_mb;             /* FASTQ text per parse unit */
  int print_params;         /* print hpgq_params_t and exit (no device) */
  char *counters_out;       /* raw u64 counter dump (tests) */
  char *kmers_out;          /* raw u64 k-mer table dump (tests) */
  char *cg_out;             /* raw u32 chaos-game tables dump (tests) */
  char *quality_dist_out;   /* raw [npos u64 | hist] per mate dump (tests) */
  char *duplication_out;    /* raw [n u64 | keys ascending | counts] per mate dump (tests) */
  char *adapters_out;       /* raw [nprobes | npos | reads | with_any | first] u64 per mate dump (tests) */
  int quiet;
  int stream_writer;        /* filter / edit: one writer thread instead of mapped outputs */
  int writer_hook;          /* tests only (--writer-test-hook): hpgq_mapout.h MAPOUT_HOOK_* */
  int copy_threads;         /* mapped writer: copier threads (0: --num-threads) */
  int prefault_threads;     /* mapped writer: prefault threads (-1: default, none past the first window) */
} cli_options_t;

/* parse + validate (exits with the reference's messages on errors) */
cli_options_t *cli_parse(int command, const char *exec_name, int argc, char **argv);
void cli_display(const cli_options_t *o);
void cli_free(cli_options_t *o);
/* NO_VALUE -> MIN/MAX defaults and the libhpgq params (src/filter_fastq.c:195-206) */
void cli_params(const cli_options_t *o, hpgq_params_t *p);
void cli_print_params(const hpgq_params_t *p);
/* src/commons_fastq.c:31-103 */
int cli_parse_range(int *min, int *max, const char *range, const char *msg);

/* pipeline: returns 0 or a negative HPGQ_E* code */
typedef struct {
  uint64_t *counters;       /* the merged counter set(s) at full length (malloc'd) */
  int lmax;                 /* their layout's lmax: max(--lmax, longest merged read) */
  uint64_t num_reads, num_passed, num_failed, num_edited;
  double seconds, fastq_bytes;
  uint64_t *kmers;          /* --kmers: by_pos [HPGQ_NUM_KMERS][kmers_npos] (malloc'd) */
  int kmers_npos;
  uint64_t *qdist[2];       /* --quality-dist: per mate hist [qdist_npos][HPGQ_QDIST_VALUES] (malloc'd) */
  int qdist_npos[2];        /* the longest counted read of the mate */
  int dup_on;               /* --duplication: dup_levels[] hold the mates' levels */
  hpgq_dup_levels_t dup_levels[2];
  uint64_t *dup_keys[2], *dup_counts[2];   /* --duplication-out: keys ascending, counts in key order (malloc'd) */
  size_t dup_n[2];
  /* --overrepresented: per mate the listed sequences, count descending (all malloc'd);
   * overrep_reads[] the merged table's total */
  int overrep_on;
  int overrep_error;        /* 1: a worker's arena was too small, 2: no table kept a listed sequence */
  size_t overrep_n[2];
  uint64_t *overrep_counts[2], *overrep_lens[2];
  unsigned char **overrep_seqs[2];
  uint64_t overrep_reads[2];
  /* --adapters: per mate first [adapter_n][adapt_npos] (malloc'd), the counted
   * reads and those with at least one probe */
  uint64_t *adapt[2];
  int adapt_npos[2];
  uint64_t adapt_reads[2], adapt_with_any[2];
  int clip_on;              /* --clip-adapters: clip[] hold the mates' scalars, the workers' added */
  hpgq_clip_info_t clip[2];
  int ovl_on;               /* --clip-overlap: ovl holds the pairs' scalars, the workers' added */
  hpgq_ovl_info_t ovl;
  int ovl_fix_on;           /* --correct-overlap: ovl_fix holds the correction's scalars, the workers' added */
  hpgq_ovl_correct_info_t ovl_fix;
  int ovl_insert_on;        /* --insert-size: ovl_inserts holds the histogram, the workers' added */
  uint64_t ovl_inserts[HPGQ_OVL_INSERT_BINS];
  int ovl_merge_on;         /* --merge-overlap: ovl_merge holds the merge's scalars, the workers' added; the merged
                             * reads that passed / failed the filter come from the workers' single-end ctxs */
  hpgq_ovl_merge_info_t ovl_merge;
  uint64_t merged_passed, merged_failed;
  uint32_t *cg_seq, *cg_q;  /* --cg: table_seq / table_q [dim*dim] (malloc'd) */
  uint32_t cg_words;        /* fq_word_count */
  int cg_exact_calls;       /* chaos-game calls the exact simulation redid */
  int num_gpus;             /* GPU worker threads that ran */
  int writer;               /* filter / edit outputs: 1 mapped files (parallel copy), 2 stream writer */
  /* HPGQ_E_PAIRING: the first pair out of step, counted over the whole input
   * (-1: not known), and what the error line says after it */
  int64_t bad_pair;
  char pairing_msg[512];
} cli_result_t;

int cli_run(const cli_options_t *o, const hpgq_params_t *p, cli_result_t *res);

/* src/stats_report.c: summary + data files (+ k-mer files when res->kmers)
 * from res->counters, named after the input's base name */
int cli_report(const cli_options_t *o, const hpgq_params_t *p, const cli_result_t *res);
/* the same from one counter set (layout of res->lmax) under `base`: paired
 * input writes one report set per mate */
int cli_report_set(const cli_options_t *o, const hpgq_params_t *p, const cli_result_t *res,
                   const uint64_t *counters, const char *base);
/* --quality-dist: <base>.quality.dist.per.nt.data from one mate's table */
int cli_report_qdist(const cli_options_t *o, const hpgq_params_t *p, const uint64_t *hist, int npos,
                     const char *base);
/* --duplication: <base>.duplication.data from one mate's levels */
int cli_report_dup(const cli_options_t *o, const hpgq_dup_levels_t *lv, const char *base);
/* --overrepresented: <base>.overrepresented.data, n sequences in rank order */
int cli_report_overrep(const cli_options_t *o, size_t n, const uint64_t *counts, const uint64_t *lens,
                       unsigned char *const *seqs, uint64_t reads, const char *base);
/* --adapters / --clip-adapters: the probe set into o->adapter_n / _names /
 * _probes, from --adapter-file / --clip-adapter-file or the default set; on a
 * violation one line on stderr and -1.  No device. */
int cli_adapters_load(cli_options_t *o);
/* --adapters: <base>.adapter.content.data from one mate's table first[nprobes][npos] */
int cli_report_adapt(const cli_options_t *o, int nprobes, const char *const *names, const uint64_t *first, int npos,
                     uint64_t reads, uint64_t with_any, const char *base);
/* --clip-adapters: <base>.adapter.clip.data from one mate's scalars */
int cli_report_clip(const cli_options_t *o, int nprobes, const char *const *names, const hpgq_clip_info_t *info,
                    const char *base);
/* --clip-overlap: <base>.overlap.clip.data from the pairs' scalars (base: mate 1's report base) */
int cli_report_ovl(const cli_options_t *o, const hpgq_ovl_info_t *info, const char *base);
/* --correct-overlap: <base>.overlap.correct.data from the pairs' and the correction's scalars */
int cli_report_ovl_correct(const cli_options_t *o, const hpgq_ovl_info_t *info, const hpgq_ovl_correct_info_t *fix,
                           const char *base);
/* --merge-overlap: <base>.overlap.merge.data from the pairs' and the merge's scalars */
int cli_report_merge(const cli_options_t *o, const hpgq_ovl_info_t *info, const hpgq_ovl_merge_info_t *merge,
                     const char *base);
/* --insert-size: <base>.insert.size.data from the pairs' scalars and the histogram */
int cli_report_insert(const cli_options_t *o, const hpgq_ovl_info_t *info, const uint64_t hist[HPGQ_OVL_INSERT_BINS],
                      const char *base);
const char *cli_base_name(const char *path);
/* the report base names of the two mates: each input's base name, or
 * <base>_1 / <base>_2 for --interleaved (out: 2 x 4096 bytes) */
void cli_mate_names(const cli_options_t *o, char out[2][4096]);

/* `hpg-fastq signature` (hpgq_signature.c): FASTA -> genomic-signature file;
 * argv[0] is the command name.  Returns the process exit code. */
int cli_signature(const char *exec_name, int argc, char **argv);

#endif
