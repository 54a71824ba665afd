/*
 * hpg_fastq.c — `hpg-fastq stats | filter | edit | signature` on MI355X (libhpgq).
 *
 * Command dispatch and result printing after src/hpg-fastq.c and the
 * stats_fastq / filter_fastq / edit_fastq drivers (src/stats_fastq.c:424-500,
 * src/filter_fastq.c:180-250, src/edit_fastq.c:236-300).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq_cli.h"

static void usage(const char *exec_name) {
  printf("Program: %s (High-performance tools for handling FastQ files, MI355X build)\n", exec_name);
  printf("Version: 1.0.0 (%s)\n", hpgq_version());
  printf("\n");
  printf("Usage: %s <command> [options]\n", exec_name);
  printf("\n");
  printf("Command: stats\t\tstatistics summary\n");
  printf("         filter\t\tfilter a FastQ file by using advanced criteria\n");
  printf("         edit\t\tedit a FastQ file according the specified options\n");
  printf("         signature\tgenomic signature (--gs-filename file) of a FASTA reference\n");
  printf("\n");
  printf("For more information about a certain command, type %s <command> --help\n", exec_name);
  exit(-1);
}

int main(int argc, char **argv) {
  const char *exec_name = argv[0];
  if (argc == 1 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) usage(exec_name);
  if (!strcmp(argv[1], "signature")) return cli_signature(exec_name, argc - 1, argv + 1);
  int cmd;
  if (!strcmp(argv[1], "stats")) cmd = CMD_STATS;
  else if (!strcmp(argv[1], "filter")) cmd = CMD_FILTER;
  else if (!strcmp(argv[1], "edit")) cmd = CMD_EDIT;
  else usage(exec_name);
  cli_options_t *o = cli_parse(cmd, exec_name, argc - 1, argv + 1);
  hpgq_params_t p;
  cli_params(o, &p);
  if ((o->adapters_on || o->clip_on) && cli_adapters_load(o)) {   /* (one line on stderr; before any GPU work) */
    cli_free(o);
    return 1;
  }
  if (o->print_params) {
    cli_print_params(&p);
    cli_free(o);
    return 0;
  }
  if (!o->quiet) cli_display(o);

  cli_result_t r;
  int rc = cli_run(o, &p, &r);
  if (rc && r.overrep_error) {   /* one line each */
    if (r.overrep_error == 1)
      fprintf(stderr,
              "hpg-fastq: --overrepresented: the sequences that reached the minimum count need more than %lu bytes; "
              "raise --overrepresented-min-count or --overrepresented-bytes\n", (unsigned long)o->overrep_bytes);
    else
      fprintf(stderr, "hpg-fastq: --overrepresented: internal error: no table kept a listed sequence\n");
    free(r.counters);
    cli_free(o);
    return 1;
  }
  if (rc) {
    /* one line with the first bad pair (0-based, over the whole input), and the two names of a mismatch */
    if (rc == HPGQ_E_PAIRING && r.pairing_msg[0]) fprintf(stderr, "hpg-fastq: pairing error at %s\n", r.pairing_msg);
    fprintf(stderr, "\nError: %s (%d)\n", hpgq_strerror(rc), rc);
    free(r.counters);
    cli_free(o);
    return 1;
  }
  /* (the full-length set: layout of r.lmax = max(--lmax, longest merged read)) */
  const uint64_t *counters = r.counters;
  const size_t clen = hpgq_counters_len(r.lmax) * (p.paired ? 2 : 1);
  if (o->counters_out) {
    FILE *f = fopen(o->counters_out, "wb");
    if (!f || fwrite(counters, sizeof(uint64_t), clen, f) != clen) rc = 1;
    if (f) fclose(f);
  }
  if (o->kmers_out && r.kmers) {
    const size_t kn = (size_t)HPGQ_NUM_KMERS * (size_t)r.kmers_npos;
    FILE *f = fopen(o->kmers_out, "wb");
    if (!f || fwrite(r.kmers, sizeof(uint64_t), kn, f) != kn) rc = 1;
    if (f) fclose(f);
  }
  if (o->quality_dist_out && r.qdist[0]) {   /* per mate: [npos u64 | hist u64 [npos][256]] */
    FILE *f = fopen(o->quality_dist_out, "wb");
    for (int m = 0; m < (p.paired ? 2 : 1); ++m) {
      const uint64_t np = (uint64_t)r.qdist_npos[m];
      const size_t qn = (size_t)HPGQ_QDIST_VALUES * (size_t)np;
      if (!f || fwrite(&np, sizeof(uint64_t), 1, f) != 1 || fwrite(r.qdist[m], sizeof(uint64_t), qn, f) != qn) rc = 1;
    }
    if (f) fclose(f);
  }
  if (o->duplication_out && r.dup_on) {   /* per mate: [n u64 | n keys ascending | n counts in key order] */
    FILE *f = fopen(o->duplication_out, "wb");
    for (int m = 0; m < (p.paired ? 2 : 1); ++m) {
      const uint64_t n = (uint64_t)r.dup_n[m];
      if (!f || fwrite(&n, sizeof(uint64_t), 1, f) != 1 || fwrite(r.dup_keys[m], sizeof(uint64_t), n, f) != n ||
          fwrite(r.dup_counts[m], sizeof(uint64_t), n, f) != n)
        rc = 1;
    }
    if (f) fclose(f);
  }
  if (o->adapters_out && r.adapt[0]) {   /* per mate: [nprobes | npos | reads | with_any | first [nprobes][npos]] u64 */
    FILE *f = fopen(o->adapters_out, "wb");
    for (int m = 0; m < (p.paired ? 2 : 1); ++m) {
      const uint64_t head[4] = {(uint64_t)o->adapter_n, (uint64_t)r.adapt_npos[m], r.adapt_reads[m], r.adapt_with_any[m]};
      const size_t an = (size_t)o->adapter_n * (size_t)r.adapt_npos[m];
      if (!f || fwrite(head, sizeof(uint64_t), 4, f) != 4 || fwrite(r.adapt[m], sizeof(uint64_t), an, f) != an) rc = 1;
    }
    if (f) fclose(f);
  }
  if (o->cg_out && r.cg_seq) {   /* [table_seq | table_q | word count] u32 */
    const size_t cells = (size_t)1 << (2 * o->k_cg);
    FILE *f = fopen(o->cg_out, "wb");
    if (!f || fwrite(r.cg_seq, 4, cells, f) != cells || fwrite(r.cg_q, 4, cells, f) != cells ||
        fwrite(&r.cg_words, 4, 1, f) != 1)
      rc = 1;
    if (f) fclose(f);
  }
  if (cmd == CMD_STATS && !p.paired && cli_report(o, &p, &r)) rc = 1;
  char mate_name[2][4096];
  if (p.paired) cli_mate_names(o, mate_name);
  /* paired input: one full report set per mate, from that mate's counter set */
  for (int m = 0; cmd == CMD_STATS && p.paired && m < 2; ++m)
    if (cli_report_set(o, &p, &r, counters + (size_t)m * hpgq_counters_len(r.lmax), mate_name[m])) rc = 1;
  /* --quality-dist: one file per mate, named as that mate's report set */
  for (int m = 0; cmd == CMD_STATS && m < (p.paired ? 2 : 1); ++m)
    if (r.qdist[m] &&
        cli_report_qdist(o, &p, r.qdist[m], r.qdist_npos[m], p.paired ? mate_name[m] : cli_base_name(o->in_filename)))
      rc = 1;
  /* --duplication: one file per mate, named as that mate's report set */
  for (int m = 0; cmd == CMD_STATS && r.dup_on && m < (p.paired ? 2 : 1); ++m)
    if (cli_report_dup(o, &r.dup_levels[m], p.paired ? mate_name[m] : cli_base_name(o->in_filename))) rc = 1;
  /* --overrepresented: one file per mate, named as that mate's report set */
  for (int m = 0; cmd == CMD_STATS && r.overrep_on && m < (p.paired ? 2 : 1); ++m)
    if (cli_report_overrep(o, r.overrep_n[m], r.overrep_counts[m], r.overrep_lens[m], r.overrep_seqs[m], r.overrep_reads[m],
                           p.paired ? mate_name[m] : cli_base_name(o->in_filename)))
      rc = 1;
  /* --adapters: one file per mate, named as that mate's report set */
  for (int m = 0; cmd == CMD_STATS && m < (p.paired ? 2 : 1); ++m) {
    const char *names[HPGQ_ADAPT_MAX_PROBES];
    for (int a = 0; a < o->adapter_n; ++a) names[a] = o->adapter_names[a];
    if (r.adapt[m] && cli_report_adapt(o, o->adapter_n, names, r.adapt[m], r.adapt_npos[m], r.adapt_reads[m],
                                       r.adapt_with_any[m], p.paired ? mate_name[m] : cli_base_name(o->in_filename)))
      rc = 1;
  }
  /* --clip-adapters: one file per mate, named as that mate's report set would be */
  for (int m = 0; r.clip_on && m < (p.paired ? 2 : 1); ++m) {
    const char *names[HPGQ_ADAPT_MAX_PROBES];
    for (int a = 0; a < o->adapter_n; ++a) names[a] = o->adapter_names[a];
    if (cli_report_clip(o, o->adapter_n, names, &r.clip[m], p.paired ? mate_name[m] : cli_base_name(o->in_filename))) rc = 1;
  }
  /* --clip-overlap: one file for the pairs, named as mate 1's report set would be */
  if (r.ovl_on && cli_report_ovl(o, &r.ovl, mate_name[0])) rc = 1;
  /* --correct-overlap and --insert-size: one file each, beside it */
  if (r.ovl_fix_on && cli_report_ovl_correct(o, &r.ovl, &r.ovl_fix, mate_name[0])) rc = 1;
  if (r.ovl_insert_on && cli_report_insert(o, &r.ovl, r.ovl_inserts, mate_name[0])) rc = 1;
  /* --merge-overlap: one more beside them */
  if (r.ovl_merge_on && cli_report_merge(o, &r.ovl, &r.ovl_merge, mate_name[0])) rc = 1;

  if (!o->quiet) {
    printf("\n\nRESULTS\n");
    printf("=================================================\n");
    if (cmd == CMD_STATS) {
      printf("Report files were stored in '%s' directory\n", o->out_dirname);
      if (p.paired) printf("\tMate 1: %s.*\n\tMate 2: %s.*\n", mate_name[0], mate_name[1]);
      if (p.filter_on) {
        printf("\nFiltering: enabled\n");
        printf("\tSo, statistics were computed for %lu of %lu reads.\n",
               (unsigned long)r.num_passed, (unsigned long)(r.num_passed + r.num_failed));
      } else {
        printf("\nFiltering: disabled\n");
        printf("\tSo, statistics were computed for the whole input file.\n");
      }
    } else if (p.paired) {
      const char *ok = cmd == CMD_FILTER ? "passed" : "edit";
      if (cmd == CMD_EDIT) printf("Num. edited reads : %lu (mate 1)\n", (unsigned long)r.num_edited);
      if (r.ovl_on) printf("Num. overlap-clipped pairs : %lu\n", (unsigned long)r.ovl.clipped);
      if (r.ovl_merge_on) {   /* (the pair lines below then count the pairs that did not merge) */
        printf("Num. merged pairs : %lu (%s/edit_merged.fq)\n", (unsigned long)r.ovl_merge.merged_pairs, o->out_dirname);
        if (p.filter_on) {
          printf("\tNum. passed merged reads : %lu\n", (unsigned long)r.merged_passed);
          printf("\tNum. failed merged reads : %lu\n", (unsigned long)r.merged_failed);
        }
      }
      if (r.ovl_fix_on) printf("Num. overlap-corrected pairs : %lu\n", (unsigned long)r.ovl_fix.corrected_pairs);
      if (r.clip_on) printf("Num. clipped reads : %lu (mate 1)\n", (unsigned long)r.clip[0].clipped);
      printf("Num. passed pairs : %lu (%s/%s_1.fq, %s/%s_2.fq)\n", (unsigned long)r.num_passed, o->out_dirname, ok,
             o->out_dirname, ok);
      if (p.filter_on)
        printf("Num. failed pairs : %lu (%s/failed_1.fq, %s/failed_2.fq)\n", (unsigned long)r.num_failed,
               o->out_dirname, o->out_dirname);
    } else if (cmd == CMD_FILTER) {
      printf("Num. passed reads: %lu (%s/passed.fq)\n", (unsigned long)r.num_passed, o->out_dirname);
      printf("Num. failed reads: %lu (%s/failed.fq)\n", (unsigned long)r.num_failed, o->out_dirname);
    } else {
      printf("Num. edited reads : %lu\n", (unsigned long)r.num_edited);
      if (r.clip_on) printf("Num. clipped reads : %lu\n", (unsigned long)r.clip[0].clipped);
      printf("Output file       : %s/edit.fq\n", o->out_dirname);
      if (p.filter_on) {
        printf("\nFiltering : Enabled\n");
        printf("\tNum. passed reads : %lu (%s/edit.fq)\n", (unsigned long)r.num_passed, o->out_dirname);
        printf("\tNum. failed reads : %lu (%s/failed.fq)\n", (unsigned long)r.num_failed, o->out_dirname);
      }
    }
    if (r.writer)
      printf("Output writer     : %s\n", r.writer == 1 ? "mapped files, parallel copy" : "one stream writer thread");
    printf("\nThroughput: %lu %s, %.3f GB of FastQ in %.3f s = %.2f M%s/s (%d GPU worker%s)\n",
           (unsigned long)r.num_reads, p.paired ? "pairs" : "reads", r.fastq_bytes / 1e9, r.seconds,
           r.seconds > 0 ? r.num_reads / r.seconds / 1e6 : 0.0, p.paired ? "pairs" : "reads", r.num_gpus,
           r.num_gpus == 1 ? "" : "s");
    printf("=================================================\n");
  }
  free(r.counters);
  free(r.kmers);
  free(r.qdist[0]);
  free(r.qdist[1]);
  free(r.adapt[0]);
  free(r.adapt[1]);
  for (int m = 0; m < 2; ++m) {
    free(r.dup_keys[m]);
    free(r.dup_counts[m]);
    for (size_t i = 0; r.overrep_seqs[m] && i < r.overrep_n[m]; ++i) free(r.overrep_seqs[m][i]);
    free(r.overrep_seqs[m]);
    free(r.overrep_counts[m]);
    free(r.overrep_lens[m]);
  }
  free(r.cg_seq);
  free(r.cg_q);
  cli_free(o);
  return rc;
}
