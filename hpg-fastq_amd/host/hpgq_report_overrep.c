/*
 * hpgq_report_overrep.c — the report file of `stats --overrepresented`
 * (build-defined).
 *
 * <in>.overrepresented.data: one line per listed sequence in rank order (count
 * descending, ties by fingerprint ascending): rank from 1, count, the share of
 * the counted reads, length, and the sequence bytes as they stand (a tab or
 * any other byte included: the length says where the line's sequence ends).
 * A zero denominator prints 0.0000.  A file of its own beside hpgq_report.c,
 * like hpgq_report_dup.c: it needs nothing of libhpgq.
 */
#include <stdio.h>

#include "hpgq_cli.h"

int cli_report_overrep(const cli_options_t *o, size_t n, const uint64_t *counts, const uint64_t *lens,
                       unsigned char *const *seqs, uint64_t reads, const char *base) {
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.overrepresented.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  fprintf(f, "# Rank\tCount\t%% of reads\tLength\tSequence\n");
  for (size_t i = 0; i < n; i++) {
    fprintf(f, "%i\t%lu\t%.4f\t%lu\t", (int)(i + 1), (unsigned long)counts[i], reads ? 100.0 * counts[i] / reads : 0.0,
            (unsigned long)lens[i]);
    if (lens[i]) fwrite(seqs[i], 1, (size_t)lens[i], f);
    fputc('\n', f);
  }
  const int bad = ferror(f);
  return fclose(f) || bad ? -1 : 0;
}
