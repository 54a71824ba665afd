/*
 * hpgq_report_insert.c — the report file of `edit --insert-size`
 * (build-defined; the reference has nothing like it).
 *
 * <mate 1's base>.insert.size.data: the pairs, those skipped, those analysed
 * without and with an overlap, the least, median and greatest insert size and
 * the mean; then one row per insert size from the least to the greatest, rows
 * of no pair included.  The median is the least F >= 1 at which twice the
 * pairs up to F reach the overlapping pairs.  Without an overlapping pair the
 * file ends with the second header.
 */
#include <stdio.h>

#include "hpgq_cli.h"

int cli_report_insert(const cli_options_t *o, const hpgq_ovl_info_t *info, const uint64_t hist[HPGQ_OVL_INSERT_BINS],
                      const char *base) {
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.insert.size.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  uint64_t with = 0;
  double sum = 0.0;
  int min = 0, max = 0, median = 0;
  for (int F = 1; F < HPGQ_OVL_INSERT_BINS; ++F) {
    if (!hist[F]) continue;
    if (!with) min = F;
    max = F;
    with += hist[F];
    sum += (double)F * (double)hist[F];
  }
  uint64_t upto = 0;
  for (int F = 1; F <= max && !median; ++F) {
    upto += hist[F];
    if (2 * upto >= with) median = F;
  }
  fprintf(f, "# Pairs\tSkipped\tWithout overlap\tWith overlap\tMin\tMedian\tMax\tMean\n");
  fprintf(f, "%lu\t%lu\t%lu\t%lu\t%d\t%d\t%d\t%.2f\n", (unsigned long)info->pairs, (unsigned long)info->skipped,
          (unsigned long)hist[0], (unsigned long)with, min, median, max, with ? sum / (double)with : 0.0);
  fprintf(f, "# Insert size\tPairs\t%% of overlapping\n");
  for (int F = min; with && F <= max; ++F)
    fprintf(f, "%d\t%lu\t%.2f\n", F, (unsigned long)hist[F], 100.0 * (double)hist[F] / (double)with);
  const int bad = ferror(f);
  if (fclose(f) || bad) return -1;
  return 0;
}
