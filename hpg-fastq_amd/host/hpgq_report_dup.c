/*
 * hpgq_report_dup.c — the report file of `stats --duplication` (build-defined,
 * DESIGN.md §2.9).
 *
 * <in>.duplication.data: the reads counted, the distinct sequences, the highest
 * count and the share of distinct sequences; then one line per duplication
 * level with the sequences at that level, the reads they account for and both
 * as percentages.  A zero denominator prints 0.00 (quirk Q14's convention).  A
 * file of its own beside hpgq_report.c, like hpgq_report_qdist.c: it needs
 * nothing of libhpgq but the levels struct.
 */
#include <stdio.h>

#include "hpgq_cli.h"

static double pct(uint64_t a, uint64_t b) { return b ? 100.0 * a / b : 0.0; }

int cli_report_dup(const cli_options_t *o, const hpgq_dup_levels_t *lv, const char *base) {
  static const char *const label[HPGQ_DUP_LEVELS] = {"1", "2", "3", "4", "5", "6", "7", "8", "9", ">=10", ">=50",
                                                     ">=100", ">=500", ">=1000", ">=5000", ">=10000"};
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.duplication.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  fprintf(f, "# Reads\tDistinct\tHighest count\t%% distinct\n");
  fprintf(f, "%lu\t%lu\t%lu\t%.2f\n", (unsigned long)lv->reads, (unsigned long)lv->distinct,
          (unsigned long)lv->max_count, pct(lv->distinct, lv->reads));
  fprintf(f, "# Level\tSequences\tReads\t%% of sequences\t%% of reads\n");
  for (int i = 0; i < HPGQ_DUP_LEVELS; i++)
    fprintf(f, "%s\t%lu\t%lu\t%.2f\t%.2f\n", label[i], (unsigned long)lv->distinct_at[i],
            (unsigned long)lv->reads_at[i], pct(lv->distinct_at[i], lv->distinct), pct(lv->reads_at[i], lv->reads));
  const int bad = ferror(f);
  return fclose(f) || bad ? -1 : 0;
}
