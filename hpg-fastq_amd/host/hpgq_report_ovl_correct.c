/*
 * hpgq_report_ovl_correct.c — the report file of `edit --correct-overlap`
 * (build-defined; the reference has nothing like it).
 *
 * <mate 1's base>.overlap.correct.data: the pairs, those whose mates overlap,
 * those with at least one corrected base, and the bases corrected in each
 * mate.  A file of its own beside hpgq_report_ovl.c.
 */
#include <stdio.h>

#include "hpgq_cli.h"

static double percent(uint64_t num, uint64_t den) { return den ? 100.0 * num / den : 0.0; }

int cli_report_ovl_correct(const cli_options_t *o, const hpgq_ovl_info_t *info, const hpgq_ovl_correct_info_t *fix,
                           const char *base) {
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.overlap.correct.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  fprintf(f, "# Pairs\tOverlapping\tCorrected pairs\t%% corrected\tBases corrected 1\tBases corrected 2\n");
  fprintf(f, "%lu\t%lu\t%lu\t%.2f\t%lu\t%lu\n", (unsigned long)info->pairs, (unsigned long)info->overlapping,
          (unsigned long)fix->corrected_pairs, percent(fix->corrected_pairs, info->pairs),
          (unsigned long)fix->corrected_bases[0], (unsigned long)fix->corrected_bases[1]);
  const int bad = ferror(f);
  if (fclose(f) || bad) return -1;
  return 0;
}
