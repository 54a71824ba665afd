/*
 * hpgq_report_ovl.c — the report file of `edit --clip-overlap` (build-defined,
 * DESIGN.md §2.13; the reference has nothing like it).
 *
 * <mate 1's base>.overlap.clip.data: the pairs, those skipped (a mate longer
 * than HPGQ_OVL_MAX_LEN), those whose mates overlap, those cut, and the bases
 * cut off each mate.  A file of its own beside hpgq_report.c, like
 * hpgq_report_clip.c.
 */
#include <stdio.h>

#include "hpgq_cli.h"

static double percent(uint64_t num, uint64_t den) { return den ? 100.0 * num / den : 0.0; }

int cli_report_ovl(const cli_options_t *o, const hpgq_ovl_info_t *info, const char *base) {
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.overlap.clip.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  fprintf(f, "# Pairs\tSkipped\tOverlapping\t%% overlapping\tClipped\t%% clipped\tBases removed 1\tBases removed 2\n");
  fprintf(f, "%lu\t%lu\t%lu\t%.2f\t%lu\t%.2f\t%lu\t%lu\n", (unsigned long)info->pairs, (unsigned long)info->skipped,
          (unsigned long)info->overlapping, percent(info->overlapping, info->pairs), (unsigned long)info->clipped,
          percent(info->clipped, info->pairs), (unsigned long)info->bases_removed[0], (unsigned long)info->bases_removed[1]);
  const int bad = ferror(f);
  if (fclose(f) || bad) return -1;
  return 0;
}
