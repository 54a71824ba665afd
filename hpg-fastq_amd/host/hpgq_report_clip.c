/*
 * hpgq_report_clip.c — the report file of `edit --clip-adapters` (build-defined,
 * DESIGN.md §2.12; the reference has nothing like it).
 *
 * <in>.adapter.clip.data: the reads, those cut and the bases cut off, then per
 * probe the reads it cut and their share of all reads.  A file of its own
 * beside hpgq_report.c, like hpgq_report_adapt.c.
 */
#include <stdio.h>

#include "hpgq_cli.h"

static double percent(uint64_t num, uint64_t den) { return den ? 100.0 * num / den : 0.0; }

int cli_report_clip(const cli_options_t *o, int nprobes, const char *const *names, const hpgq_clip_info_t *info,
                    const char *base) {
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.adapter.clip.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  fprintf(f, "# Reads\tClipped\t%% clipped\tBases removed\n");
  fprintf(f, "%lu\t%lu\t%.2f\t%lu\n", (unsigned long)info->reads, (unsigned long)info->clipped,
          percent(info->clipped, info->reads), (unsigned long)info->bases_removed);
  fprintf(f, "# Adapter\tReads\t%% of reads\n");
  for (int a = 0; a < nprobes; ++a)
    fprintf(f, "%s\t%lu\t%.2f\n", names[a], (unsigned long)info->by_probe[a], percent(info->by_probe[a], info->reads));
  const int bad = ferror(f);
  if (fclose(f) || bad) return -1;
  return 0;
}
