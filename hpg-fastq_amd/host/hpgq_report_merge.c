/*
 * hpgq_report_merge.c — the report file of `edit --merge-overlap`
 * (build-defined; the reference has nothing like it).
 *
 * <mate 1's base>.overlap.merge.data: the pairs, those whose mates overlap,
 * those merged into one read, the merged reads' bases and the facing bases
 * each mate resolved.  A file of its own beside hpgq_report_ovl.c.
 */
#include <stdio.h>

#include "hpgq_cli.h"

static double percent(uint64_t num, uint64_t den) { return den ? 100.0 * num / den : 0.0; }

int cli_report_merge(const cli_options_t *o, const hpgq_ovl_info_t *info, const hpgq_ovl_merge_info_t *merge,
                     const char *base) {
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.overlap.merge.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  fprintf(f, "# Pairs\tOverlapping\tMerged\t%% merged\tMerged bases\tResolved by mate 1\tResolved by mate 2\n");
  fprintf(f, "%lu\t%lu\t%lu\t%.2f\t%lu\t%lu\t%lu\n", (unsigned long)info->pairs, (unsigned long)info->overlapping,
          (unsigned long)merge->merged_pairs, percent(merge->merged_pairs, info->pairs),
          (unsigned long)merge->merged_bases, (unsigned long)merge->resolved[0], (unsigned long)merge->resolved[1]);
  const int bad = ferror(f);
  if (fclose(f) || bad) return -1;
  return 0;
}
