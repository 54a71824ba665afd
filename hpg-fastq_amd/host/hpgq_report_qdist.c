/*
 * hpgq_report_qdist.c — the report file of `stats --quality-dist`
 * (build-defined; the reference's report has means only).
 *
 * <in>.quality.dist.per.nt.data: a header line, then one line per position
 * 1..npos with the bases counted there and the min, P10, Q1, median, Q3, P90
 * and max quality (hpgq_qdist_quantiles).  A file of its own beside
 * hpgq_report.c: that one restates src/stats_report.c and needs nothing of
 * libhpgq but the counter layout.
 */
#include <stdio.h>
#include <stdlib.h>

#include "hpgq_cli.h"

int cli_report_qdist(const cli_options_t *o, const hpgq_params_t *p, const uint64_t *hist, int npos,
                     const char *base) {
  hpgq_qdist_row_t *rows = calloc((size_t)npos + 1, sizeof(*rows));
  if (!rows || hpgq_qdist_quantiles(hist, npos, p->phred, rows)) {
    free(rows);
    return -1;
  }
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.quality.dist.per.nt.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) {
    free(rows);
    return -1;
  }
  fprintf(f, "# Position\tCount\tMin\tP10\tQ1\tMedian\tQ3\tP90\tMax\n");
  for (int k = 0; k < npos; k++)
    fprintf(f, "%i\t%lu\t%i\t%i\t%i\t%i\t%i\t%i\t%i\n", k + 1, (unsigned long)rows[k].count, rows[k].min, rows[k].p10,
            rows[k].q1, rows[k].median, rows[k].q3, rows[k].p90, rows[k].max);
  fclose(f);
  free(rows);
  return 0;
}
