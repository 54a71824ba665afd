/*
 * hpgq_report_adapt.c — the probe set and the report file of `stats --adapters`
 * (build-defined; the reference has nothing like it).
 *
 * cli_adapters_load: the set a run counts, from --adapter-file (lines of name,
 * tab(s), sequence) or libhpgq's default set; `edit --clip-adapters` takes its
 * set through it too, from --clip-adapter-file.
 *
 * <in>.adapter.content.data: the counted reads and those with any probe, then
 * per position p = 1 .. npos and probe the percentage of the counted reads in
 * which the probe's first occurrence starts at or before p.  A file of its own
 * beside hpgq_report.c, like hpgq_report_qdist.c.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq_cli.h"

static const char *file_flag = "--adapter-file";   /* the flag the file came with (cli_adapters_load sets it) */

static int file_error(const char *path, long line, const char *what) {
  fprintf(stderr, "hpg-fastq: %s: %s:%ld: %s\n", file_flag, path, line, what);
  return -1;
}

int cli_adapters_load(cli_options_t *o) {
  o->adapter_n = 0;
  file_flag = o->clip_on ? "--clip-adapter-file" : "--adapter-file";
  if (!o->adapter_file) {
    const int n = hpgq_adapt_default(-1, NULL, NULL);
    for (int i = 0; i < n && i < HPGQ_ADAPT_MAX_PROBES; ++i) {
      const char *name = "", *probe = "";
      hpgq_adapt_default(i, &name, &probe);
      snprintf(o->adapter_names[i], sizeof(o->adapter_names[i]), "%s", name);
      snprintf(o->adapter_probes[i], sizeof(o->adapter_probes[i]), "%s", probe);
      o->adapter_n = i + 1;
    }
    return 0;
  }
  const char *path = o->adapter_file;
  FILE *f = fopen(path, "r");
  if (!f) return file_error(path, 0, "cannot open the file");
  char *line = NULL;
  size_t cap = 0;
  ssize_t got;
  long ln = 0;
  int rc = 0;
  while (rc == 0 && (got = getline(&line, &cap, f)) >= 0) {
    ++ln;
    size_t n = (size_t)got;
    if (n && line[n - 1] == '\n') --n;
    if (n && line[n - 1] == '\r') --n;
    if (n == 0 || line[0] == '#') continue;
    if (memchr(line, 0, n)) {
      rc = file_error(path, ln, "a NUL byte in the line");
      break;
    }
    line[n] = 0;
    /* split at the last run of tabs: the name may hold tabs, the sequence cannot */
    size_t s = n;
    while (s > 0 && line[s - 1] != '\t') --s;         /* the sequence is line[s, n) */
    size_t e = s;
    while (e > 0 && line[e - 1] == '\t') --e;         /* the name is line[0, e) */
    if (s == 0) rc = file_error(path, ln, "expected a name, one or more tabs and a sequence");
    else if (e == 0) rc = file_error(path, ln, "the name is empty");
    else if (e > CLI_ADAPTER_NAME_MAX) rc = file_error(path, ln, "the name is longer than 64 bytes");
    else if (hpgq_adapt_find(NULL, 0, line + s) == -2)
      rc = file_error(path, ln, "the sequence must be 8 to 32 of the letters A C G T (upper case)");
    else if (o->adapter_n == HPGQ_ADAPT_MAX_PROBES) rc = file_error(path, ln, "more than 32 adapters");
    if (rc) break;
    memcpy(o->adapter_names[o->adapter_n], line, e);
    o->adapter_names[o->adapter_n][e] = 0;
    snprintf(o->adapter_probes[o->adapter_n], sizeof(o->adapter_probes[0]), "%s", line + s);
    o->adapter_n++;
  }
  free(line);
  fclose(f);
  if (rc == 0 && o->adapter_n == 0) rc = file_error(path, ln, "no adapter in the file");
  return rc;
}

int cli_report_adapt(const cli_options_t *o, int nprobes, const char *const *names, const uint64_t *first, int npos,
                     uint64_t reads, uint64_t with_any, const char *base) {
  uint64_t *cum = calloc((size_t)nprobes + 1, sizeof(uint64_t));
  if (!cum) return -1;
  char path[4096];
  snprintf(path, sizeof(path), "%s/%s.adapter.content.data", o->out_dirname, base);
  FILE *f = fopen(path, "w");
  if (!f) {
    free(cum);
    return -1;
  }
  fprintf(f, "# Reads\tWith adapter\t%% with adapter\n");
  fprintf(f, "%lu\t%lu\t%.2f\n", (unsigned long)reads, (unsigned long)with_any, reads ? 100.0 * with_any / reads : 0.0);
  fprintf(f, "# Position");
  for (int a = 0; a < nprobes; ++a) fprintf(f, "\t%s", names[a]);
  fprintf(f, "\n");
  for (int p = 0; p < npos; ++p) {
    fprintf(f, "%i", p + 1);
    for (int a = 0; a < nprobes; ++a) {
      cum[a] += first[(size_t)a * (size_t)npos + (size_t)p];
      fprintf(f, "\t%.4f", reads ? 100.0 * cum[a] / reads : 0.0);
    }
    fprintf(f, "\n");
  }
  const int bad = ferror(f);
  if (fclose(f) || bad) {
    free(cum);
    return -1;
  }
  free(cum);
  return 0;
}
