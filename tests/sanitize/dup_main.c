/*
 * dup_main.c — hpgq_dup_fingerprint / hpgq_dup_levels_of (csrc/hpgq_dup_post.cpp)
 * and the report writer (host/hpgq_report_dup.c) under ASan + UBSan, no GPU.
 * Built and run by tests/test_dup_cpu.py.
 *
 * argv[1]: a text file, one case per line:
 *   F n hex want          the fingerprint (hex) of the n bytes given in hex ("-" for none)
 *   L n c_1 .. c_n  reads distinct max d_0 .. d_15 r_0 .. r_15
 *                         the levels of n counts
 * argv[2], argv[3]: an output directory and a base name; the levels of the LAST
 * L case are written to <dir>/<base>.duplication.data (the test compares the
 * bytes).  Every input is a heap block of its exact size, so a read past it is
 * caught.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq_cli.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "dup_main: %s (case %ld)\n", what, line);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 4) return fail("usage: dup_main <cases.txt> <outdir> <base>", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the cases", 0);
  long ncase = 0;
  char kind;
  size_t n;
  hpgq_dup_levels_t last;
  int have_levels = 0;
  while (fscanf(f, " %c %zu", &kind, &n) == 2) {
    if (kind == 'F') {
      unsigned char *s = malloc(n ? n : 1);
      char *hex = malloc(2 * n + 2);
      uint64_t want;
      if (!s || !hex) return fail("out of memory", ncase);
      if (fscanf(f, "%s %" SCNx64, hex, &want) != 2) return fail("bad fingerprint case", ncase);
      if (n && strlen(hex) != 2 * n) return fail("bad hex length", ncase);
      for (size_t i = 0; i < n; ++i) {
        unsigned b;
        if (sscanf(hex + 2 * i, "%2x", &b) != 1) return fail("bad hex", ncase);
        s[i] = (unsigned char)b;
      }
      /* (n == 0: a pointer to no readable byte at all) */
      const uint64_t got = hpgq_dup_fingerprint(n ? s : NULL, n);
      if (got != want) {
        fprintf(stderr, "got %016" PRIx64 " want %016" PRIx64 "\n", got, want);
        return fail("wrong fingerprint", ncase);
      }
      free(s);
      free(hex);
    } else if (kind == 'L') {
      uint64_t *c = malloc((n ? n : 1) * sizeof(uint64_t));
      hpgq_dup_levels_t *got = malloc(sizeof(*got)), want;
      if (!c || !got) return fail("out of memory", ncase);
      for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%" SCNu64, &c[i]) != 1) return fail("bad count", ncase);
      if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &want.reads, &want.distinct, &want.max_count) != 3)
        return fail("bad expectation", ncase);
      for (int i = 0; i < HPGQ_DUP_LEVELS; ++i)
        if (fscanf(f, "%" SCNu64, &want.distinct_at[i]) != 1) return fail("bad expectation", ncase);
      for (int i = 0; i < HPGQ_DUP_LEVELS; ++i)
        if (fscanf(f, "%" SCNu64, &want.reads_at[i]) != 1) return fail("bad expectation", ncase);
      if (hpgq_dup_levels_of(n ? c : NULL, n, got) != HPGQ_OK) return fail("hpgq_dup_levels_of failed", ncase);
      if (got->reads != want.reads || got->distinct != want.distinct || got->max_count != want.max_count ||
          memcmp(got->distinct_at, want.distinct_at, sizeof(want.distinct_at)) ||
          memcmp(got->reads_at, want.reads_at, sizeof(want.reads_at)))
        return fail("wrong levels", ncase);
      last = *got;
      have_levels = 1;
      free(c);
      free(got);
    } else {
      return fail("unknown case kind", ncase);
    }
    ++ncase;
  }
  fclose(f);
  if (!ncase || !have_levels) return fail("no cases", 0);
  if (hpgq_dup_levels_of(NULL, 1, &last) != HPGQ_E_INVALID || hpgq_dup_levels_of(NULL, 0, NULL) != HPGQ_E_INVALID)
    return fail("a NULL argument was accepted", -1);
  if (hpgq_dup_level_bound(-1) != 0 || hpgq_dup_level_bound(HPGQ_DUP_LEVELS) != 0 || hpgq_dup_level_bound(10) != 50)
    return fail("wrong level bounds", -1);

  cli_options_t *o = calloc(1, sizeof(*o));
  if (!o) return fail("out of memory", -1);
  o->out_dirname = argv[2];
  if (cli_report_dup(o, &last, argv[3])) return fail("cli_report_dup failed", -1);
  free(o);
  printf("dup_main: ok %ld cases\n", ncase);
  return 0;
}
