/*
 * overrep_main.c — hpgq_dup_top_of (csrc/hpgq_dup_post.cpp) and the report
 * writer (host/hpgq_report_overrep.c) under ASan + UBSan, no GPU.  Built and
 * run by tests/test_overrep_cpu.py.
 *
 * argv[1]: a text file, one case per line:
 *   T n cap min  k_1 c_1 .. k_n c_n  total m  ok_1 oc_1 .. ok_m oc_m
 *        the selection over n pairs: `total` qualify, the first m = min(cap,
 *        total) are expected in order
 *   R base reads n  c_1 len_1 hex_1 .. c_n len_n hex_n
 *        n listed sequences ("-" for no bytes) written to
 *        <argv[2]>/<base>.overrepresented.data (the test compares the bytes)
 * Every input and output is a heap block of its exact size, so an access past
 * it is caught.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq_cli.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "overrep_main: %s (case %ld)\n", what, line);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 3) return fail("usage: overrep_main <cases.txt> <outdir>", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the cases", 0);
  long ncase = 0;
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'T') {
      size_t n, cap, total, m, got_total = 0;
      uint64_t min_count;
      if (fscanf(f, "%zu %zu %" SCNu64, &n, &cap, &min_count) != 3) return fail("bad selection case", ncase);
      uint64_t *k = malloc((n ? n : 1) * sizeof(uint64_t)), *c = malloc((n ? n : 1) * sizeof(uint64_t));
      uint64_t *ok = malloc((cap ? cap : 1) * sizeof(uint64_t)), *oc = malloc((cap ? cap : 1) * sizeof(uint64_t));
      if (!k || !c || !ok || !oc) return fail("out of memory", ncase);
      for (size_t i = 0; i < n; ++i)
        if (fscanf(f, "%" SCNu64 " %" SCNu64, &k[i], &c[i]) != 2) return fail("bad pair", ncase);
      if (fscanf(f, "%zu %zu", &total, &m) != 2 || m > cap) return fail("bad expectation", ncase);
      if (hpgq_dup_top_of(n ? k : NULL, n ? c : NULL, n, min_count, NULL, NULL, 0, &got_total) != HPGQ_OK ||
          got_total != total)
        return fail("wrong total of the query", ncase);
      got_total = 0;
      if (hpgq_dup_top_of(n ? k : NULL, n ? c : NULL, n, min_count, ok, oc, cap, &got_total) != HPGQ_OK)
        return fail("hpgq_dup_top_of failed", ncase);
      if (got_total != total) return fail("wrong total", ncase);
      for (size_t i = 0; i < m; ++i) {
        uint64_t wk, wc;
        if (fscanf(f, "%" SCNu64 " %" SCNu64, &wk, &wc) != 2) return fail("bad expectation", ncase);
        if (ok[i] != wk || oc[i] != wc) return fail("wrong entry", ncase);
      }
      free(k);
      free(c);
      free(ok);
      free(oc);
    } else if (kind == 'R') {
      char base[256];
      uint64_t reads;
      size_t n;
      if (fscanf(f, "%255s %" SCNu64 " %zu", base, &reads, &n) != 3) return fail("bad render case", ncase);
      uint64_t *c = malloc((n ? n : 1) * sizeof(uint64_t)), *len = malloc((n ? n : 1) * sizeof(uint64_t));
      unsigned char **s = malloc((n ? n : 1) * sizeof(*s));
      if (!c || !len || !s) return fail("out of memory", ncase);
      for (size_t i = 0; i < n; ++i) {
        if (fscanf(f, "%" SCNu64 " %" SCNu64, &c[i], &len[i]) != 2) return fail("bad entry", ncase);
        char *hex = malloc(2 * len[i] + 2);
        s[i] = malloc(len[i] ? len[i] : 1);
        if (!hex || !s[i] || fscanf(f, "%s", hex) != 1) return fail("bad entry bytes", ncase);
        if (len[i] && strlen(hex) != 2 * len[i]) return fail("bad hex length", ncase);
        for (size_t j = 0; j < len[i]; ++j) {
          unsigned b;
          if (sscanf(hex + 2 * j, "%2x", &b) != 1) return fail("bad hex", ncase);
          s[i][j] = (unsigned char)b;
        }
        free(hex);
      }
      cli_options_t *o = calloc(1, sizeof(*o));
      if (!o) return fail("out of memory", ncase);
      o->out_dirname = argv[2];
      if (cli_report_overrep(o, n, c, len, s, reads, base)) return fail("cli_report_overrep failed", ncase);
      free(o);
      for (size_t i = 0; i < n; ++i) free(s[i]);
      free(s);
      free(c);
      free(len);
    } else {
      return fail("unknown case kind", ncase);
    }
    ++ncase;
  }
  fclose(f);
  if (!ncase) return fail("no cases", 0);
  size_t t = 0;
  uint64_t one = 1;
  if (hpgq_dup_top_of(NULL, NULL, 1, 1, NULL, NULL, 0, &t) != HPGQ_E_INVALID ||
      hpgq_dup_top_of(&one, &one, 1, 0, NULL, NULL, 0, &t) != HPGQ_E_INVALID ||
      hpgq_dup_top_of(&one, &one, 1, 1, NULL, NULL, 0, NULL) != HPGQ_E_INVALID)
    return fail("a bad argument was accepted", -1);
  printf("overrep_main: ok %ld cases\n", ncase);
  return 0;
}
