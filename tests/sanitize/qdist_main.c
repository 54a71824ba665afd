/*
 * qdist_main.c — hpgq_qdist_quantiles / hpgq_qdist_add (csrc/hpgq_qdist_post.cpp)
 * under ASan + UBSan, no GPU.  Built and run by tests/test_qdist_cpu.py.
 *
 * argv[1]: a text file, one case per line:
 *   phred k  byte_1 count_1 ... byte_k count_k  count min p10 q1 median q3 p90 max
 * Every case becomes one row of a heap table (exact size, so a read past it is
 * caught), all rows go through one hpgq_qdist_quantiles call per phred value
 * met, and each result must equal the line's eight numbers.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "qdist_main: %s (case %ld)\n", what, line);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: qdist_main <cases.txt>", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the cases", 0);
  long ncase = 0;
  int phred, k;
  while (fscanf(f, "%d %d", &phred, &k) == 2) {
    uint64_t *row = calloc(HPGQ_QDIST_VALUES, sizeof(uint64_t));
    hpgq_qdist_row_t *got = calloc(1, sizeof(*got));
    if (!row || !got) return fail("out of memory", ncase);
    for (int i = 0; i < k; ++i) {
      int b;
      uint64_t c;
      if (fscanf(f, "%d %" SCNu64, &b, &c) != 2 || b < 0 || b > 255) return fail("bad cell", ncase);
      row[b] = c;
    }
    uint64_t wc;
    int w[7];
    if (fscanf(f, "%" SCNu64 " %d %d %d %d %d %d %d", &wc, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6]) != 8)
      return fail("bad expectation", ncase);
    if (hpgq_qdist_quantiles(row, 1, phred, got) != HPGQ_OK) return fail("hpgq_qdist_quantiles failed", ncase);
    const int g[7] = {got->min, got->p10, got->q1, got->median, got->q3, got->p90, got->max};
    if (got->count != wc || memcmp(g, w, sizeof(g))) {
      fprintf(stderr, "got %" PRIu64 " %d %d %d %d %d %d %d\n", got->count, g[0], g[1], g[2], g[3], g[4], g[5], g[6]);
      return fail("wrong quantiles", ncase);
    }
    free(row);
    free(got);
    ++ncase;
  }
  fclose(f);
  if (!ncase) return fail("no cases", 0);

  /* hpgq_qdist_add: the first rows added, the rest untouched, a longer source rejected */
  const int nd = 3, ns = 2;
  uint64_t *dst = malloc((size_t)nd * HPGQ_QDIST_VALUES * sizeof(uint64_t));
  uint64_t *src = malloc((size_t)ns * HPGQ_QDIST_VALUES * sizeof(uint64_t));
  if (!dst || !src) return fail("out of memory", -1);
  for (int i = 0; i < nd * HPGQ_QDIST_VALUES; ++i) dst[i] = (uint64_t)i;
  for (int i = 0; i < ns * HPGQ_QDIST_VALUES; ++i) src[i] = 1000u + (uint64_t)i;
  if (hpgq_qdist_add(dst, nd, src, ns) != HPGQ_OK) return fail("hpgq_qdist_add failed", -1);
  for (int i = 0; i < nd * HPGQ_QDIST_VALUES; ++i)
    if (dst[i] != (uint64_t)i + (i < ns * HPGQ_QDIST_VALUES ? 1000u + (uint64_t)i : 0)) return fail("wrong sum", i);
  if (hpgq_qdist_add(src, ns, dst, nd) != HPGQ_E_INVALID) return fail("a longer source was accepted", -1);
  if (hpgq_qdist_add(dst, nd, src, 0) != HPGQ_OK || hpgq_qdist_quantiles(NULL, 0, 33, NULL) != HPGQ_OK)
    return fail("the empty table was rejected", -1);
  free(dst);
  free(src);
  printf("qdist_main: ok %ld cases\n", ncase);
  return 0;
}
