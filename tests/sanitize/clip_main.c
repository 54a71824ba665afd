/*
 * clip_main.c — hpgq_clip_find (csrc/hpgq_clip_post.cpp) under ASan + UBSan, no
 * GPU.  Built and run by tests/test_clip_cpu.py.
 *
 * argv[1]: a text file, one case per line:
 *   min_overlap nprobes probe_hex_1 .. probe_hex_nprobes read_hex want_c want_probe
 * ("-": no bytes).  hpgq_clip_find over the read must return want_c and set the
 * winner to want_probe.  The read and every probe are heap blocks of their
 * exact size (a probe's NUL is its last byte), so an access past them is caught.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "clip_main: %s (case %ld)\n", what, line);
  return 1;
}

/* hex -> a heap block of exactly its length + extra ("-": length 0) */
static unsigned char *unhex(const char *hex, size_t *len, size_t extra) {
  *len = strcmp(hex, "-") ? strlen(hex) / 2 : 0;
  unsigned char *b = malloc(*len + extra ? *len + extra : 1);
  for (size_t j = 0; b && j < *len; ++j) {
    unsigned v;
    if (sscanf(hex + 2 * j, "%2x", &v) != 1) return NULL;
    b[j] = (unsigned char)v;
  }
  if (b && extra) b[*len] = 0;
  return b;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: clip_main <cases.txt>", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the cases", 0);
  char *word = malloc(1 << 20);
  if (!word) return fail("out of memory", 0);
  long ncase = 0;
  int min_overlap, nprobes;
  while (fscanf(f, "%d %d", &min_overlap, &nprobes) == 2) {
    if (nprobes < 0 || nprobes > 64) return fail("bad case", ncase);
    char *probes[64];
    size_t n;
    for (int a = 0; a < nprobes; ++a) {
      if (fscanf(f, "%1048575s", word) != 1) return fail("bad probe", ncase);
      probes[a] = (char *)unhex(word, &n, 1);
      if (!probes[a]) return fail("bad probe bytes", ncase);
    }
    long long want_c;
    int want_probe, got_probe = 12345;
    if (fscanf(f, "%1048575s %lld %d", word, &want_c, &want_probe) != 3) return fail("bad read", ncase);
    unsigned char *s = unhex(word, &n, 0);
    if (!s) return fail("bad read bytes", ncase);
    const long long c = hpgq_clip_find(s, n, (const char *const *)probes, nprobes, min_overlap, &got_probe);
    if (c != want_c || got_probe != want_probe) {
      fprintf(stderr, "clip_main: got c %lld probe %d, want %lld %d\n", c, got_probe, want_c, want_probe);
      return fail("wrong result", ncase);
    }
    if (hpgq_clip_find(s, n, (const char *const *)probes, nprobes, min_overlap, NULL) != want_c)
      return fail("wrong result without the probe output", ncase);
    free(s);
    for (int a = 0; a < nprobes; ++a) free(probes[a]);
    ++ncase;
  }
  free(word);
  fclose(f);
  printf("clip_main: ok %ld cases\n", ncase);
  return 0;
}
