/*
 * ovl_main.cpp — `edit --clip-overlap` without a GPU, under ASan + UBSan:
 * hpgq_ovl_find (csrc/hpgq_ovl_post.cpp) and the lane arithmetic of the kernel
 * (csrc/hpgq_ovl_lane.h) walked on the host, lane by lane and block by block as
 * ovl_find_kernel does.  Built and run by tests/test_ovl_cpu.py.
 *
 * argv[1]: a text file, one case per line:
 *   min_overlap max_mismatches mate1_hex mate2_hex want
 * ("-": no bytes).  Both must give `want`.  The mates and the packed pair are
 * heap blocks of their exact size, so an access past them is caught.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hpgq.h"
#include "../../hpg-fastq_amd/csrc/hpgq_ovl_lane.h"

using namespace hpgq::ovl;

static int fail(const char *what, long line) {
  fprintf(stderr, "ovl_main: %s (case %ld)\n", what, line);
  return 1;
}

/* hex -> a heap block of exactly its length ("-": length 0) */
static unsigned char *unhex(const char *hex, size_t *len) {
  *len = strcmp(hex, "-") ? strlen(hex) / 2 : 0;
  unsigned char *b = static_cast<unsigned char *>(malloc(*len ? *len : 1));
  for (size_t j = 0; b && j < *len; ++j) {
    unsigned v;
    if (sscanf(hex + 2 * j, "%2x", &v) != 1) return NULL;
    b[j] = (unsigned char)v;
  }
  return b;
}

/* what pack4 makes of the read's bytes 4 q .. 4 q + 3 (those past its end: no base) */
static void pack4_host(const unsigned char *s, size_t n, int q, uint32_t *c, uint32_t *ok) {
  *c = *ok = 0;
  for (int j = 0; j < 4; ++j) {
    const size_t p = 4 * (size_t)q + j;
    const unsigned char b = p < n ? s[p] : 0;
    *c |= (uint32_t)(b >> 1 & 3) << (2 * j);
    *ok |= (uint32_t)(b == 'A' || b == 'C' || b == 'G' || b == 'T') << j;
  }
}

/* ovl_find_kernel's pair: the packed pair, then blocks of 64 candidates from the top, one lane each */
static long lanes_find(const unsigned char *s1, size_t n1, const unsigned char *s2, size_t n2, int min_ov, int max_mm) {
  if (n1 > kMaxLen || n2 > kMaxLen) return -1;
  if ((int)(n1 < n2 ? n1 : n2) < min_ov) return 0;
  uint64_t *pair = static_cast<uint64_t *>(calloc(kPairWords, 8));
  if (!pair) return -3;
  for (int q = 0; q < 128; ++q) {
    uint32_t c, ok;
    pack4_host(s1, n1, q, &c, &ok);
    put_mate1(reinterpret_cast<uint8_t *>(pair), q, c, ok);
    pack4_host(s2, n2, q, &c, &ok);
    put_mate2(reinterpret_cast<uint8_t *>(pair), q, c, ok);
  }
  long best = 0;
  for (int fb = (int)(n1 + n2) - min_ov; fb >= min_ov && !best; fb -= 64) {
    const Block b = block_of((int)n1, (int)n2, min_ov, fb);
    for (int lane = 0; lane < 64 && !best; ++lane) {
      const bool mine = fb - lane >= min_ov;
      const int F = mine ? fb - lane : b.fmin;
      const int ov = ov_of((int)n1, (int)n2, F);
      const int m = matches_of(pair, F, b.wlo, b.whi);   /* (every lane computes, as on the device) */
      if (mine && ov >= min_ov && ov - m <= max_mm) best = F;
    }
  }
  free(pair);
  return best;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: ovl_main <cases.txt>", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the cases", 0);
  char *w1 = static_cast<char *>(malloc(1 << 20)), *w2 = static_cast<char *>(malloc(1 << 20));
  if (!w1 || !w2) return fail("out of memory", 0);
  long ncase = 0;
  int min_ov, max_mm;
  long long want;
  while (fscanf(f, "%d %d %1048575s %1048575s %lld", &min_ov, &max_mm, w1, w2, &want) == 5) {
    size_t n1, n2;
    unsigned char *s1 = unhex(w1, &n1), *s2 = unhex(w2, &n2);
    if (!s1 || !s2) return fail("bad mate bytes", ncase);
    const long long got = hpgq_ovl_find(s1, n1, s2, n2, min_ov, max_mm);
    if (got != want) {
      fprintf(stderr, "ovl_main: hpgq_ovl_find gives %lld, want %lld\n", got, want);
      return fail("wrong result", ncase);
    }
    if (want != -2) {
      const long lanes = lanes_find(s1, n1, s2, n2, min_ov, max_mm);
      if (lanes != want) {
        fprintf(stderr, "ovl_main: the lanes give %ld, want %lld\n", lanes, want);
        return fail("wrong result of the lane arithmetic", ncase);
      }
    }
    free(s1);
    free(s2);
    ++ncase;
  }
  free(w1);
  free(w2);
  fclose(f);
  printf("ovl_main: ok %ld cases\n", ncase);
  return 0;
}
