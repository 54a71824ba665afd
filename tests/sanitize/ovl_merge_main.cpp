/*
 * ovl_merge_main.cpp — `edit --merge-overlap` without a GPU, under ASan + UBSan:
 * hpgq_ovl_merge (csrc/hpgq_ovl_post.cpp), and the arithmetic
 * of the merge kernel's lanes (merge4, csrc/hpgq_ovl_lane.h) walked on the host,
 * four positions at a time as ovl_merge_kernel does, against the same bytes.
 * Built and run by tests/test_ovl_merge_cpu.py.
 *
 * argv[1]: a text file, one case per line:
 *   s1_hex q1_hex s2_hex q2_hex F want_return merged_hex quality_hex resolved1 resolved2
 * ("-": no bytes).  The mates and both outputs are heap blocks of their exact
 * size (the outputs: F bytes), so an access past them is caught.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hpgq.h"
#include "../../hpg-fastq_amd/csrc/hpgq_ovl_lane.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "ovl_merge_main: %s (case %ld)\n", what, line);
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

/* ovl_merge_kernel's lanes: positions p .. p + 3, mate 1's bytes zeroed from hi on (lane_bytes), the facing bytes
 * of mate 2 where there are any and, where there are none, what a neighbouring read may hold at its worst: a base
 * at the highest quality byte */
static int lanes_merge(const unsigned char *s1, const unsigned char *q1, size_t n1, const unsigned char *s2,
                       const unsigned char *q2, size_t n2, long long F, const unsigned char *m, const unsigned char *qm,
                       unsigned r1, unsigned r2) {
  const long long lo = F > (long long)n2 ? F - (long long)n2 : 0, hi = (long long)n1 < F ? (long long)n1 : F;
  unsigned won1 = 0, won2 = 0;
  for (long long p = 0; p < F + 3; p += 4) {   /* (one group more: the kernel's extra step computes past F too) */
    uint32_t b1 = 0, p1 = 0, b2 = 0, p2 = 0;
    for (int t = 0; t < 4; ++t) {
      const long long pt = p + t, j = F - 1 - pt;
      if (pt < hi) {
        b1 |= (uint32_t)s1[pt] << (8 * t);
        p1 |= (uint32_t)q1[pt] << (8 * t);
      }
      const bool have = j >= 0 && j < (long long)n2;
      b2 |= (uint32_t)(have ? s2[j] : 'A') << (8 * t);
      p2 |= (uint32_t)(have ? q2[j] : 0xFF) << (8 * t);
    }
    const hpgq::ovl::Merged4 r = hpgq::ovl::merge4(b1, p1, b2, p2, (int)(hi - p), (int)(lo - p));
    for (int t = 0; t < 4 && p + t < F; ++t)
      if ((r.seq >> (8 * t) & 255u) != m[p + t] || (r.qual >> (8 * t) & 255u) != qm[p + t]) return 1;
    if (p < F) {
      won1 += r.won1;
      won2 += r.won2;
    }
  }
  return won1 != r1 || won2 != r2 ? 2 : 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: ovl_merge_main <cases.txt>", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the cases", 0);
  enum { W = 4096 };
  char w[6][W];
  long ncase = 0;
  long long F, want;
  unsigned r1, r2;
  while (fscanf(f, "%4095s %4095s %4095s %4095s %lld %lld %4095s %4095s %u %u", w[0], w[1], w[2], w[3], &F, &want, w[4], w[5],
                &r1, &r2) == 10) {
    size_t n[6];
    unsigned char *b[6];
    for (int k = 0; k < 6; ++k)
      if (!(b[k] = unhex(w[k], &n[k]))) return fail("bad bytes", ncase);
    if (n[0] != n[1] || n[2] != n[3] || n[4] != n[5]) return fail("a quality is as long as its sequence", ncase);
    const size_t nout = want > 0 ? (size_t)want : 0;
    if (n[4] != nout) return fail("the wanted read has the wanted length", ncase);
    unsigned char *m = static_cast<unsigned char *>(malloc(nout ? nout : 1));
    unsigned char *qm = static_cast<unsigned char *>(malloc(nout ? nout : 1));
    if (!m || !qm) return fail("out of memory", ncase);
    uint32_t res[2] = {77, 77};
    const long long got = hpgq_ovl_merge(b[0], b[1], n[0], b[2], b[3], n[2], F, m, qm, res);
    if (got != want) {
      fprintf(stderr, "ovl_merge_main: hpgq_ovl_merge gives %lld, want %lld\n", got, want);
      return fail("wrong result", ncase);
    }
    if (want >= 0) {
      if (memcmp(m, b[4], nout) || memcmp(qm, b[5], nout)) return fail("wrong merged bytes", ncase);
      if (res[0] != r1 || res[1] != r2) return fail("wrong resolved counts", ncase);
      /* resolved may be NULL */
      if (hpgq_ovl_merge(b[0], b[1], n[0], b[2], b[3], n[2], F, m, qm, NULL) != want) return fail("wrong result without counts", ncase);
      if (want > 0 && lanes_merge(b[0], b[1], n[0], b[2], b[3], n[2], F, b[4], b[5], r1, r2))
        return fail("wrong result of the lane arithmetic", ncase);
    }
    for (int k = 0; k < 6; ++k) free(b[k]);
    free(m);
    free(qm);
    ++ncase;
  }
  fclose(f);
  printf("ovl_merge_main: ok %ld cases\n", ncase);
  return 0;
}
