/*
 * prefix_main.c — hpgq_fastq_record_prefix / hpgq_fastq_count_lines
 * (hpg-fastq_amd/csrc/hpgq_fastq_text.c, HIP-free) under ASan + UBSan, as a
 * stand-alone program: every cut point of a 25-record text (LF and CRLF, bare
 * and repeated '+' headers, quality lines that begin with '@' and with '+')
 * for max_records in {0, 1, 3, 10^9}, against a byte-by-byte line splitter.
 * Each prefix is copied into a heap block of exactly its size, so a read past
 * the end is an ASan error.  tests/test_pairing_cpu.py builds and runs it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq.h"

static const char *SEQ[5] = {"ACGT", "", "NNACG", NULL, "GATTACA"};
static const char *QUAL[5] = {"IIII", "", "@@@@@", NULL, "+5+5+5+"};

static size_t build(char *out, int crlf, int plus_header) {
  const char *nl = crlf ? "\r\n" : "\n";
  char a50[51], q50[51];
  memset(a50, 'A', 50);
  a50[50] = 0;
  memset(q50, 'I', 50);
  q50[0] = '@';
  q50[50] = 0;
  size_t n = 0;
  for (int i = 0; i < 25; ++i) {
    const char *s = SEQ[i % 5] ? SEQ[i % 5] : a50, *q = QUAL[i % 5] ? QUAL[i % 5] : q50;
    char h[64];
    snprintf(h, sizeof(h), "r%d extra:%d", i, i % 7);
    n += (size_t)sprintf(out + n, "@%s%s%s%s+%s%s%s%s", h, nl, s, nl, plus_header ? h : "", nl, q, nl);
  }
  return n;
}

/* the reference: bytes and count of the first min(maxrec, whole records) records */
static long ref_prefix(const char *t, long n, long maxrec, long *recs) {
  long lines = 0, end = 0, r = 0;
  for (long i = 0; i < n && r < maxrec; ++i)
    if (t[i] == '\n' && ++lines % 4 == 0) {
      ++r;
      end = i + 1;
    }
  *recs = r;
  return end;
}

int main(void) {
  static char text[8192];
  const long maxes[4] = {0, 1, 3, 1000000000L};
  long checks = 0;
  for (int crlf = 0; crlf < 2; ++crlf)
    for (int ph = 0; ph < 2; ++ph) {
      const long len = (long)build(text, crlf, ph);
      for (long n = 0; n <= len; ++n) {
        char *cut = malloc(n ? (size_t)n : 1);   /* exactly n readable bytes */
        memcpy(cut, text, (size_t)n);
        long nl = 0;
        for (long i = 0; i < n; ++i) nl += cut[i] == '\n';
        if (hpgq_fastq_count_lines(cut, n) != nl) {
          printf("count_lines: crlf %d plus %d n %ld\n", crlf, ph, n);
          return 1;
        }
        for (int k = 0; k < 4; ++k) {
          long want_r = 0;
          const long want = ref_prefix(cut, n, maxes[k], &want_r);
          int64_t got_r = -1;
          const int64_t got = hpgq_fastq_record_prefix(cut, n, maxes[k], &got_r);
          if (got != want || got_r != want_r || hpgq_fastq_record_prefix(cut, n, maxes[k], NULL) != want) {
            printf("record_prefix: crlf %d plus %d n %ld max %ld: got %lld / %lld, want %ld / %ld\n", crlf, ph, n,
                   maxes[k], (long long)got, (long long)got_r, want, want_r);
            return 1;
          }
          ++checks;
        }
        free(cut);
      }
    }
  int64_t r = 7;
  if (hpgq_fastq_record_prefix(NULL, 0, 5, &r) != 0 || r != 0 || hpgq_fastq_count_lines(NULL, 0) != 0) return 1;
  printf("prefix_main: ok %ld\n", checks);
  return 0;
}
