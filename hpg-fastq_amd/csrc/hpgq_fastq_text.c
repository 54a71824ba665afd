/*
 * hpgq_fastq_text.c — host-side record cuts and line counting over FASTQ text.
 *
 * Plain C without HIP: libhpgq links it in, and a stand-alone program can
 * compile it on its own (tests/sanitize/prefix_main.c and reader_main.c under
 * ASan + UBSan).  The CLI's reader (host/hpgq_reader.c) cuts single-end input at
 * the last whole record with hpgq_fastq_complete_prefix and its paired inputs
 * at the same record count with the other two; the line and record counters
 * validate nothing, the GPU parser does (csrc/hpgq_parse.hip).
 */
#include <string.h>

#include "hpgq.h"

/* content length of line j of a candidate record (without its '\r') */
static int64_t line_len(const char *buf, const int64_t *b, const int64_t *e, int j) {
  return (e[j] > b[j] && buf[e[j] - 1] == '\r') ? e[j] - 1 - b[j] : e[j] - b[j];
}

int64_t hpgq_fastq_complete_prefix(const char *buf, int64_t n, int at_eof) {
  if (!buf || n <= 0) return 0;
  if (at_eof) return n;
  /* from the end: the last line start '@' whose 4 lines are complete and
   * well formed ('+' third line, quality as long as the sequence) */
  for (int64_t p = n - 1; p >= 0; --p) {
    if (buf[p] != '@' || (p > 0 && buf[p - 1] != '\n')) continue;
    int64_t b[4], e[4], q = p;
    int k = 0;
    for (; k < 4; ++k) {
      const char *nl = memchr(buf + q, '\n', (size_t)(n - q));
      if (!nl) break;
      b[k] = q;
      e[k] = nl - buf;
      q = e[k] + 1;
    }
    if (k < 4) continue;   /* a partial record: look further back */
    if (buf[b[2]] == '+' && line_len(buf, b, e, 1) == line_len(buf, b, e, 3)) return e[3] + 1;
  }
  return 0;
}

int64_t hpgq_fastq_count_lines(const char *buf, int64_t n) {
  if (!buf || n <= 0) return 0;
  int64_t c = 0;
  for (int64_t i = 0; i < n; ++i) c += buf[i] == '\n';   /* (vectorised by the compiler) */
  return c;
}

int64_t hpgq_fastq_record_prefix(const char *buf, int64_t n, int64_t max_records, int64_t *records) {
  int64_t recs = 0, end = 0;
  if (buf && n > 0) {
    int64_t pos = 0;
    int lines = 0;
    while (recs < max_records) {
      const char *nl = memchr(buf + pos, '\n', (size_t)(n - pos));
      if (!nl) break;
      pos = (nl - buf) + 1;
      if (++lines == 4) {
        lines = 0;
        ++recs;
        end = pos;
      }
      if (pos >= n) break;
    }
  }
  if (records) *records = recs;
  return end;
}
