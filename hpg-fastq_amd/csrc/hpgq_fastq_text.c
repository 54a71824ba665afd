/*
 * hpgq_fastq_text.c — host-side line and record counting over FASTQ text.
 *
 * Plain C without HIP: libhpgq links it in, and a stand-alone program can
 * compile it on its own (tests/sanitize/prefix_main.c under ASan + UBSan).
 * The paired reader of the CLI cuts its two inputs at the same record count
 * with these (host/hpgq_pipeline.c); nothing here validates the format, the
 * GPU parser does (csrc/hpgq_parse.hip).
 */
#include <string.h>

#include "hpgq.h"

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
