/*
 * hpgq_reader.h — the FASTQ chunk reader of the CLI, without the pipeline.
 *
 * Reads one input (single-end, or an interleaved file) or two (--fq1 + --fq2)
 * with parallel pread()s into buffers the caller owns and cuts every chunk at a
 * record end; what follows the cut is carried into the next chunk, per side.
 * Plain C on hpgq.h's HIP-free text functions: no slots, no locks, no GPU, so
 * a stand-alone program drives it (tests/sanitize/reader_main.c).
 */
#ifndef HPGQ_READER_H
#define HPGQ_READER_H

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

/* one input: an open descriptor (the caller's), its size and its name for the
 * pairing messages */
typedef struct {
  int fd;
  off_t size;
  const char *name;
} reader_input_t;

typedef struct {
  size_t len[2];       /* bytes in buf[m] */
  size_t use[2];       /* the chunk: whole records, buf[m][0, use[m]) */
  int last;            /* the last chunk of the input */
  int64_t pair0;       /* paired: whole-input number of the chunk's first pair */
  /* an error found at the end of the input, to be raised after
   * this chunk has been handed on: 0, HPGQ_E_PAIRING with its line and pair
   * number, or HPGQ_E_FORMAT (a partial record at the end of a mate file) */
  int tail_err;
  int64_t tail_pair;
  char tail_msg[512];
} reader_chunk_t;

typedef struct reader reader_t;

/* nsides inputs holding nmates mates (1 + 1 single-end, 1 + 2 interleaved,
 * 2 + 2 two mate files).  chunk: the bytes a paired side holds per chunk, carry
 * included (single-end input fills the caller's buffer).  cg_batch > 0
 * (single-end): every chunk ends at the last record end at or before the next
 * multiple of cg_batch.  threads: pread threads; a read below split_min bytes is
 * not split over them.  carry_max: the longest partial record single-end input
 * may carry over a cut.  HPGQ_OK, HPGQ_E_INVALID or HPGQ_E_NOMEM. */
int reader_open(reader_t **R, const reader_input_t *in, int nsides, int nmates, size_t chunk, int64_t cg_batch,
                int threads, size_t carry_max, size_t split_min);

/* The next chunk into buf[0 .. nsides), each of cap >= chunk + carry_max bytes.
 * HPGQ_OK with *out filled, HPGQ_E_IO, or HPGQ_E_FORMAT (no whole record in a
 * full chunk, said on stderr; or a carry above carry_max).  Not to be called
 * again after an error or a chunk with `last` set. */
int reader_next(reader_t *R, char *const buf[2], size_t cap, reader_chunk_t *out);

void reader_close(reader_t *R);

#endif
