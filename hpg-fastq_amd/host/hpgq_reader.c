/*
 * hpgq_reader.c — the FASTQ chunk reader of the CLI (hpgq_reader.h).
 *
 * A side is one input file with its read position and its carry, the bytes
 * after the last cut.  Every chunk is the carry plus a read of the file, by up
 * to `threads` parallel pread()s, cut at a record end.  Single-end input counts
 * no lines (it delivers 40-80 GB/s); paired input counts each pread piece's
 * lines in its pread worker to cut its sides at one record count.
 */
#define _GNU_SOURCE
#include "hpgq_reader.h"

#include <errno.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "hpgq.h"

#define MAX_PREADS 64
#define MAX_PIECES (MAX_PREADS + 2)   /* the carry, the preads, a final newline */

typedef struct {
  int fd;
  off_t size, pos;
  char *carry;
  size_t carry_len;
  int64_t carry_lines;   /* '\n' bytes in the carry (paired) */
  const char *name;
} side_t;

struct reader {
  int nsides, nmates, threads;
  size_t chunk, carry_max, split_min;
  int64_t cg_batch;
  int64_t target;   /* --cg: file offset of the current chaos-game batch end */
  int64_t pairs;    /* paired: pairs handed out so far */
  side_t side[2];
};

typedef struct {
  int fd;
  char *dst;
  size_t n;
  off_t off;
  ssize_t got;
  int count;        /* paired: count the piece's lines here, in parallel */
  int64_t lines;
} pread_job_t;

static void *pread_worker(void *arg) {
  pread_job_t *j = arg;
  size_t done = 0;
  while (done < j->n) {
    ssize_t r = pread(j->fd, j->dst + done, j->n - done, j->off + (off_t)done);
    if (r < 0 && errno == EINTR) continue;
    if (r < 0) {
      j->got = -1;
      return NULL;
    }
    if (r == 0) break;
    done += (size_t)r;
  }
  j->got = (ssize_t)done;
  if (j->count) j->lines = hpgq_fastq_count_lines(j->dst, (int64_t)done);
  return NULL;
}

/* a piece of a side's buffer and the lines that end in it */
typedef struct {
  size_t off, len;
  int64_t lines;
} piece_t;

/* read up to n bytes of the side at its position with the reader threads and
 * move the position on; pc (paired): the pieces read, appended at pc[*npc],
 * each with its line count */
static ssize_t read_parallel_fd(const reader_t *R, side_t *sd, char *dst, size_t n, const char *base, piece_t *pc,
                                int *npc) {
  pthread_t th[MAX_PREADS];
  pread_job_t jobs[MAX_PREADS];
  /* one piece on this thread, or one per reader thread */
  const int k = R->threads <= 1 || n < R->split_min ? 1 : R->threads > MAX_PREADS ? MAX_PREADS : R->threads;
  const size_t per = (n + k - 1) / k;
  int started = 0;
  for (int i = 0; i < k; ++i) {
    const size_t a = (size_t)i * per;
    if (a >= n) break;
    jobs[i] = (pread_job_t){sd->fd, dst + a, (a + per > n ? n - a : per), sd->pos + (off_t)a, 0, pc != NULL, 0};
    if (k == 1) pread_worker(&jobs[i]);
    else pthread_create(&th[i], NULL, pread_worker, &jobs[i]);
    started++;
  }
  ssize_t total = 0;
  int short_read = 0, failed = 0;
  for (int i = 0; i < started; ++i) {
    if (k > 1) pthread_join(th[i], NULL);
    if (jobs[i].got < 0) failed = 1;
    if (!short_read && jobs[i].got > 0) {
      total += jobs[i].got;
      if (pc) pc[(*npc)++] = (piece_t){(size_t)(jobs[i].dst - base), (size_t)jobs[i].got, jobs[i].lines};
    }
    if (jobs[i].got < 0 || (size_t)jobs[i].got < jobs[i].n) short_read = 1;   /* EOF inside this piece */
  }
  if (failed) return -1;
  sd->pos += total;
  return total;
}

/* ---- single-end ------------------------------------------------------------ */

/* The caller's buffer filled and cut at the last whole record; with --cg at a
 * chaos-game batch end.  At EOF the rest goes to the parser as it is. */
static int next_single(reader_t *R, char *buf, size_t cap, reader_chunk_t *c) {
  side_t *sd = &R->side[0];
  memcpy(buf, sd->carry, sd->carry_len);
  size_t len = sd->carry_len;
  const off_t g0 = sd->pos - (off_t)sd->carry_len;   /* file offset of buf[0] */
  int64_t use = 0;
  int eof;
  if (R->cg_batch > 0) {
    /* the next batch end(s): the last record ending at or before target */
    for (;;) {
      R->target += R->cg_batch;
      const size_t want = (size_t)(R->target - g0) < cap - 1 ? (size_t)(R->target - g0) : cap - 1;
      if (want > len) {
        const ssize_t got = read_parallel_fd(R, sd, buf + len, want - len, buf, NULL, NULL);
        if (got < 0) return HPGQ_E_IO;
        len += (size_t)got;
      }
      eof = sd->pos >= sd->size;
      if (eof) break;
      use = hpgq_fastq_complete_prefix(buf, (int64_t)len, 0);
      if (use > 0 || len >= cap - 1) break;
      /* no record ends in this batch (one longer than the batch): the next */
    }
  } else {
    const ssize_t got = read_parallel_fd(R, sd, buf + len, cap - 1 - len, buf, NULL, NULL);   /* 1 byte for a final newline */
    if (got < 0) return HPGQ_E_IO;
    len += (size_t)got;
    eof = sd->pos >= sd->size;
  }
  if (eof && len > 0 && buf[len - 1] != '\n') buf[len++] = '\n';
  if (eof || R->cg_batch <= 0) use = hpgq_fastq_complete_prefix(buf, (int64_t)len, eof);
  if (use <= 0 && !eof) {
    fprintf(stderr, "hpg-fastq: a record longer than --chunk-mb, or not FASTQ\n");
    return HPGQ_E_FORMAT;
  }
  c->len[0] = len;
  c->use[0] = (size_t)(use > 0 ? use : 0);
  c->last = eof;
  sd->carry_len = len - c->use[0];
  if (sd->carry_len > R->carry_max) return HPGQ_E_FORMAT;
  memcpy(sd->carry, buf + c->use[0], sd->carry_len);
  return HPGQ_OK;
}

/* ---- paired ---------------------------------------------------------------- */

/* The carry and a read of this side into buf: about `chunk` bytes in all, so
 * the side with the shorter records, which carries more of them over every cut,
 * reads less the next time and its carry does not grow.  pc: the pieces (the
 * carry first), each with its line count from the pread workers. */
static int fill_side(const reader_t *R, side_t *sd, char *buf, size_t cap, size_t *len, piece_t *pc, int *npc) {
  *npc = 0;
  memcpy(buf, sd->carry, sd->carry_len);
  if (sd->carry_len) pc[(*npc)++] = (piece_t){0, sd->carry_len, sd->carry_lines};
  *len = sd->carry_len;
  size_t want = sd->carry_len < R->chunk ? R->chunk - sd->carry_len : 0;
  if (want > cap - 1 - *len) want = cap - 1 - *len;   /* 1 byte for a final newline */
  if (want > 0 && sd->pos < sd->size) {
    const ssize_t got = read_parallel_fd(R, sd, buf + *len, want, buf, pc, npc);
    if (got < 0) return HPGQ_E_IO;
    *len += (size_t)got;
    if (got == 0) sd->size = sd->pos;   /* (the file shrank: its end is here) */
  }
  if (sd->pos >= sd->size && *len > 0 && buf[*len - 1] != '\n') {   /* the last line lacks its newline */
    buf[(*len)++] = '\n';
    pc[(*npc)++] = (piece_t){*len - 1, 1, 1};
  }
  return 0;
}

/* bytes of the first n records of buf, n <= the whole records in it: the pieces'
 * line counts lead to the last piece that starts before record n's end, and
 * hpgq_fastq_record_prefix counts on from the record start that follows it */
static size_t cut_records(const char *buf, size_t len, const piece_t *pc, int npc, int64_t n) {
  size_t anchor = 0;
  int64_t before = 0, lines = 0;   /* whole records before the anchor; lines before piece p */
  for (int p = 1; p < npc; ++p) {
    lines += pc[p - 1].lines;
    if ((lines + 3) / 4 >= n) break;
    /* piece p starts inside line `lines`: (4 - lines % 4) % 4 newlines on, record ceil(lines / 4)
     * starts; with lines % 4 == 0 the piece starts inside that record's first line, which counts
     * the same for hpgq_fastq_record_prefix (it looks at newlines only) */
    size_t a = pc[p].off;
    for (int k = (int)((4 - lines % 4) % 4); k > 0 && a < len; --k) {
      const char *nl = memchr(buf + a, '\n', len - a);
      a = nl ? (size_t)(nl - buf) + 1 : len;
    }
    anchor = a;
    before = (lines + 3) / 4;
  }
  int64_t got = 0;
  return anchor + (size_t)hpgq_fastq_record_prefix(buf + anchor, (int64_t)(len - anchor), n - before, &got);
}

static int blank_only(const char *p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i] != '\n' && p[i] != '\r') return 0;
  return 1;
}

static int64_t piece_lines(const piece_t *pc, int npc) {
  int64_t t = 0;
  for (int p = 0; p < npc; ++p) t += pc[p].lines;
  return t;
}

/* Two files: a chunk of each, each with its own carry, both cut at n = min(whole
 * records in either); the rest of each side is carried.  Interleaved: one file,
 * cut at an even record count.  At the end every side must be at EOF with
 * nothing carried; otherwise the pairing error names the file that has records
 * left. */
static int next_paired(reader_t *R, char *const buf[2], size_t cap, reader_chunk_t *c) {
  const int ns = R->nsides;
  piece_t pc[2][MAX_PIECES];
  int npc[2] = {0, 0}, eof[2] = {1, 1};
  int64_t lines[2] = {0, 0}, rec[2] = {0, 0};
  for (int m = 0; m < ns; ++m) {
    const int rc = fill_side(R, &R->side[m], buf[m], cap, &c->len[m], pc[m], &npc[m]);
    if (rc) return rc;
    eof[m] = R->side[m].pos >= R->side[m].size;
    lines[m] = piece_lines(pc[m], npc[m]);
    rec[m] = lines[m] / 4;
  }
  /* records per side in this chunk */
  const int64_t n = ns == 2 ? (rec[0] < rec[1] ? rec[0] : rec[1]) : rec[0] & ~(int64_t)1;
  const int any_eof = eof[0] || (ns == 2 && eof[1]);
  const int last = (eof[0] && eof[1]) || (n == 0 && any_eof);
  if (n == 0 && !last) {
    fprintf(stderr, "hpg-fastq: a record longer than --chunk-mb, or not FASTQ\n");
    return HPGQ_E_FORMAT;
  }
  for (int m = 0; m < ns; ++m) {
    side_t *sd = &R->side[m];
    c->use[m] = n > 0 ? cut_records(buf[m], c->len[m], pc[m], npc[m], n) : 0;
    sd->carry_len = c->len[m] - c->use[m];
    sd->carry_lines = lines[m] - 4 * n;
    memcpy(sd->carry, buf[m] + c->use[m], sd->carry_len);
  }
  c->last = last;
  c->pair0 = R->pairs;
  R->pairs += ns == 2 ? n : n / 2;
  /* at the end nothing may be left on either side (blank lines aside); the
   * caller raises the error after the chunk's own pairs have gone to a worker,
   * whose name check may find an earlier bad pair */
  for (int m = 0; last && m < ns && !c->tail_err; ++m) {
    const side_t *sd = &R->side[m];
    if (sd->pos >= sd->size && blank_only(sd->carry, sd->carry_len)) continue;
    if (rec[m] > n || sd->pos < sd->size) {   /* whole records without a mate */
      if (ns == 2)
        snprintf(c->tail_msg, sizeof(c->tail_msg), "pair %lld: %s has records left after the last record of %s",
                 (long long)R->pairs, sd->name, R->side[1 - m].name);
      else
        snprintf(c->tail_msg, sizeof(c->tail_msg), "pair %lld: %s holds an odd number of records",
                 (long long)R->pairs, sd->name);
      c->tail_err = HPGQ_E_PAIRING;
      c->tail_pair = R->pairs;
    } else {   /* a partial record at the end of the file */
      c->tail_err = HPGQ_E_FORMAT;
    }
  }
  return HPGQ_OK;
}

/* ---- open / next / close ----------------------------------------------------- */

int reader_open(reader_t **out, const reader_input_t *in, int nsides, int nmates, size_t chunk, int64_t cg_batch,
                int threads, size_t carry_max, size_t split_min) {
  *out = NULL;
  if (nsides < 1 || nsides > nmates || nmates > 2 || (cg_batch > 0 && nmates != 1)) return HPGQ_E_INVALID;
  reader_t *R = calloc(1, sizeof(*R));
  if (!R) return HPGQ_E_NOMEM;
  *R = (reader_t){.nsides = nsides, .nmates = nmates, .threads = threads, .chunk = chunk, .carry_max = carry_max,
                  .split_min = split_min, .cg_batch = cg_batch};
  for (int m = 0; m < nsides; ++m) {
    R->side[m] = (side_t){in[m].fd, in[m].size, 0, NULL, 0, 0, in[m].name};
    /* (a paired side carries whole records the other side had no mates for yet: up to a chunk) */
    R->side[m].carry = malloc((nmates == 2 ? chunk : 0) + carry_max + 16);
    if (!R->side[m].carry) {
      reader_close(R);
      return HPGQ_E_NOMEM;
    }
  }
  *out = R;
  return HPGQ_OK;
}

int reader_next(reader_t *R, char *const buf[2], size_t cap, reader_chunk_t *out) {
  memset(out, 0, sizeof(*out));
  return R->nmates == 2 ? next_paired(R, buf, cap, out) : next_single(R, buf[0], cap, out);
}

void reader_close(reader_t *R) {
  if (!R) return;
  free(R->side[0].carry);
  free(R->side[1].carry);
  free(R);
}
