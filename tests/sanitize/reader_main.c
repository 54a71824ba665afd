/*
 * reader_main.c — the CLI's chunk reader (hpg-fastq_amd/host/hpgq_reader.c on
 * csrc/hpgq_fastq_text.c, both HIP-free) under ASan + UBSan, as a stand-alone
 * program without a GPU: FASTQ texts of 240 records of 0 ... 300 bases (LF and
 * CRLF, bare and repeated '+' headers, quality lines that begin with '@' and
 * '+', with and without a final newline, with trailing blank lines, an empty
 * file; two mate files of different record lengths and the same pairs
 * interleaved) are written to the working directory and read back single-end,
 * as two files and interleaved, at chunk sizes from just above the longest
 * record (pair) to past the file, on 1, 3 and 4 pread threads that split every
 * read of 64 bytes or more, into heap buffers of exactly the capacity given.
 * The cuts are checked against a byte-by-byte line splitter; the pairing and
 * format errors of DESIGN.md §2.7 against their messages and pair numbers.
 * tests/test_reader_cpu.py builds and runs it.
 */
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "hpgq.h"
#include "hpgq_reader.h"

#define NREC 240
#define MAXC 4096   /* chunks per run at most */
#define SPLIT 64

static char ctx[256];   /* the case under test, for a failure's line */
static long checks;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++checks;                                              \
    if (!(cond)) {                                         \
      printf("reader_main: FAILED %s: %s: ", ctx, #cond);  \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
      exit(1);                                             \
    }                                                      \
  } while (0)

typedef struct {
  char *p;
  size_t n;
} text_t;

enum { CRLF = 1, PLUS = 2, NO_FINAL_NL = 4, BLANKS = 8 };

/* record i of mate `mate` (1, 2): mate 2's reads are a third as long, so the two
 * sides of a chunk carry different amounts */
static size_t record(char *out, int i, int mate, int flags) {
  const char *nl = flags & CRLF ? "\r\n" : "\n";
  const int len = ((i * 37 + 13) % 301) / (mate == 2 ? 3 : 1);
  char h[64], s[304], q[304];
  snprintf(h, sizeof(h), "r%d/%d len:%d", i, mate, len);
  for (int k = 0; k < len; ++k) {
    s[k] = "ACGTN"[(i + 3 * k + mate) % 5];
    q[k] = (char)('#' + (i * 7 + k * 11) % 40);
  }
  if (len && i % 5 == 1) q[0] = '@';
  if (len && i % 5 == 3) q[0] = '+';
  s[len] = q[len] = 0;
  return (size_t)sprintf(out, "@%s%s%s%s+%s%s%s%s", h, nl, s, nl, flags & PLUS ? h : "", nl, q, nl);
}

/* records [0, nrec) of one mate, or with mate 0 of both mates interleaved (2 nrec records) */
static text_t make_text(int nrec, int mate, int flags) {
  text_t t = {malloc((size_t)nrec * 2 * 800 + 64), 0};
  for (int i = 0; i < nrec; ++i)
    for (int m = 1; m <= 2; ++m)
      if (mate == 0 || mate == m) t.n += record(t.p + t.n, i, m, flags);
  if (flags & NO_FINAL_NL && t.n) t.n -= 1;   /* (CRLF: the '\r' stays, the parser's affair) */
  if (flags & BLANKS && !(flags & NO_FINAL_NL)) {
    const char *b = flags & CRLF ? "\r\n\r\n\r\n" : "\n\n\n";
    memcpy(t.p + t.n, b, strlen(b));
    t.n += strlen(b);
  }
  return t;
}

/* the reference: the end offset of every whole record (4 lines), byte by byte;
 * a last line without its newline counts as ended (the reader appends one) */
typedef struct {
  size_t *end;   /* end[r]: bytes of the first r records; end[0] = 0 */
  int64_t n;
  size_t total;  /* the text's bytes, the appended newline included */
  size_t longest;
} ends_t;

static ends_t record_ends(const text_t *t) {
  ends_t e = {malloc((t->n / 4 + 2) * sizeof(size_t)), 0, t->n, 0};
  long lines = 0;
  e.end[0] = 0;
  for (size_t i = 0; i < t->n; ++i)
    if (t->p[i] == '\n' && ++lines % 4 == 0) e.end[++e.n] = i + 1;
  if (t->n && t->p[t->n - 1] != '\n') {
    e.total = t->n + 1;
    if (++lines % 4 == 0) e.end[++e.n] = e.total;
  }
  for (int64_t r = 0; r < e.n; ++r)
    if (e.end[r + 1] - e.end[r] > e.longest) e.longest = e.end[r + 1] - e.end[r];
  return e;
}

/* records ending at offset `off`, or -1 when no record ends there */
static int64_t records_at(const ends_t *e, size_t off) {
  for (int64_t r = 0; r <= e->n; ++r)
    if (e->end[r] == off) return r;
  return -1;
}

static int open_text(const text_t *t, const char *name) {
  char path[128];
  snprintf(path, sizeof(path), "reader_main_%d_%s.fq", (int)getpid(), name);
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(t->p, 1, t->n, f) != t->n || fclose(f)) {
    printf("reader_main: cannot write %s\n", path);
    exit(1);
  }
  const int fd = open(path, O_RDONLY);
  unlink(path);
  if (fd < 0) exit(1);
  return fd;
}

/* one pass of the reader over 1 or 2 texts */
typedef struct {
  int status;          /* the last reader_next's */
  int nchunks, last;   /* chunks handed out; the last one said `last` */
  size_t end[2][MAXC]; /* bytes used per side up to and including chunk k */
  int64_t pair0[MAXC];
  int tail_err, tail_chunk;
  int64_t tail_pair;
  char tail_msg[512];
  char *cat[2];        /* the used bytes of all chunks, per side */
} run_t;

static void run_free(run_t *r) {
  free(r->cat[0]);
  free(r->cat[1]);
}

static run_t run(const text_t *t, const char *const *name, int nsides, int nmates, size_t chunk, int64_t cg,
                 int threads, size_t carry_max) {
  run_t r;
  memset(&r, 0, sizeof(r));
  reader_input_t in[2];
  char *buf[2] = {NULL, NULL};
  const size_t cap = (cg > 0 && (size_t)cg > chunk ? (size_t)cg : chunk) + carry_max;   /* as the CLI sizes its slots */
  for (int m = 0; m < nsides; ++m) {
    in[m] = (reader_input_t){open_text(&t[m], name[m]), (off_t)t[m].n, name[m]};
    buf[m] = malloc(cap);
    r.cat[m] = malloc(t[m].n + 2);
  }
  reader_t *R = NULL;
  const int rc = reader_open(&R, in, nsides, nmates, chunk, cg, threads, carry_max, SPLIT);
  CHECK(rc == HPGQ_OK && R, "reader_open %d", rc);
  size_t done[2] = {0, 0};
  while (!r.last && r.nchunks < MAXC) {
    reader_chunk_t c;
    for (int m = 0; m < nsides; ++m) memset(buf[m], 0x5a, cap);
    r.status = reader_next(R, buf, cap, &c);
    if (r.status) break;
    const int k = r.nchunks++;
    for (int m = 0; m < nsides; ++m) {
      CHECK(c.use[m] <= c.len[m] && c.len[m] <= cap, "side %d use %zu len %zu cap %zu", m, c.use[m], c.len[m], cap);
      CHECK(done[m] + c.use[m] <= t[m].n + 1, "side %d hands out more than the file", m);
      memcpy(r.cat[m] + done[m], buf[m], c.use[m]);
      done[m] += c.use[m];
      r.end[m][k] = done[m];
    }
    r.pair0[k] = c.pair0;
    r.last = c.last;
    CHECK(!c.tail_err || c.last, "a tail error before the last chunk (chunk %d)", k);
    if (c.tail_err) {
      r.tail_err = c.tail_err;
      r.tail_chunk = k;
      r.tail_pair = c.tail_pair;
      memcpy(r.tail_msg, c.tail_msg, sizeof(r.tail_msg));
    }
  }
  CHECK(r.nchunks < MAXC, "no end after %d chunks", r.nchunks);
  reader_close(R);
  for (int m = 0; m < nsides; ++m) {
    free(buf[m]);
    close(in[m].fd);
  }
  return r;
}

/* the used bytes of a side are the text's first `want` bytes (with its appended newline) */
static void check_bytes(const run_t *r, int m, const text_t *t, size_t want) {
  const size_t got = r->nchunks ? r->end[m][r->nchunks - 1] : 0;
  CHECK(got == want, "side %d: %zu bytes used, want %zu", m, got, want);
  const size_t file = want < t->n ? want : t->n;
  CHECK(memcmp(r->cat[m], t->p, file) == 0, "side %d: bytes differ from the file", m);
  if (want > t->n) CHECK(r->cat[m][t->n] == '\n', "side %d: no newline appended", m);
}

/* single-end: every byte of the file comes out, every chunk but the last ends at
 * a record end and holds a record; the last one takes the rest as it is */
static void check_single(const run_t *r, const text_t *t, const ends_t *e) {
  CHECK(r->status == HPGQ_OK && r->last && !r->tail_err, "status %d last %d tail %d", r->status, r->last, r->tail_err);
  check_bytes(r, 0, t, e->total);
  for (int k = 0; k + 1 < r->nchunks; ++k) {
    CHECK(records_at(e, r->end[0][k]) >= 0, "chunk %d ends inside a record (offset %zu)", k, r->end[0][k]);
    CHECK(r->end[0][k] > (k ? r->end[0][k - 1] : 0), "chunk %d holds no record", k);
  }
}

/* paired: every side's records come out (trailing blank lines are dropped),
 * every chunk holds the same record count on both sides (an even one of an
 * interleaved text), at least one but for the last, and pair0 is the running sum */
static void check_paired(const run_t *r, const text_t *t, const ends_t *e, int nsides) {
  CHECK(r->status == HPGQ_OK && r->last && !r->tail_err, "status %d last %d tail %d", r->status, r->last, r->tail_err);
  for (int m = 0; m < nsides; ++m) check_bytes(r, m, &t[m], e[m].end[e[m].n]);
  int64_t pairs = 0;
  for (int k = 0; k < r->nchunks; ++k) {
    const int64_t r0 = records_at(&e[0], r->end[0][k]);
    CHECK(r0 >= 0, "chunk %d ends inside a record of side 0 (offset %zu)", k, r->end[0][k]);
    if (nsides == 2) CHECK(records_at(&e[1], r->end[1][k]) == r0, "chunk %d: sides at %lld and %lld records", k,
                           (long long)r0, (long long)records_at(&e[1], r->end[1][k]));
    else CHECK(r0 % 2 == 0, "chunk %d ends after an odd record count %lld", k, (long long)r0);
    CHECK(r->pair0[k] == pairs, "chunk %d: pair0 %lld, want %lld", k, (long long)r->pair0[k], (long long)pairs);
    const int64_t now = nsides == 2 ? r0 : r0 / 2;
    CHECK(now > pairs || k + 1 == r->nchunks, "chunk %d holds no pair", k);
    pairs = now;
  }
}

/* --cg: the chunk ends are the last record end at or before each multiple of
 * the batch size B (a multiple no record ends before adds none); the batch that
 * reaches the end of the file takes the rest */
static void check_cg(const run_t *r, const text_t *t, const ends_t *e, size_t B) {
  check_single(r, t, e);
  size_t prev = 0;
  int k = 0;
  for (size_t T = B;; T += B) {
    size_t end = e->total;
    if (T < t->n) {
      int64_t q = 0;
      while (q < e->n && e->end[q + 1] <= T) ++q;
      end = e->end[q];
      if (end == prev) continue;
    }
    CHECK(k < r->nchunks && r->end[0][k] == end, "batch end %d at %zu, want %zu", k, k < r->nchunks ? r->end[0][k] : 0,
          end);
    ++k;
    prev = end;
    if (T >= t->n) break;
  }
  CHECK(k == r->nchunks, "%d chunks, want %d batches", r->nchunks, k);
}

/* a run that must end in a tail error after `pairs` good pairs have been handed out */
static void check_tail(const run_t *r, const ends_t *e, int nsides, int err, int64_t pairs, const char *msg) {
  CHECK(r->status == HPGQ_OK && r->last, "status %d last %d", r->status, r->last);
  CHECK(r->tail_err == err && r->tail_chunk == r->nchunks - 1, "tail error %d in chunk %d of %d, want %d", r->tail_err,
        r->tail_chunk, r->nchunks, err);
  const int64_t r0 = records_at(&e[0], r->end[0][r->nchunks - 1]);
  CHECK(r0 == (nsides == 2 ? pairs : 2 * pairs), "%lld records of side 0 handed out before the error, want %lld pairs",
        (long long)r0, (long long)pairs);
  if (nsides == 2) CHECK(records_at(&e[1], r->end[1][r->nchunks - 1]) == pairs, "side 1 not at %lld pairs", (long long)pairs);
  if (err == HPGQ_E_PAIRING) {
    CHECK(r->tail_pair == pairs, "pair %lld, want %lld", (long long)r->tail_pair, (long long)pairs);
    CHECK(strcmp(r->tail_msg, msg) == 0, "message '%s', want '%s'", r->tail_msg, msg);
  }
}

static const int THREADS[3] = {1, 3, 4};
static const char *const NAMES[2] = {"mate1.fq", "mate2.fq"};

int main(void) {
  const int flagsets[8] = {0, CRLF, PLUS, CRLF | PLUS, NO_FINAL_NL, CRLF | PLUS | NO_FINAL_NL, PLUS | BLANKS, CRLF | BLANKS};
  for (int fi = 0; fi < 8; ++fi) {
    const int fl = flagsets[fi];
    /* [0], [1]: the mate files; [2]: the same pairs interleaved */
    text_t t[3] = {make_text(NREC, 1, fl), make_text(NREC, 2, fl), make_text(NREC, 0, fl)};
    ends_t e[3] = {record_ends(&t[0]), record_ends(&t[1]), record_ends(&t[2])};
    CHECK(e[0].n == NREC && e[1].n == NREC && e[2].n == 2 * NREC, "the texts' own record counts");
    const size_t longest = e[0].longest, carry_max = longest + 8;
    const size_t chunks[6] = {longest + 1, 1000, 1777, 4096, 16384, t[2].n + 100};
    size_t cg_ends[MAXC];
    int cg_n = -1;
    /* (the run time goes into starting pread threads under ASan, a few per read: every chunk size
     * on 3 and 4 threads for the plain text and the one with every oddity, two sizes for the others) */
    const int all_chunks = fl == 0 || fl == (CRLF | PLUS | NO_FINAL_NL);
    for (int ci = 0; ci < 6; ++ci)
      for (int ti = 0; ti < 3 && (all_chunks || ti == 0 || ci == 1 || ci == 5); ++ti) {
        const int th = THREADS[ti];
        snprintf(ctx, sizeof(ctx), "flags %d chunk %zu threads %d single", fl, chunks[ci], th);
        run_t r = run(&t[0], NAMES, 1, 1, chunks[ci], 0, th, carry_max);
        check_single(&r, &t[0], &e[0]);
        run_free(&r);
        snprintf(ctx, sizeof(ctx), "flags %d chunk %zu threads %d two files", fl, chunks[ci], th);
        r = run(t, NAMES, 2, 2, chunks[ci], 0, th, carry_max);
        check_paired(&r, t, e, 2);
        run_free(&r);
        /* (an interleaved chunk holds a pair at least: above the longest two records) */
        const size_t ichunk = ci == 0 ? e[2].longest + e[0].longest + 1 : chunks[ci];
        snprintf(ctx, sizeof(ctx), "flags %d chunk %zu threads %d interleaved", fl, ichunk, th);
        r = run(&t[2], NAMES, 1, 2, ichunk, 0, th, carry_max);
        check_paired(&r, &t[2], &e[2], 1);
        run_free(&r);
        /* --cg batches of 5000 bytes: the same ends at every chunk size and thread count */
        snprintf(ctx, sizeof(ctx), "flags %d chunk %zu threads %d cg", fl, chunks[ci], th);
        r = run(&t[0], NAMES, 1, 1, chunks[ci], 5000, th, carry_max);
        check_cg(&r, &t[0], &e[0], 5000);
        if (cg_n < 0) {
          cg_n = r.nchunks;
          memcpy(cg_ends, r.end[0], sizeof(size_t) * (size_t)cg_n);
        }
        CHECK(r.nchunks == cg_n && memcmp(cg_ends, r.end[0], sizeof(size_t) * (size_t)cg_n) == 0,
              "the batch ends depend on the chunk size or the thread count");
        run_free(&r);
      }
    /* --cg with a batch shorter than most records: multiples without a record end are passed over */
    snprintf(ctx, sizeof(ctx), "flags %d cg batch 150", fl);
    run_t r = run(&t[0], NAMES, 1, 1, 2000, 150, 3, carry_max);
    check_cg(&r, &t[0], &e[0], 150);
    run_free(&r);

    /* ---- errors: at the smallest chunk on 1 thread (the plain text: on 3 and 4
     * too), at a large one on 4 ---- */
    for (int ci = 0; ci < 6; ci += 4)
      for (int ti = ci ? 2 : 0; ti < (ci || fl == 0 ? 3 : 1); ++ti) {
        const int th = THREADS[ti];
        char msg[256];
        /* one mate file longer by 1 and by 100 records, either one */
        for (int longer = 0; longer < 2; ++longer)
          for (int extra = 1; extra <= 100; extra += 99) {
            const int64_t shortn = NREC - extra;
            text_t u[2] = {t[0], t[1]};
            u[1 - longer] = make_text((int)shortn, 2 - longer, fl);
            ends_t ue[2] = {record_ends(&u[0]), record_ends(&u[1])};
            snprintf(ctx, sizeof(ctx), "flags %d chunk %zu threads %d side %d longer by %d", fl, chunks[ci], th, longer,
                     extra);
            snprintf(msg, sizeof(msg), "pair %lld: %s has records left after the last record of %s", (long long)shortn,
                     NAMES[longer], NAMES[1 - longer]);
            r = run(u, NAMES, 2, 2, chunks[ci], 0, th, carry_max);
            check_tail(&r, ue, 2, HPGQ_E_PAIRING, shortn, msg);
            run_free(&r);
            free(u[1 - longer].p);
            free(ue[0].end);
            free(ue[1].end);
          }
        /* an odd interleaved count: the last record dropped */
        {
          text_t u = t[2];
          u.n = e[2].end[2 * NREC - 1];
          ends_t ue = record_ends(&u);
          const size_t ichunk = ci == 0 ? e[2].longest + e[0].longest + 1 : chunks[ci];
          snprintf(ctx, sizeof(ctx), "flags %d chunk %zu threads %d odd interleaved", fl, ichunk, th);
          snprintf(msg, sizeof(msg), "pair %d: %s holds an odd number of records", NREC - 1, NAMES[0]);
          r = run(&u, NAMES, 1, 2, ichunk, 0, th, carry_max);
          check_tail(&r, &ue, 1, HPGQ_E_PAIRING, NREC - 1, msg);
          run_free(&r);
          free(ue.end);
        }
        /* a partial record (two lines) after the last pair of either mate file: format, not pairing */
        for (int side = 0; side < 2 && !(fl & (NO_FINAL_NL | BLANKS)); ++side) {
          text_t u[2] = {t[0], t[1]};
          u[side].p = malloc(t[side].n + 32);
          memcpy(u[side].p, t[side].p, t[side].n);
          memcpy(u[side].p + t[side].n, "@partial\nACGT\n", 14);
          u[side].n = t[side].n + 14;
          snprintf(ctx, sizeof(ctx), "flags %d chunk %zu threads %d partial record on side %d", fl, chunks[ci], th, side);
          r = run(u, NAMES, 2, 2, chunks[ci], 0, th, carry_max);
          check_tail(&r, e, 2, HPGQ_E_FORMAT, NREC, "");
          run_free(&r);
          free(u[side].p);
        }
      }
    /* a record longer than the chunk and its carry: a format error, after the records before it */
    if (!(fl & (NO_FINAL_NL | BLANKS))) {
      text_t u[2];
      for (int m = 0; m < 2; ++m) {
        u[m] = (text_t){malloc(t[m].n + 8192), 0};
        const size_t half = e[m].end[NREC / 2];
        memcpy(u[m].p, t[m].p, half);
        u[m].n = half + (size_t)sprintf(u[m].p + half, "@long\n%04000d\n+\n%04000d\n", 0, 0);
        memcpy(u[m].p + u[m].n, t[m].p + half, t[m].n - half);
        u[m].n += t[m].n - half;
      }
      for (int ti = 0; ti < 3; ++ti) {
        snprintf(ctx, sizeof(ctx), "flags %d threads %d long record, single", fl, THREADS[ti]);
        r = run(u, NAMES, 1, 1, longest + 1, 0, THREADS[ti], carry_max);
        CHECK(r.status == HPGQ_E_FORMAT && !r.last, "status %d", r.status);
        CHECK(r.nchunks == 0 || r.end[0][r.nchunks - 1] <= e[0].end[NREC / 2], "chunks past the long record");
        run_free(&r);
        snprintf(ctx, sizeof(ctx), "flags %d threads %d long record, two files", fl, THREADS[ti]);
        r = run(u, NAMES, 2, 2, longest + 1, 0, THREADS[ti], carry_max);
        CHECK(r.status == HPGQ_E_FORMAT && !r.last, "status %d", r.status);
        CHECK(r.nchunks > 0 && r.end[0][r.nchunks - 1] == e[0].end[NREC / 2], "the records before the long one");
        run_free(&r);
      }
      free(u[0].p);
      free(u[1].p);
    }
    for (int m = 0; m < 3; ++m) {
      free(t[m].p);
      free(e[m].end);
    }
  }

  /* an empty file: one empty last chunk; beside a mate file with records, pair 0 has no mate */
  {
    text_t t[2] = {{malloc(1), 0}, make_text(3, 2, 0)};
    ends_t e[2] = {record_ends(&t[0]), record_ends(&t[1])};
    for (int ti = 0; ti < 3; ++ti) {
      snprintf(ctx, sizeof(ctx), "empty file, threads %d", THREADS[ti]);
      run_t r = run(t, NAMES, 1, 1, 1000, 0, THREADS[ti], 512);
      check_single(&r, &t[0], &e[0]);
      CHECK(r.nchunks == 1, "%d chunks", r.nchunks);
      run_free(&r);
      r = run(t, NAMES, 1, 2, 1000, 0, THREADS[ti], 512);
      check_paired(&r, t, e, 1);
      CHECK(r.nchunks == 1, "%d chunks", r.nchunks);
      run_free(&r);
      text_t tt[2] = {t[0], t[0]};
      ends_t ee[2] = {e[0], e[0]};
      r = run(tt, NAMES, 2, 2, 1000, 0, THREADS[ti], 512);
      check_paired(&r, tt, ee, 2);
      run_free(&r);
      r = run(t, NAMES, 2, 2, 1000, 0, THREADS[ti], 512);
      check_tail(&r, e, 2, HPGQ_E_PAIRING, 0, "pair 0: mate2.fq has records left after the last record of mate1.fq");
      run_free(&r);
    }
    free(t[0].p);
    free(t[1].p);
    free(e[0].end);
    free(e[1].end);
  }
  printf("reader_main: ok %ld\n", checks);
  return 0;
}
