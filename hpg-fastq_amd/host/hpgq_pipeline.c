/*
 * hpgq_pipeline.c — producer -> GPU worker -> consumer for hpg-fastq on libhpgq.
 *
 * The reference runs producer (fastq_fread_se into 10,000-read batches),
 * worker threads (bioinfo-libs filter / stats / edit) and an ordered consumer
 * (merge or write), src/stats_fastq.c:174-250, src/filter_fastq.c:106-174,
 * src/edit_fastq.c:113-206.  Here:
 *   reader     one thread fills page-locked chunks of FASTQ text (--chunk-mb)
 *              through hpgq_reader.c: --num-threads parallel pread()s, every
 *              chunk cut at a record end and the rest carried into the next
 *              one.  Single-end input is one side holding one mate.
 *   GPU        --gpu-workers threads per GPU (default 2: one copies a chunk
 *              in while the other's kernels run) on --gpus devices (default
 *              every visible one), chunk k on worker k mod G: hpgq_parse_host (H2D +
 *              parse into a device batch) and hpgq_run_device (filter / edit /
 *              stats fused) on the worker's ctx stream; for filter / edit the
 *              mask, trims and record offsets come back.  At the end the
 *              workers' device counters (k-mer tables, CGR tables) are summed
 *              on the host: the read-sharded merge of DESIGN.md §6.
 *   --cg       one chaos_game_fill_tables call per batch of --cg-batch-size
 *              bytes of FASTQ text (default 64,000,000, the old tool's
 *              batch_size, old/main_hpg_fastq_old.c:116): batch j holds the
 *              records ending in ((j-1)B, jB], so the calls (whose double
 *              state starts afresh, old/chaos_game.c:180-181) do not depend on
 *              --chunk-mb or --gpus; the reader then cuts every chunk at a
 *              batch end.
 *   outputs    (filter / edit) passed.fq / failed.fq / edit.fq in input
 *              order: filter copies whole input records; edit writes the
 *              header and '+' lines as read and the trimmed sequence /
 *              quality.  Regular output files are mapped shared, sized to the
 *              bound (each output is at most the input), and every chunk is
 *              placed in input order from its per-class byte counts and then
 *              copied into the maps by its worker's copy threads in parallel
 *              (one writer thread through write() capped filter at 18 and edit
 *              at 15-17 Mreads/s: a tmpfs or page-cache file takes one write()
 *              at a time, page stores from many threads at once); the files
 *              are truncated to their final sizes at the end.  Otherwise
 *              (--stream-writer, or a map that fails) one writer thread
 *              writes the chunks in order.
 *   paired     (--fq1 + --fq2, or --interleaved -f) two mates
 *              on two sides or on one: the reader fills a second page-locked
 *              text per chunk for --fq2 and cuts both texts at the same record
 *              count (an interleaved text at an even one); the worker parses
 *              both mates (or splits the interleaved text on the device),
 *              checks the mate names (hpgq_parse_pair_check) and makes one
 *              engine call over the pairs; the stream writer writes
 *              passed_1/_2, failed_1/_2 (edit_1/_2).  A pair out of step ends
 *              the run with its number over the whole input.
 * Stats never leave the device until the end (hpgq_read_counters).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/statvfs.h>
#include <sys/uio.h>
#include <time.h>
#include <unistd.h>

#include "hpgq_cli.h"
#include "hpgq_mapout.h"
#include "hpgq_reader.h"

#define MAX_WORKERS 16
#define MAX_SLOTS (2 * MAX_WORKERS + 2)
#define MAX_CARRY (64u << 20)    /* longest record the reader can carry over */
#define SPLIT_MIN (4u << 20)     /* a read below this is one pread, not --num-threads */
#define TRACE_MAX 1024

typedef struct {
  char *buf;          /* page-locked */
  size_t cap, use;
  int state;          /* 0 free, 1 filled (reader -> GPU), 2 processed (GPU -> writer) */
  int64_t chunk;      /* the chunk it holds */
  /* GPU results for the writer */
  int64_t nreads;
  uint8_t *mask;
  uint32_t *trim, *rec_start, *seq_start, *plus_start, *qual_start;
  int32_t *idx;
  size_t res_cap;
  /* paired input: mate 2's text (--fq2; interleaved mates share buf) and the
   * whole-input number of the chunk's first pair.  The results then hold both
   * mates (mate_view): trim and idx one mate after the other, the record
   * offsets per text */
  char *buf2;
  size_t use2;
  int64_t pair0;
  /* edit: the chunk's output records per mate and class ([2 m + c]; c: 0
   * edit.fq / passed, 1 failed), assembled by the GPU worker so the writer only
   * writes them in order */
  char *out[6];       /* ([4], [5]: --merge-overlap's merged reads, edit_merged.fq / failed_merged.fq) */
  size_t out_cap[6], out_len[6];
  uint64_t out_n[6];
  /* mapped outputs: this chunk's copy parts (copy_part_t[MAX_COPIERS]) and
   * how many are still being copied (state 3 until the last one is done) */
  void *parts;
  int parts_left;
} slot_t;

typedef struct {
  const cli_options_t *o;
  reader_t *rd;
  int nslots, nworkers;
  slot_t slot[MAX_SLOTS];
  pthread_mutex_t mu;
  pthread_cond_t cv;
  int reader_done, error;
  int64_t chunks;
  /* the mates (2: paired input) and the texts per chunk they come in (2:
   * --fq2); the output files per mate and class ([2 m + c] like slot_t.out:
   * passed / edit, failed; NULL: not written) and the first pair out of step */
  int nmates, nsides;
  FILE *out[6];          /* ([4], [5]: edit_merged.fq, failed_merged.fq) */
  uint64_t written_pass, written_fail;
  int64_t bad_pair, bad_chunk;
  char pairing_msg[512];
  /* mapped outputs: [0] passed / edit.fq, [1] failed.fq (NULL: not written) */
  int mmap_out;
  mapout_t mo;           /* the mappings: reservation, prefault threads, SIGBUS guard */
  char *map[2];          /* (= mo.map) */
  size_t map_cap;
  uint64_t out_off[2];   /* bytes placed so far per output */
  int64_t placed;        /* chunks placed (in input order) */
  /* the copy pool: placed chunks' parts, copied into the maps by --num-threads
   * copier threads while the GPU workers go on with the next chunks */
  void **cq;             /* ring of copy_part_t * */
  int cq_cap, cq_head, cq_tail, cq_exit, ncopiers;
  pthread_mutex_t cq_mu;
  pthread_cond_t cq_cv;
  int copies_pending;    /* slots in state 3 (under mu) */
  pthread_t copier[64];
  /* HPGQ_TRACE=1: per chunk (the first TRACE_MAX) the reader's and the worker's
   * start / end times, printed to stderr at the end (diagnostics only) */
  int trace;
  double t0;
  /* read start, read end, worker start, sync start, worker end, parsed,
   * synced, placed */
  double tr[TRACE_MAX][8];
  int tw[TRACE_MAX];
} pipe_t;

static double now_s(void);
static void trace_at(pipe_t *P, int64_t k, int i, int w) {
  if (!P->trace || k >= TRACE_MAX) return;
  P->tr[k][i] = now_s() - P->t0;
  if (w >= 0) P->tw[k] = w;
}

static double now_s(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

/* ---- NUMA placement --------------------------------------------------------- */

/* Run this process's threads (reader, GPU workers, writer -- created after
 * this call, so they inherit it) on the CPUs of the GPUs' NUMA node, within
 * the CPUs it may use, and so allocate the page-locked chunks there (first
 * touch): the reader's copies and the chunks' H2D stay on the GPU's side of
 * the socket link.  Skipped when the GPUs sit on different nodes, the node is
 * unknown, or it holds none of the allowed CPUs. */
static void bind_numa(const cli_options_t *o, int ngpus, int ndev) {
  int node = -2;
  for (int g = 0; g < ngpus && g < ndev; ++g) {
    const int nd = hpgq_device_numa_node((o->device + g) % ndev);
    if (nd < 0 || (node != -2 && nd != node)) return;
    node = nd;
  }
  if (node < 0) return;
  char path[96], list[4096];
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  FILE *f = fopen(path, "r");
  if (!f) return;
  const int ok = fgets(list, sizeof(list), f) != NULL;
  fclose(f);
  if (!ok) return;
  cpu_set_t allowed, want;
  if (sched_getaffinity(0, sizeof(allowed), &allowed)) return;
  CPU_ZERO(&want);
  for (char *p = list; *p && *p != '\n';) {   /* "a-b,c,d-e" */
    char *e;
    long a = strtol(p, &e, 10), b = a;
    if (e == p) break;
    if (*e == '-') b = strtol(e + 1, &e, 10);
    for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
      if (CPU_ISSET((int)c, &allowed)) CPU_SET((int)c, &want);
    p = *e == ',' ? e + 1 : e;
  }
  if (CPU_COUNT(&want) == 0) return;
  if (sched_setaffinity(0, sizeof(want), &want) == 0 && getenv("HPGQ_TRACE"))
    fprintf(stderr, "hpg-fastq: threads on NUMA node %d (%d CPUs)\n", node, CPU_COUNT(&want));
}

/* ---- reader ------------------------------------------------------------- */

static void reader_fail(pipe_t *P, int code) {
  pthread_mutex_lock(&P->mu);
  P->error = code;
  pthread_cond_broadcast(&P->cv);
  pthread_mutex_unlock(&P->mu);
}

/* A pairing error: keeps the lowest pair number reported, so
 * that workers on different chunks agree on the first bad pair. */
static void pairing_fail(pipe_t *P, int64_t chunk, int64_t pair, const char *msg) {
  pthread_mutex_lock(&P->mu);
  if (P->bad_pair < 0 || pair < P->bad_pair) {
    P->bad_pair = pair;
    P->bad_chunk = chunk;
    snprintf(P->pairing_msg, sizeof(P->pairing_msg), "%s", msg);
  }
  if (!P->error) P->error = HPGQ_E_PAIRING;
  pthread_cond_broadcast(&P->cv);
  pthread_mutex_unlock(&P->mu);
}

/* Chunk k into slot k mod nslots once it is free.  An error at the end of the
 * input is raised after the last chunk is published: its pairs go to a worker,
 * whose name check may find an earlier bad pair. */
static void *reader_main(void *arg) {
  pipe_t *P = arg;
  for (int64_t k = 0;; ++k) {
    slot_t *s = &P->slot[k % P->nslots];
    pthread_mutex_lock(&P->mu);
    while (s->state != 0 && !P->error) pthread_cond_wait(&P->cv, &P->mu);
    const int err = P->error;
    pthread_mutex_unlock(&P->mu);
    if (err) break;
    trace_at(P, k, 0, -1);
    char *const buf[2] = {s->buf, s->buf2};
    reader_chunk_t c;
    const int rc = reader_next(P->rd, buf, s->cap, &c);
    if (rc) {
      reader_fail(P, rc);
      break;
    }
    s->use = c.use[0];
    s->use2 = c.use[1];
    s->pair0 = c.pair0;
    trace_at(P, k, 1, -1);
    pthread_mutex_lock(&P->mu);
    s->chunk = k;
    s->state = 1;
    P->chunks = k + 1;
    if (c.last) P->reader_done = 1;
    pthread_cond_broadcast(&P->cv);
    pthread_mutex_unlock(&P->mu);
    if (c.tail_err == HPGQ_E_PAIRING) pairing_fail(P, k + 1, c.tail_pair, c.tail_msg);
    else if (c.tail_err) reader_fail(P, c.tail_err);
    if (c.last) break;
  }
  pthread_mutex_lock(&P->mu);
  P->reader_done = 1;
  pthread_cond_broadcast(&P->cv);
  pthread_mutex_unlock(&P->mu);
  return NULL;
}

/* ---- writer ------------------------------------------------------------- */

/* One mate's records in a processed slot.  Record i of the mate is record
 * r = first + i * stride of its text (rs / ss / ps / qs: the record, sequence,
 * '+' line and quality offsets of the text's `total` records); its trim and
 * data_indices are at [i].  Single-end input is mate 0 with stride 1. */
typedef struct {
  const char *buf;
  size_t use;
  const uint32_t *rs, *ss, *ps, *qs, *trim;
  const int32_t *idx;
  int64_t total;
  int first, stride;
  FILE *f[2];   /* its outputs: [0] passed / edit, [1] failed */
} mate_view_t;

static mate_view_t mate_view(const pipe_t *P, const slot_t *s, int m) {
  const int64_t n = s->nreads;
  mate_view_t v = {s->buf, s->use, s->rec_start, s->seq_start, s->plus_start, s->qual_start, s->trim, s->idx,
                   n, 0, 1, {P->out[2 * m], P->out[2 * m + 1]}};
  if (P->nmates == 2) {
    v.trim = s->trim + (size_t)m * n;
    v.idx = s->idx + (size_t)m * (n + 1);
    if (P->nsides == 1) {   /* interleaved: records 2 i + m of the one text */
      v.total = 2 * n;
      v.first = m;
      v.stride = 2;
    } else if (m) {         /* mate 2's own text; its offsets follow mate 1's */
      v.buf = s->buf2;
      v.use = s->use2;
      v.rs += n, v.ss += n, v.ps += n, v.qs += n;
    }
  }
  return v;
}

static int write_span(FILE *f, const char *p, size_t n) { return fwrite(p, 1, n, f) == n ? 0 : -1; }

/* the spans of one output class, flushed by writev (the stream is drained
 * first: nothing of it is buffered in stdio across these calls) */
#define SPAN_IOV 1024
typedef struct {
  FILE *f;
  struct iovec v[SPAN_IOV];
  int n;
} spans_t;

static int spans_flush(spans_t *S) {
  int k = 0;
  while (k < S->n) {
    const int cnt = S->n - k;
    const ssize_t w = writev(fileno(S->f), S->v + k, cnt);
    if (w < 0) {
      if (errno == EINTR) continue;
      return -1;
    }
    size_t left = (size_t)w;   /* partial write: skip the whole iovecs, trim the next */
    while (k < S->n && left >= S->v[k].iov_len) left -= S->v[k++].iov_len;
    if (k < S->n) {
      S->v[k].iov_base = (char *)S->v[k].iov_base + left;
      S->v[k].iov_len -= left;
    }
  }
  S->n = 0;
  return 0;
}

static int spans_add(spans_t *S, const char *p, size_t n) {
  if (S->n && (const char *)S->v[S->n - 1].iov_base + S->v[S->n - 1].iov_len == p) {   /* contiguous */
    S->v[S->n - 1].iov_len += n;
    return 0;
  }
  if (S->n == SPAN_IOV && spans_flush(S)) return -1;
  S->v[S->n].iov_base = (void *)p;
  S->v[S->n].iov_len = n;
  S->n++;
  return 0;
}

static int write_slot(pipe_t *P, slot_t *s) {
  const int edit = P->o->command == CMD_EDIT;
  const int filter_on = P->o->filter_on;
  if (edit) {   /* the worker assembled the trimmed records (assemble_edit) */
    for (int m = 0; m < P->nmates; ++m) {
      const mate_view_t v = mate_view(P, s, m);
      for (int c = 0; c < 2; ++c)
        if (v.f[c] && s->out_len[2 * m + c] && write_span(v.f[c], s->out[2 * m + c], s->out_len[2 * m + c]))
          return -1;
    }
    for (int c = 4; c < 6; ++c)   /* (--merge-overlap: the merged reads) */
      if (P->out[c] && s->out_len[c] && write_span(P->out[c], s->out[c], s->out_len[c])) return -1;
    P->written_pass += s->out_n[0];
    P->written_fail += s->out_n[1];
    return 0;
  }
  /* whole input records, consecutive records of one class as one span, the
   * spans of each class gathered into writev calls of up to SPAN_IOV spans
   * (one write per span -- ~5 KB at 6 % failed reads -- ran at 4 GB/s into
   * tmpfs, which takes 8.6 GB/s in 64 KB writes) */
  static __thread spans_t S[2];
  for (int m = 0; m < P->nmates; ++m) {
    const mate_view_t v = mate_view(P, s, m);
    S[0].f = v.f[0];
    S[1].f = v.f[1];   /* (without a filter every record is class 0) */
    for (int c = 0; c < 2; ++c) {
      S[c].n = 0;
      if (S[c].f && fflush(S[c].f)) return -1;
    }
    for (int64_t i = 0; i < s->nreads; ++i) {
      const int pass = s->mask[i] != 0;
      spans_t *sp = &S[pass || !filter_on ? 0 : 1];
      int64_t j = i + 1;   /* (interleaved mates: the other mate's record lies between) */
      while (v.stride == 1 && j < s->nreads && (s->mask[j] != 0) == pass) ++j;
      if (sp->f) {
        const int64_t r0 = v.first + i * v.stride, r1 = v.first + (j - 1) * v.stride + 1;
        const uint32_t a = v.rs[r0];
        const uint32_t ee = r1 < v.total ? v.rs[r1] : (uint32_t)v.use;
        if (spans_add(sp, v.buf + a, ee - a)) return -1;
        if (m == 0) {
          if (pass) P->written_pass += (uint64_t)(j - i);
          else P->written_fail += (uint64_t)(j - i);
        }
      }
      i = j - 1;
    }
    for (int c = 0; c < 2; ++c)
      if (S[c].f && S[c].n && spans_flush(&S[c])) return -1;
  }
  return 0;
}

static void *writer_main(void *arg) {
  pipe_t *P = arg;
  for (int64_t k = 0;; ++k) {
    slot_t *s = &P->slot[k % P->nslots];
    pthread_mutex_lock(&P->mu);
    while (!(s->state == 2 && s->chunk == k) && !P->error && !(P->reader_done && k >= P->chunks))
      pthread_cond_wait(&P->cv, &P->mu);
    const int stop = P->error || !(s->state == 2 && s->chunk == k);
    pthread_mutex_unlock(&P->mu);
    if (stop) break;
    const int rc = write_slot(P, s);
    pthread_mutex_lock(&P->mu);
    if (rc) P->error = -1;
    s->state = 0;
    pthread_cond_broadcast(&P->cv);
    pthread_mutex_unlock(&P->mu);
    if (rc) break;
  }
  return NULL;
}

/* ---- GPU worker (this thread) -------------------------------------------- */

/* edit: a chunk's trimmed records per output class, in input order (header
 * line, seq[ts, len - te), '+' line, qual[ts, len - te); each at most its input
 * record's bytes), built on the worker thread: with the writer formatting them
 * read by read through stdio (6 calls per read) `edit` ran at 6.8 Mreads/s end
 * to end against 135 for `stats` */
static int assemble_edit(pipe_t *P, slot_t *s) {
  const int filter_on = P->o->filter_on;
  for (int m = 0; m < P->nmates; ++m) {
    const mate_view_t v = mate_view(P, s, m);
    char **out = s->out + 2 * m;
    for (int c = 0; c < 2; ++c) {
      s->out_len[2 * m + c] = 0;
      s->out_n[2 * m + c] = 0;
      if (v.f[c] && s->out_cap[2 * m + c] < v.use + 64) {
        free(out[c]);
        s->out_cap[2 * m + c] = v.use + v.use / 8 + 64;
        out[c] = malloc(s->out_cap[2 * m + c]);
        if (!out[c]) {
          s->out_cap[2 * m + c] = 0;
          return HPGQ_E_NOMEM;
        }
      }
    }
    char *d[2] = {out[0], out[1]};
    for (int64_t i = 0; i < s->nreads; ++i) {
      const int c = s->mask[i] != 0 || !filter_on ? 0 : 1;
      if (!v.f[c]) continue;
      const int64_t r = v.first + i * v.stride;
      const uint32_t a = v.rs[r];
      const uint32_t ts = v.trim[i] & 0xFFFFu, te = v.trim[i] >> 16;
      const uint32_t len = (uint32_t)(v.idx[i + 1] - v.idx[i]);
      const uint32_t keep = len - ts - te;
      const uint32_t hl = v.ss[r] - a, pl = v.qs[r] - v.ps[r];
      char *o = d[c];
      memcpy(o, v.buf + a, hl);                               /* header line */
      o += hl;
      memcpy(o, v.buf + v.ss[r] + ts, keep);
      o += keep;
      *o++ = '\n';
      memcpy(o, v.buf + v.ps[r], pl);                         /* '+' line */
      o += pl;
      memcpy(o, v.buf + v.qs[r] + ts, keep);
      o += keep;
      *o++ = '\n';
      d[c] = o;
      s->out_n[2 * m + c]++;
    }
    for (int c = 0; c < 2; ++c) s->out_len[2 * m + c] = v.f[c] ? (size_t)(d[c] - out[c]) : 0;
  }
  return 0;
}

/* room for `need` bytes in output k of the slot */
static int out_room(slot_t *s, int k, size_t need) {
  if (s->out_cap[k] >= need) return 0;
  free(s->out[k]);
  s->out_cap[k] = need + need / 8;
  s->out[k] = malloc(s->out_cap[k]);
  if (!s->out[k]) {
    s->out_cap[k] = 0;
    return HPGQ_E_NOMEM;
  }
  return 0;
}

/* one output record: header line, keep bases, '+' line, keep qualities */
static inline char *put_record(char *o, const char *hdr, uint32_t hl, const char *seq, const char *plus, uint32_t pl,
                               const char *qual, uint32_t keep) {
  memcpy(o, hdr, hl);
  o += hl;
  memcpy(o, seq, keep);
  o += keep;
  *o++ = '\n';
  memcpy(o, plus, pl);
  o += pl;
  memcpy(o, qual, keep);
  o += keep;
  *o++ = '\n';
  return o;
}

/* edit --merge-overlap: assemble_edit over a unit whose pairs
 * split in two.  ins: the unit's F*.  Pair i with ins[i] <= 0 is the next
 * unmerged pair: its mates go to edit_1/2 or failed_1/2 from the paired ctx's
 * mask, trims and kept offsets at that rank (n_un of them).  A pair with
 * ins[i] > 0 is the next merged read: mate 1's header and '+' line as they
 * stand, between them the merged bases and qualities, rebuilt from the text by
 * the host rule (hpgq_ovl_merge), trimmed and classed by the merged ctx's
 * results at that rank.  (Its unmerged branch is assemble_edit's record path
 * once more, through out_room and put_record; assemble_edit itself is left as
 * it was and could use the two helpers as well.) */
static int assemble_merge(pipe_t *P, slot_t *s, const int32_t *ins, int64_t n_un, const uint8_t *mmask,
                          const uint32_t *mtrim, const int32_t *midx) {
  const int filter_on = P->o->filter_on;
  mate_view_t v[2] = {mate_view(P, s, 0), mate_view(P, s, 1)};
  for (int m = 0; m < 2; ++m) {   /* (the engine's results are n_un long, the record offsets the unit's) */
    v[m].trim = s->trim + (size_t)m * (size_t)n_un;
    v[m].idx = s->idx + (size_t)m * (size_t)(n_un + 1);
  }
  char *d[6] = {NULL, NULL, NULL, NULL, NULL, NULL};
  for (int k = 0; k < 6; ++k) {
    s->out_len[k] = 0;
    s->out_n[k] = 0;
    if (!P->out[k]) continue;
    const int rc = out_room(s, k, k < 4 ? v[k / 2].use + 64 : v[0].use + v[1].use + 64);
    if (rc) return rc;
    d[k] = s->out[k];
  }
  static __thread unsigned char mseq[2 * HPGQ_OVL_MAX_LEN], mqual[2 * HPGQ_OVL_MAX_LEN];
  int64_t u = 0, g = 0;
  for (int64_t i = 0; i < s->nreads; ++i) {
    const int64_t r0 = v[0].first + i * v[0].stride;
    if (ins[i] > 0) {
      const int c = mmask[g] != 0 || !filter_on ? 0 : 1;
      if (d[4 + c]) {
        const char *seq[2], *qual[2];
        size_t len[2];
        for (int m = 0; m < 2; ++m) {
          const int64_t r = v[m].first + i * v[m].stride;
          seq[m] = v[m].buf + v[m].ss[r];
          qual[m] = v[m].buf + v[m].qs[r];
          len[m] = v[m].ps[r] - v[m].ss[r] - 1;
          if (len[m] && seq[m][len[m] - 1] == '\r') --len[m];
        }
        const uint32_t F = (uint32_t)ins[i], ts = mtrim[g] & 0xFFFFu, te = mtrim[g] >> 16;
        if ((uint32_t)(midx[g + 1] - midx[g]) != F || ts + te > F ||
            hpgq_ovl_merge(seq[0], qual[0], len[0], seq[1], qual[1], len[1], ins[i], mseq, mqual, NULL) != ins[i])
          return HPGQ_E_INVALID;
        d[4 + c] = put_record(d[4 + c], v[0].buf + v[0].rs[r0], v[0].ss[r0] - v[0].rs[r0], (const char *)mseq + ts,
                              v[0].buf + v[0].ps[r0], v[0].qs[r0] - v[0].ps[r0], (const char *)mqual + ts, F - ts - te);
        s->out_n[4 + c]++;
      }
      ++g;
      continue;
    }
    const int c = s->mask[u] != 0 || !filter_on ? 0 : 1;
    for (int m = 0; m < 2; ++m) {
      if (!d[2 * m + c]) continue;
      const int64_t r = v[m].first + i * v[m].stride;
      const uint32_t ts = v[m].trim[u] & 0xFFFFu, te = v[m].trim[u] >> 16;
      const uint32_t keep = (uint32_t)(v[m].idx[u + 1] - v[m].idx[u]) - ts - te;
      d[2 * m + c] = put_record(d[2 * m + c], v[m].buf + v[m].rs[r], v[m].ss[r] - v[m].rs[r], v[m].buf + v[m].ss[r] + ts,
                                v[m].buf + v[m].ps[r], v[m].qs[r] - v[m].ps[r], v[m].buf + v[m].qs[r] + ts, keep);
      s->out_n[2 * m + c]++;
    }
    ++u;
  }
  for (int k = 0; k < 6; ++k) s->out_len[k] = d[k] ? (size_t)(d[k] - s->out[k]) : 0;
  return 0;
}

/* the per-chunk results come back by DMA: page-locked buffers (pageable
 * destinations are staged through the runtime's bounce buffer, synchronously) */
static void free_results(slot_t *s) {
  void **b[7] = {(void **)&s->mask, (void **)&s->trim, (void **)&s->rec_start, (void **)&s->seq_start,
                 (void **)&s->plus_start, (void **)&s->qual_start, (void **)&s->idx};
  for (int i = 0; i < 7; ++i) {
    hpgq_host_free(*b[i]);
    *b[i] = NULL;
  }
  s->res_cap = 0;
}

/* n reads (pairs), nm mates: the mask per read, everything else per mate */
static int ensure_results(slot_t *s, int64_t n, int nm) {
  if ((size_t)n <= s->res_cap) return 0;
  free_results(s);
  const size_t c = (size_t)n + (size_t)n / 4 + 1024, cm = c * (size_t)nm;
  void **b[7] = {(void **)&s->mask, (void **)&s->trim, (void **)&s->rec_start, (void **)&s->seq_start,
                 (void **)&s->plus_start, (void **)&s->qual_start, (void **)&s->idx};
  const size_t sz[7] = {c, cm * 4, cm * 4, cm * 4, cm * 4, cm * 4, (cm + 2) * 4};
  for (int i = 0; i < 7; ++i)
    if (hpgq_host_alloc(b[i], sz[i])) {
      free_results(s);
      return -1;
    }
  s->res_cap = c;
  return 0;
}

/* ---- mapped outputs: placement in input order, parallel copy -------------- */

/* output class of record i (0: passed / edit.fq, 1: failed.fq) and its output
 * bytes: the whole input record (filter) or the trimmed one (edit) */
static inline int rec_class(const pipe_t *P, const slot_t *s, int64_t i) {
  return s->mask[i] != 0 || !P->o->filter_on ? 0 : 1;
}

static inline uint64_t rec_out_bytes(const pipe_t *P, const slot_t *s, int64_t i) {
  if (P->o->command != CMD_EDIT) {
    const uint32_t ee = i + 1 < s->nreads ? s->rec_start[i + 1] : (uint32_t)s->use;
    return ee - s->rec_start[i];
  }
  const uint32_t ts = s->trim[i] & 0xFFFFu, te = s->trim[i] >> 16;
  const uint32_t keep = (uint32_t)(s->idx[i + 1] - s->idx[i]) - ts - te;
  return (uint64_t)(s->seq_start[i] - s->rec_start[i]) + (s->qual_start[i] - s->plus_start[i]) + 2u * keep + 2u;
}

#define MAX_COPIERS 64
typedef struct {
  pipe_t *P;
  slot_t *s;
  int64_t i0, i1;      /* records of this part */
  uint64_t bytes[2];   /* its output bytes per class */
  char *dst[2];        /* where its records go */
  pthread_t th;
  int started;
} copy_part_t;

/* records [i0, i1) into the maps at dst[class] */
static void copy_records(pipe_t *P, slot_t *s, int64_t i0, int64_t i1, char *dst[2]) {
  const int edit = P->o->command == CMD_EDIT;
  for (int64_t i = i0; i < i1; ++i) {
    const int c = rec_class(P, s, i);
    if (!P->map[c]) continue;
    if (!edit) {   /* a run of same-class records is one contiguous span */
      int64_t j = i + 1;
      while (j < i1 && rec_class(P, s, j) == c) ++j;
      const uint32_t a = s->rec_start[i];
      const uint32_t ee = j < s->nreads ? s->rec_start[j] : (uint32_t)s->use;
      memcpy(dst[c], s->buf + a, ee - a);
      dst[c] += ee - a;
      i = j - 1;
      continue;
    }
    const uint32_t a = s->rec_start[i];
    const uint32_t ts = s->trim[i] & 0xFFFFu, te = s->trim[i] >> 16;
    const uint32_t keep = (uint32_t)(s->idx[i + 1] - s->idx[i]) - ts - te;
    const uint32_t hl = s->seq_start[i] - a, pl = s->qual_start[i] - s->plus_start[i];
    char *o = dst[c];
    memcpy(o, s->buf + a, hl);                              /* header line */
    o += hl;
    memcpy(o, s->buf + s->seq_start[i] + ts, keep);
    o += keep;
    *o++ = '\n';
    memcpy(o, s->buf + s->plus_start[i], pl);                /* '+' line */
    o += pl;
    memcpy(o, s->buf + s->qual_start[i] + ts, keep);
    o += keep;
    *o++ = '\n';
    dst[c] = o;
  }
}

static void *size_part(void *arg) {
  copy_part_t *cp = arg;
  cp->bytes[0] = cp->bytes[1] = 0;
  for (int64_t i = cp->i0; i < cp->i1; ++i) cp->bytes[rec_class(cp->P, cp->s, i)] += rec_out_bytes(cp->P, cp->s, i);
  return NULL;
}

/* fn over the parts: part 0 on this thread, the others on threads of their own
 * (a part whose thread cannot start runs here too) */
static void run_parts(void *(*fn)(void *), copy_part_t *part, int n) {
  for (int t = 1; t < n; ++t) part[t].started = pthread_create(&part[t].th, NULL, fn, &part[t]) == 0;
  fn(&part[0]);
  for (int t = 1; t < n; ++t) {
    if (part[t].started) pthread_join(part[t].th, NULL);
    else fn(&part[t]);
  }
}

static void copy_part_run(void *arg) {
  copy_part_t *cp = arg;
  copy_records(cp->P, cp->s, cp->i0, cp->i1, cp->dst);
}

/* copier thread: takes parts off the queue; the last part of a chunk frees its
 * slot for the reader */
static void *copier_main(void *arg) {
  pipe_t *P = arg;
  for (;;) {
    pthread_mutex_lock(&P->cq_mu);
    while (P->cq_head == P->cq_tail && !P->cq_exit) pthread_cond_wait(&P->cq_cv, &P->cq_mu);
    if (P->cq_head == P->cq_tail) {
      pthread_mutex_unlock(&P->cq_mu);
      break;
    }
    copy_part_t *cp = P->cq[P->cq_head % P->cq_cap];
    P->cq_head++;
    pthread_mutex_unlock(&P->cq_mu);
    /* a store the file system cannot back ends the copy with HPGQ_E_IO, not SIGBUS */
    const int e = mapout_guard(copy_part_run, cp);
    pthread_mutex_lock(&P->mu);
    if (e && !P->error) P->error = e;
    if (--cp->s->parts_left == 0) {
      cp->s->state = 0;
      P->copies_pending--;
      pthread_cond_broadcast(&P->cv);
    }
    pthread_mutex_unlock(&P->mu);
  }
  return NULL;
}

static int start_copiers(pipe_t *P) {
  int n = P->o->copy_threads > 0 ? P->o->copy_threads : P->o->num_threads;
  if (n > 64) n = 64;
  if (n < 1) n = 1;
  P->cq_cap = P->nslots * MAX_COPIERS;
  P->cq = calloc((size_t)P->cq_cap, sizeof(void *));
  if (!P->cq) return HPGQ_E_NOMEM;
  for (int i = 0; i < P->nslots; ++i) {
    P->slot[i].parts = calloc(MAX_COPIERS, sizeof(copy_part_t));
    if (!P->slot[i].parts) return HPGQ_E_NOMEM;
  }
  for (int t = 0; t < n; ++t) {
    if (pthread_create(&P->copier[t], NULL, copier_main, P)) break;
    P->ncopiers++;
  }
  return P->ncopiers ? 0 : HPGQ_E_NOMEM;
}

/* every placed chunk copied, then the copiers end */
static void stop_copiers(pipe_t *P) {
  pthread_mutex_lock(&P->mu);
  while (P->copies_pending > 0) pthread_cond_wait(&P->cv, &P->mu);
  pthread_mutex_unlock(&P->mu);
  pthread_mutex_lock(&P->cq_mu);
  P->cq_exit = 1;
  pthread_cond_broadcast(&P->cq_cv);
  pthread_mutex_unlock(&P->cq_mu);
  for (int t = 0; t < P->ncopiers; ++t) pthread_join(P->copier[t], NULL);
  P->ncopiers = 0;
}

/* a processed chunk into the mapped outputs: size its records per class (in
 * parallel), place it after chunk k-1 (which only needs k-1's sizes, not its
 * copies), queue its parts for the copier threads (the slot stays busy, state
 * 3, until they are copied) */
static int place_and_copy(pipe_t *P, slot_t *s, int *handed) {
  copy_part_t *part = s->parts;
  int n = P->ncopiers;   /* one part per copier thread (--copy-threads, default --num-threads) */
  const int64_t per_min = 16384;   /* records per copier at least */
  if (n > MAX_COPIERS) n = MAX_COPIERS;
  if ((int64_t)n > s->nreads / per_min + 1) n = (int)(s->nreads / per_min + 1);
  if (n < 1) n = 1;
  const int64_t per = (s->nreads + n - 1) / n;
  for (int t = 0; t < n; ++t) {
    copy_part_t *cp = &part[t];
    cp->P = P;
    cp->s = s;
    cp->i0 = (int64_t)t * per < s->nreads ? (int64_t)t * per : s->nreads;
    cp->i1 = cp->i0 + per < s->nreads ? cp->i0 + per : s->nreads;
  }
  run_parts(size_part, part, n);
  uint64_t sz[2] = {0, 0}, base[2] = {0, 0}, npass = 0, nfail = 0;
  for (int t = 0; t < n; ++t) {
    sz[0] += part[t].bytes[0];
    sz[1] += part[t].bytes[1];
  }
  int rc = 0;
  pthread_mutex_lock(&P->mu);
  while (P->placed != s->chunk && !P->error) pthread_cond_wait(&P->cv, &P->mu);
  if (P->error) {
    rc = P->error;   /* (stop; a copier's HPGQ_E_IO reaches the caller as is) */
  } else if (P->out_off[0] + sz[0] > P->map_cap || P->out_off[1] + sz[1] > P->map_cap) {
    rc = HPGQ_E_IO;   /* (cannot happen: each output is at most the input) */
  } else if ((rc = mapout_error(&P->mo)) == 0) {   /* (a window the prefault threads could not back) */
    for (int c = 0; c < 2; ++c) {
      base[c] = P->out_off[c];
      P->out_off[c] += sz[c];
      mapout_advance(&P->mo, c, P->out_off[c]);
    }
    P->placed++;
  }
  pthread_cond_broadcast(&P->cv);
  pthread_mutex_unlock(&P->mu);
  if (rc) return rc;
  trace_at(P, s->chunk, 7, -1);
  for (int t = 0; t < n; ++t) {
    for (int c = 0; c < 2; ++c) {
      part[t].dst[c] = P->map[c] ? P->map[c] + base[c] : NULL;
      base[c] += part[t].bytes[c];
    }
  }
  for (int64_t i = 0; i < s->nreads; ++i) {
    if (rec_class(P, s, i)) ++nfail;
    else ++npass;
  }
  const int queue = s->nreads > 0;
  pthread_mutex_lock(&P->mu);
  P->written_pass += npass;
  P->written_fail += nfail;
  if (queue) {   /* busy until copied (set before the parts can finish) */
    s->state = 3;
    s->parts_left = n;
    P->copies_pending++;
  }
  pthread_mutex_unlock(&P->mu);
  /* from here the copiers own the slot: the last part frees it and the reader
   * may refill it at once, so neither this function nor the worker touches s */
  *handed = queue;
  if (queue) {
    pthread_mutex_lock(&P->cq_mu);
    for (int t = 0; t < n; ++t) P->cq[P->cq_tail++ % P->cq_cap] = &part[t];
    pthread_cond_broadcast(&P->cq_cv);
    pthread_mutex_unlock(&P->cq_mu);
  }
  return 0;
}

/* map the outputs for the parallel writer (hpgq_mapout.h): each is at most
 * the input (+ the final newline the reader may add); 0 when mapped, 1: the
 * stream writer runs (files left empty), < 0 an error */
static int map_outputs(pipe_t *P, off_t input_size) {
  const int fd[2] = {P->out[0] ? fileno(P->out[0]) : -1, P->out[1] ? fileno(P->out[1]) : -1};
  P->map_cap = (size_t)input_size + 4096;
  /* --prefault-threads N: populate two chunks ahead of the placed records on
   * N threads.  Default none past the reserved first window: on MI355X boxes
   * the prefault threads made stored `filter` slower (same box, alternating:
   * median 16 vs 24-26 Mreads/s with 2 threads vs none, profiles/
   * r05_writer_ab.json) -- they contend with the copiers for the one file's
   * page allocation; the SIGBUS guard covers what is not reserved */
  const size_t ahead = (size_t)2 * ((size_t)P->o->chunk_mb << 20);
  const int pft = P->o->prefault_threads < 0 ? 0 : P->o->prefault_threads;
  const int rc = mapout_open(&P->mo, fd, P->map_cap, ahead, pft, P->o->writer_hook);
  if (rc) return rc;
  P->map[0] = P->mo.map[0];
  P->map[1] = P->mo.map[1];
  P->mmap_out = 1;
  return 0;
}

static void unmap_outputs(pipe_t *P, int *rc) {
  const uint64_t size[2] = {P->out_off[0], P->out_off[1]};
  const int e = mapout_close(&P->mo, size);
  if (e && *rc == 0) *rc = e;
  P->map[0] = P->map[1] = NULL;
}

/* --duplication: a worker's table starts at 16 MB and doubles as the input
 * needs, up to 64 GB (hpgq_dup_open) */
#define DUP_LOG2_SLOTS 20
#define DUP_LOG2_MAX_SLOTS 32

/* all of src's pairs on the host (malloc'd; *n == 0: both NULL) */
static int dup_pairs(hpgq_dup_t *src, uint64_t **keys, uint64_t **counts, size_t *n) {
  *keys = *counts = NULL;
  int rc = hpgq_dup_export(src, NULL, NULL, 0, n);
  if (rc || *n == 0) return rc;
  *keys = malloc(*n * sizeof(uint64_t));
  *counts = malloc(*n * sizeof(uint64_t));
  if (!*keys || !*counts) rc = HPGQ_E_NOMEM;
  if (rc == 0) rc = hpgq_dup_export(src, *keys, *counts, *n, n);
  if (rc) {
    free(*keys);
    free(*counts);
    *keys = *counts = NULL;
  }
  return rc;
}

/* dst += src through the host: works between GPUs too */
static int dup_move(hpgq_dup_t *dst, hpgq_dup_t *src) {
  uint64_t *keys, *counts;
  size_t n = 0;
  int rc = dup_pairs(src, &keys, &counts, &n);
  if (rc == 0 && n) rc = hpgq_dup_import(dst, keys, counts, n);
  free(keys);
  free(counts);
  return rc;
}

typedef struct { uint64_t key, count; } dup_pair_t;
static int dup_pair_cmp(const void *a, const void *b) {
  const uint64_t x = ((const dup_pair_t *)a)->key, y = ((const dup_pair_t *)b)->key;
  return x < y ? -1 : x > y;
}

/* the table with its keys ascending */
static int dup_sorted(hpgq_dup_t *src, uint64_t **keys, uint64_t **counts, size_t *n) {
  int rc = dup_pairs(src, keys, counts, n);
  if (rc || *n == 0) return rc;
  dup_pair_t *pr = malloc(*n * sizeof(*pr));
  if (!pr) return HPGQ_E_NOMEM;   /* (the caller frees the arrays with its result) */
  for (size_t i = 0; i < *n; ++i) pr[i] = (dup_pair_t){(*keys)[i], (*counts)[i]};
  qsort(pr, *n, sizeof(*pr), dup_pair_cmp);
  for (size_t i = 0; i < *n; ++i) {
    (*keys)[i] = pr[i].key;
    (*counts)[i] = pr[i].count;
  }
  free(pr);
  return 0;
}

/* one GPU worker: its own ctx, parser, k-mer and CGR accumulators on one device */
typedef struct {
  pipe_t *P;
  const hpgq_params_t *p;
  int w, device;
  hpgq_ctx_t *ctx;
  hpgq_parser_t *ps[2];   /* one per side ([1]: --fq2), both on the ctx stream */
  hpgq_kmers_t *km;
  hpgq_qdist_t *qd[2];    /* --quality-dist: one table per mate, on the ctx stream */
  hpgq_dup_t *dp[2];      /* --duplication: one hash table per mate, on the ctx stream */
  hpgq_adapt_t *ad[2];    /* --adapters: one table per mate, on the ctx stream */
  hpgq_clip_t *cl[2];     /* --clip-adapters: one handle per mate, on the ctx stream */
  hpgq_ovl_t *ov;         /* --clip-overlap: one handle for the pair, on the ctx stream */
  int32_t *h_ins;         /* --correct-overlap, --merge-overlap: the unit's F* on the host ([ins_cap]) */
  size_t ins_cap;
  /* --merge-overlap (§2.15): a single-end ctx for the merged reads on the paired ctx's stream (the run's
   * parameters with paired = 0; it runs behind the merge and the paired ctx), its mask and trims on the device
   * and, page-locked on the host, with the merged reads' kept offsets ([mcap], [mcap], [mcap + 1]) */
  hpgq_params_t p2;
  hpgq_ctx_t *ctx2;
  uint8_t *d_mask2, *h_mmask;
  uint32_t *d_trim2, *h_mtrim;
  int32_t *h_midx;
  size_t mcap;
  hpgq_cgr_t *cg;
  uint8_t *d_mask;
  uint32_t *d_trim;
  size_t dcap;
  int rc;
  pthread_t th;
  uint64_t num_reads;
  int cg_exact_calls;
  double fastq_bytes;
} worker_t;

static int worker_open(worker_t *W) {
  const cli_options_t *o = W->P->o;
  int rc = hpgq_open(&W->ctx, W->device, W->p);
  for (int m = 0; m < W->P->nsides && rc == 0; ++m) rc = hpgq_parser_open(&W->ps[m], W->device, hpgq_stream(W->ctx));
  /* --kmers counts the reads the stats merge (passed ones when filtering,
   * src/stats_fastq.c:268-272,384-410) on the engine's stream, after it */
  if (rc == 0 && o->kmers_on) rc = hpgq_kmers_open(&W->km, W->device, W->p->lmax, hpgq_stream(W->ctx));
  /* --quality-dist counts the same reads, per mate (passed pairs for paired
   * input): lmax rows to start with, the window of on-chip values from phred */
  for (int m = 0; m < W->P->nmates && rc == 0 && o->quality_dist_on; ++m)
    rc = hpgq_qdist_open(&W->qd[m], W->device, W->p->lmax, W->p->phred, hpgq_stream(W->ctx));
  /* --adapters counts the same reads, per mate: lmax rows to start with */
  for (int m = 0; m < W->P->nmates && rc == 0 && o->adapters_on; ++m) {
    const char *probes[HPGQ_ADAPT_MAX_PROBES];
    for (int a = 0; a < o->adapter_n; ++a) probes[a] = o->adapter_probes[a];
    rc = hpgq_adapt_open(&W->ad[m], W->device, probes, o->adapter_n, W->p->lmax, hpgq_stream(W->ctx));
  }
  /* --clip-overlap cuts both mates of a pair before anything else sees them */
  if (rc == 0 && o->ovl_on)
    rc = hpgq_ovl_open(&W->ov, W->device, o->ovl_min_overlap, o->ovl_max_mismatches, hpgq_stream(W->ctx));
  /* --correct-overlap and --insert-size are switches of that handle (§2.14) */
  if (rc == 0 && o->ovl_fix_on)
    rc = hpgq_ovl_set_correct(W->ov, 1, o->quality_encoding_value, o->ovl_fix_high, o->ovl_fix_low);
  if (rc == 0 && o->ovl_insert_on) rc = hpgq_ovl_count_inserts(W->ov, 1);
  if (rc == 0 && o->ovl_merge_on) {
    W->p2 = *W->p;
    W->p2.paired = 0;
    rc = hpgq_open_on_stream(&W->ctx2, W->device, &W->p2, hpgq_stream(W->ctx));
  }
  /* --clip-adapters cuts each mate on its own before the engine sees it */
  for (int m = 0; m < W->P->nmates && rc == 0 && o->clip_on; ++m) {
    const char *probes[HPGQ_ADAPT_MAX_PROBES];
    for (int a = 0; a < o->adapter_n; ++a) probes[a] = o->adapter_probes[a];
    rc = hpgq_clip_open(&W->cl[m], W->device, probes, o->adapter_n, o->clip_min_overlap, hpgq_stream(W->ctx));
  }
  /* --duplication counts the same reads again, per mate, by their sequence;
   * --overrepresented needs the same tables, keeping the bytes of the sequences
   * that reach ceil(K / workers) in one of them: a sequence with K or more in
   * all has that many in at least one */
  for (int m = 0; m < W->P->nmates && rc == 0 && (o->duplication_on || o->overrep_on); ++m) {
    rc = hpgq_dup_open(&W->dp[m], W->device, DUP_LOG2_SLOTS, DUP_LOG2_MAX_SLOTS, hpgq_stream(W->ctx));
    const uint64_t nw = (uint64_t)W->P->nworkers;
    if (rc == 0 && o->overrep_on)
      rc = hpgq_dup_keep_sequences(W->dp[m], o->overrep_min_count / nw + (o->overrep_min_count % nw != 0), o->overrep_bytes);
  }
  /* --cg: chaos_game_fill_tables per batch (= chunk), the base quality from
   * --quality-encoding; with a filter only the passed reads (ONLY_VALID_READS
   * with the mask as read_status, old/chaos_game.c:188) */
  if (rc == 0 && o->cg_on) rc = hpgq_cgr_open(&W->cg, W->device, o->k_cg, W->p->phred);
  return rc;
}

static void worker_close(worker_t *W) {
  hpgq_device_free(W->d_mask);
  hpgq_device_free(W->d_trim);
  hpgq_parser_close(W->ps[0]);
  hpgq_parser_close(W->ps[1]);
  hpgq_kmers_close(W->km);
  hpgq_qdist_close(W->qd[0]);
  hpgq_qdist_close(W->qd[1]);
  hpgq_adapt_close(W->ad[0]);
  hpgq_adapt_close(W->ad[1]);
  hpgq_clip_close(W->cl[0]);
  hpgq_clip_close(W->cl[1]);
  hpgq_ovl_close(W->ov);
  free(W->h_ins);
  hpgq_device_free(W->d_mask2);
  hpgq_device_free(W->d_trim2);
  hpgq_host_free(W->h_mmask);
  hpgq_host_free(W->h_mtrim);
  hpgq_host_free(W->h_midx);
  hpgq_close(W->ctx2);
  hpgq_dup_close(W->dp[0]);
  hpgq_dup_close(W->dp[1]);
  hpgq_cgr_close(W->cg);
  hpgq_close(W->ctx);
}

/* --overrepresented, mate m, after the merge into worker 0's table: the top N
 * of the merged counts, and each one's bytes from the first worker's table
 * that kept them (the merge moves counts, never bytes; every arena was found
 * large enough before the merge, and an import keeps nothing) */
static int overrep_list(const cli_options_t *o, worker_t *W, int G, int m, cli_result_t *res) {
  size_t total = 0;
  const size_t cap = (size_t)o->overrep_top;
  uint64_t *keys = malloc(cap * sizeof(uint64_t));
  res->overrep_counts[m] = malloc(cap * sizeof(uint64_t));
  res->overrep_lens[m] = calloc(cap, sizeof(uint64_t));
  res->overrep_seqs[m] = calloc(cap, sizeof(unsigned char *));
  res->overrep_reads[m] = res->dup_levels[m].reads;
  int rc = keys && res->overrep_counts[m] && res->overrep_lens[m] && res->overrep_seqs[m] ? 0 : HPGQ_E_NOMEM;
  if (rc == 0) rc = hpgq_dup_top(W[0].dp[m], o->overrep_min_count, keys, res->overrep_counts[m], cap, &total);
  const size_t n = total < cap ? total : cap;
  for (size_t i = 0; i < n && rc == 0; ++i) {
    int64_t len = -1;
    for (int w = 0; w < G && rc == 0 && len < 0; ++w) {
      rc = hpgq_dup_sequence(W[w].dp[m], keys[i], NULL, 0, &len);
      if (rc || len < 0) continue;
      res->overrep_seqs[m][i] = malloc(len ? (size_t)len : 1);
      if (!res->overrep_seqs[m][i]) rc = HPGQ_E_NOMEM;
      else rc = hpgq_dup_sequence(W[w].dp[m], keys[i], res->overrep_seqs[m][i], (size_t)len, &len);
      res->overrep_lens[m][i] = (uint64_t)len;
    }
    if (rc == 0 && len < 0) {   /* no table kept a listed sequence: the shard rule is broken */
      res->overrep_error = 2;
      rc = HPGQ_E_STATE;
    }
  }
  if (rc == 0) res->overrep_n[m] = n;
  free(keys);
  return rc;
}

/* the mate name of record r of a text, for the error line */
static void record_name(const char *buf, size_t use, int64_t r, char *out, size_t cap) {
  size_t a = (size_t)hpgq_fastq_record_prefix(buf, (int64_t)use, r, NULL) + 1, k = 0;   /* after '@' */
  for (; a < use && k + 1 < cap; ++a) {
    const char c = buf[a];
    if (c == ' ' || c == '\t' || c == '\r' || c == '\n') break;
    out[k++] = c;
  }
  out[k] = 0;
}

/* --correct-overlap: the writers assemble the outputs from
 * the unit's text, not from the device's kept reads, so the correction the
 * device made for the stages behind it is made here once more, by the same
 * rule on the host (hpgq_ovl_correct), in place in the text: pair i with
 * ins[i] = F* > 0, each mate's sequence and quality line.  The lengths are the
 * records' own (a "\r\n" line end is not part of them). */
static int correct_text(const pipe_t *P, slot_t *s, const int32_t *ins) {
  const cli_options_t *o = P->o;
  const mate_view_t v[2] = {mate_view(P, s, 0), mate_view(P, s, 1)};
  for (int64_t i = 0; i < s->nreads; ++i) {
    if (ins[i] <= 0) continue;
    char *seq[2], *qual[2];
    size_t len[2];
    for (int m = 0; m < 2; ++m) {
      const int64_t r = v[m].first + i * v[m].stride;
      char *buf = (char *)v[m].buf;   /* (the slot's own, writable text) */
      seq[m] = buf + v[m].ss[r];
      qual[m] = buf + v[m].qs[r];
      len[m] = v[m].ps[r] - v[m].ss[r] - 1;
      if (len[m] && seq[m][len[m] - 1] == '\r') --len[m];
    }
    if (hpgq_ovl_correct(seq[0], qual[0], len[0], seq[1], qual[1], len[1], ins[i], o->quality_encoding_value,
                         o->ovl_fix_high, o->ovl_fix_low, NULL) < 0)
      return HPGQ_E_INVALID;
  }
  return HPGQ_OK;
}

/* One chunk on the worker's GPU: its nm mates parsed (one text, two texts, or
 * one interleaved text split on the device), for pairs the mate names checked,
 * one engine call, k-mers and CGR (single-end only: validation); for filter /
 * edit the mask per read and every mate's trims and data_indices come back,
 * and every side's record offsets. */
static int worker_chunk(worker_t *W, slot_t *s) {
  pipe_t *P = W->P;
  const cli_options_t *o = P->o;
  const int nm = P->nmates, ns = P->nsides;
  const int writes = o->command != CMD_STATS;
  const int edit = o->command == CMD_EDIT;
  const int need_mask = writes || ((W->km || W->cg || W->qd[0] || W->dp[0] || W->ad[0]) && o->filter_on);
  const char *const text[2] = {s->buf, s->buf2};
  const size_t use[2] = {s->use, s->use2};
  hpgq_batch_t b[2];
  s->nreads = 0;
  int rc = 0;
  if (nm > ns) rc = hpgq_parse_host_interleaved(W->ps[0], text[0], (int64_t)use[0], &b[0], &b[1]);
  else
    for (int m = 0; m < ns && rc == 0; ++m) rc = hpgq_parse_host(W->ps[m], text[m], (int64_t)use[m], &b[m]);
  trace_at(P, s->chunk, 5, -1);
  if (nm == 2) {
    const int two = ns == 2;
    int64_t bad = -1;
    if (rc == 0) rc = hpgq_parse_pair_check(W->ps[0], W->ps[1], &bad);
    if (rc == HPGQ_E_PAIRING) {
      char msg[512], n1[160] = "", n2[160] = "";
      if (bad >= 0 && bad < b[0].num_reads && bad < b[1].num_reads) {
        record_name(s->buf, s->use, two ? bad : 2 * bad, n1, sizeof(n1));
        record_name(two ? s->buf2 : s->buf, two ? s->use2 : s->use, two ? bad : 2 * bad + 1, n2, sizeof(n2));
        snprintf(msg, sizeof(msg), "pair %lld: mate names differ: '%s' and '%s'", (long long)(s->pair0 + bad), n1, n2);
      } else {
        snprintf(msg, sizeof(msg), "pair %lld: the mates' record counts differ", (long long)(s->pair0 + (bad > 0 ? bad : 0)));
      }
      pairing_fail(P, s->chunk, s->pair0 + (bad > 0 ? bad : 0), msg);
      return rc;
    }
  }
  if (rc || b[0].num_reads == 0) return rc;
  /* --clip-overlap: from here on the pair is the kept reads, in buffers the
   * handle owns until its next chunk; the probes below see what it kept */
  const size_t na = (size_t)b[0].num_reads;   /* the unit's reads (pairs): what the texts hold */
  const int merging = W->ov && o->ovl_merge_on;
  hpgq_batch_t bm = {0, NULL, NULL, NULL};
  /* --merge-overlap (§2.15): the pairs without an overlap go on as pairs, uncut; the others as one read each */
  if (merging) {
    if ((rc = hpgq_ovl_merge_device(W->ov, &b[0], &b[1], &b[0], &b[1], &bm)) != 0) return rc;
  } else if (W->ov && (rc = hpgq_ovl_batch_device(W->ov, &b[0], &b[1], &b[0], &b[1])) != 0) return rc;
  /* --clip-adapters: from here on the batch is the kept reads, in buffers the
   * handle owns until its next chunk (this chunk's hpgq_sync comes before that) */
  for (int m = 0; m < nm && W->cl[m]; ++m)
    if (b[m].num_reads && (rc = hpgq_clip_batch_device(W->cl[m], &b[m], &b[m])) != 0) return rc;
  const size_t n = (size_t)b[0].num_reads;
  if (need_mask && n > W->dcap) {
    hpgq_device_free(W->d_mask);
    hpgq_device_free(W->d_trim);
    W->d_mask = NULL;
    W->d_trim = NULL;
    W->dcap = n + n / 4 + 1024;
    rc = hpgq_device_alloc(W->device, (void **)&W->d_mask, W->dcap);
    if (rc == 0) rc = hpgq_device_alloc(W->device, (void **)&W->d_trim, W->dcap * 4 * (size_t)nm);
  }
  if (rc == 0) {   /* the long-read tails for the unit's longest record: no second pass */
    int64_t ml = hpgq_parser_max_length(W->ps[0]);
    if (ns == 2 && hpgq_parser_max_length(W->ps[1]) > ml) ml = hpgq_parser_max_length(W->ps[1]);
    rc = hpgq_reserve_length(W->ctx, ml);
    if (rc == 0 && W->km) rc = hpgq_kmers_reserve_length(W->km, ml);
    for (int m = 0; m < nm && rc == 0 && W->qd[m]; ++m) rc = hpgq_qdist_reserve_length(W->qd[m], ml);
    for (int m = 0; m < nm && rc == 0 && W->ad[m]; ++m) rc = hpgq_adapt_reserve_length(W->ad[m], ml);
  }
  if (rc == 0 && (n || !merging))   /* (--merge-overlap: every pair of the unit may have merged) */
    rc = hpgq_run_device(W->ctx, &b[0], nm == 2 ? &b[1] : NULL, need_mask ? W->d_mask : NULL, edit ? W->d_trim : NULL);
  /* the merged reads through the single-end ctx: no adapter clip, everything behind base F* is gone */
  const size_t M = (size_t)bm.num_reads;
  if (rc == 0 && M) {
    if (M > W->mcap) {
      hpgq_device_free(W->d_mask2);
      hpgq_device_free(W->d_trim2);
      hpgq_host_free(W->h_mmask);
      hpgq_host_free(W->h_mtrim);
      hpgq_host_free(W->h_midx);
      W->d_mask2 = W->h_mmask = NULL;
      W->d_trim2 = W->h_mtrim = NULL;
      W->h_midx = NULL;
      W->mcap = M + M / 4 + 1024;
      rc = hpgq_device_alloc(W->device, (void **)&W->d_mask2, W->mcap);
      if (rc == 0) rc = hpgq_device_alloc(W->device, (void **)&W->d_trim2, W->mcap * 4);
      if (rc == 0) rc = hpgq_host_alloc((void **)&W->h_mmask, W->mcap);
      if (rc == 0) rc = hpgq_host_alloc((void **)&W->h_mtrim, W->mcap * 4);
      if (rc == 0) rc = hpgq_host_alloc((void **)&W->h_midx, (W->mcap + 1) * 4);
      if (rc) W->mcap = 0;
    }
    if (rc == 0) rc = hpgq_reserve_length(W->ctx2, 2 * HPGQ_OVL_MAX_LEN - 8);
    if (rc == 0) rc = hpgq_run_device(W->ctx2, &bm, NULL, W->d_mask2, W->d_trim2);
    if (rc == 0) rc = hpgq_copy_to_host(W->ctx2, W->h_mmask, W->d_mask2, M);
    if (rc == 0) rc = hpgq_copy_to_host(W->ctx2, W->h_mtrim, W->d_trim2, M * 4);
    if (rc == 0) rc = hpgq_copy_to_host(W->ctx2, W->h_midx, bm.data_indices, (M + 1) * 4);
  }
  if (rc == 0 && W->km) rc = hpgq_kmers_count_device(W->km, &b[0], o->filter_on ? W->d_mask : NULL);
  for (int m = 0; m < nm && rc == 0 && W->qd[m]; ++m)   /* (paired: the pair mask for both mates) */
    rc = hpgq_qdist_count_device(W->qd[m], &b[m], o->filter_on ? W->d_mask : NULL);
  for (int m = 0; m < nm && rc == 0 && W->ad[m]; ++m)   /* (the same reads, the same mask) */
    rc = hpgq_adapt_count_device(W->ad[m], &b[m], o->filter_on ? W->d_mask : NULL);
  for (int m = 0; m < nm && rc == 0 && W->dp[m]; ++m)   /* (the same reads, the same mask) */
    rc = hpgq_dup_count_device(W->dp[m], &b[m], o->filter_on ? W->d_mask : NULL);
  if (rc == 0 && writes) {
    s->nreads = (int64_t)na;
    if (ensure_results(s, (int64_t)na, nm)) rc = HPGQ_E_NOMEM;
    if (rc == 0 && n) rc = hpgq_copy_to_host(W->ctx, s->mask, W->d_mask, n);
    if (rc == 0 && edit) {   /* (trim_out: mate m of read i at [m n + i]) */
      rc = hpgq_copy_to_host(W->ctx, s->trim, W->d_trim, n * 4 * (size_t)nm);
      for (int m = 0; m < nm && rc == 0; ++m)
        rc = hpgq_copy_to_host(W->ctx, s->idx + (size_t)m * (n + 1), b[m].data_indices, (n + 1) * 4);
    }
    /* the record offsets: an interleaved text's 2 n in text order, else mate 2's after mate 1's */
    for (int m = 0; m < ns && rc == 0; ++m)
      rc = hpgq_parse_records(W->ps[m], s->rec_start + m * na, s->seq_start + m * na, s->plus_start + m * na,
                              s->qual_start + m * na);
    /* --correct-overlap: the unit's F* for correct_text */
    if (rc == 0 && W->ov && (o->ovl_fix_on || merging)) {
      const int32_t *d_ins = NULL;
      rc = hpgq_ovl_last_inserts(W->ov, &d_ins);
      if (rc == 0 && na > W->ins_cap) {
        free(W->h_ins);
        W->ins_cap = na + na / 4 + 1024;
        W->h_ins = malloc(W->ins_cap * sizeof(int32_t));
        if (!W->h_ins) W->ins_cap = 0, rc = HPGQ_E_NOMEM;
      }
      if (rc == 0) rc = hpgq_copy_to_host(W->ctx, W->h_ins, d_ins, na * sizeof(int32_t));
    }
  }
  trace_at(P, s->chunk, 3, -1);
  if (rc == 0) rc = hpgq_sync(W->ctx);
  if (rc == 0 && M) rc = hpgq_sync(W->ctx2);
  trace_at(P, s->chunk, 6, -1);
  if (rc == 0 && writes && W->ov && o->ovl_fix_on) rc = correct_text(P, s, W->h_ins);
  if (rc == 0 && edit && !P->mmap_out)
    rc = merging ? assemble_merge(P, s, W->h_ins, (int64_t)n, W->h_mmask, W->h_mtrim, W->h_midx) : assemble_edit(P, s);
  if (rc == 0 && W->cg) {   /* after the parse and the mask; settled before the next parse reuses b */
    rc = hpgq_cgr_fill_device(W->cg, &b[0], o->filter_on ? W->d_mask : NULL,
                              o->filter_on ? HPGQ_CGR_ONLY_VALID_READS : HPGQ_CGR_ALL_READS);
    if (rc == 0) rc = hpgq_cgr_sync(W->cg);
    if (rc == 0) W->cg_exact_calls += hpgq_cgr_last_exact(W->cg);
  }
  W->num_reads += (uint64_t)na;
  return rc;
}

static void *worker_main(void *arg) {
  worker_t *W = arg;
  pipe_t *P = W->P;
  const int writes = P->o->command != CMD_STATS;
  for (int64_t k = W->w;; k += P->nworkers) {
    slot_t *s = &P->slot[k % P->nslots];
    pthread_mutex_lock(&P->mu);
    while (!(s->state == 1 && s->chunk == k) && !P->error && !(P->reader_done && k >= P->chunks))
      pthread_cond_wait(&P->cv, &P->mu);
    /* (after a pairing error the chunks before it are still checked: the error
     * line names the first bad pair of the whole input) */
    const int stop = (P->error && !(P->error == HPGQ_E_PAIRING && k < P->bad_chunk)) ||
                     !(s->state == 1 && s->chunk == k);
    pthread_mutex_unlock(&P->mu);
    if (stop) break;
    trace_at(P, k, 2, W->w);
    const size_t use = s->use + (P->nsides == 2 ? s->use2 : 0);   /* (s is the copiers' once place_and_copy handed it over) */
    int handed = 0;
    int rc = worker_chunk(W, s);
    if (rc == 0 && writes && P->mmap_out) {
      rc = place_and_copy(P, s, &handed);   /* (an empty chunk is placed too: input order) */
    }
    trace_at(P, k, 4, -1);
    W->fastq_bytes += (double)use;
    pthread_mutex_lock(&P->mu);
    if (rc && !P->error) P->error = rc;
    if (!handed) s->state = writes && rc == 0 && !P->mmap_out ? 2 : 0;   /* (handed: the copiers free it) */
    pthread_cond_broadcast(&P->cv);
    pthread_mutex_unlock(&P->mu);
    if (rc) {
      W->rc = rc;
      break;
    }
  }
  return NULL;
}

/* dst (nm sets, layout of lmax ld) += src (nm sets, layout of lmax ls <= ld):
 * the workers' full-length counter sets (hpgq_read_counters_ext) */
static void add_relayout(uint64_t *dst, int ld, const uint64_t *src, int ls, int nm) {
  for (int m = 0; m < nm; ++m) {
    uint64_t *d = dst + (size_t)m * hpgq_counters_len(ld);
    const uint64_t *x = src + (size_t)m * hpgq_counters_len(ls);
    for (int i = 0; i < HPGQ_NUM_SCALARS; ++i) d[i] += x[i];
    for (int i = 0; i <= ls; ++i) d[hpgq_off_hist_len(ld) + i] += x[hpgq_off_hist_len(ls) + i];
    for (int i = 0; i < HPGQ_MEANQ_BINS; ++i) d[hpgq_off_hist_meanq(ld) + i] += x[hpgq_off_hist_meanq(ls) + i];
    for (int i = 0; i < HPGQ_GC_BINS; ++i) d[hpgq_off_hist_gc(ld) + i] += x[hpgq_off_hist_gc(ls) + i];
    for (int i = 0; i < ls; ++i) d[hpgq_off_pos_qsum(ld) + i] += x[hpgq_off_pos_qsum(ls) + i];
    for (int b = 0; b < 5; ++b)
      for (int i = 0; i < ls; ++i) d[hpgq_off_pos_base(ld, b) + i] += x[hpgq_off_pos_base(ls, b) + i];
  }
}

static void close_inputs(const reader_input_t *in) {
  for (int m = 0; m < 2; ++m)
    if (in[m].fd >= 0) close(in[m].fd);
}

int cli_run(const cli_options_t *o, const hpgq_params_t *p, cli_result_t *res) {
  pipe_t P;
  memset(&P, 0, sizeof(P));
  P.trace = getenv("HPGQ_TRACE") != NULL;
  P.o = o;
  memset(res, 0, sizeof(*res));
  res->bad_pair = -1;
  /* the mates and the sides they come on: --fq1 + --fq2 are two sides, an
   * --interleaved file two mates on one, single-end input one mate on one */
  P.nmates = p->paired ? 2 : 1;
  P.nsides = o->in_filename2 ? 2 : 1;
  P.bad_pair = -1;
  reader_input_t in[2] = {{-1, 0, o->in_filename}, {-1, 0, o->in_filename2}};
  for (int m = 0; m < P.nsides; ++m) {
    struct stat st;
    in[m].fd = open(in[m].name, O_RDONLY);
    if (in[m].fd < 0 || fstat(in[m].fd, &st)) {
      close_inputs(in);
      return HPGQ_E_INVALID;
    }
    in[m].size = st.st_size;
  }
  pthread_mutex_init(&P.mu, NULL);
  pthread_cond_init(&P.cv, NULL);
  pthread_mutex_init(&P.cq_mu, NULL);
  pthread_cond_init(&P.cq_cv, NULL);

  /* GPU workers: --gpu-workers per device on --gpus devices (0: every visible
   * one); worker w on device (gpu + w mod ngpus) mod ndev */
  const int ndev = hpgq_device_count();
  if (ndev <= 0) {
    close_inputs(in);
    return HPGQ_E_NO_DEVICE;
  }
  const int ngpus = o->num_gpus > 0 ? o->num_gpus : ndev;
  int G = ngpus * (o->gpu_workers > 0 ? o->gpu_workers : 1);
  if (G > MAX_WORKERS) G = MAX_WORKERS;
  P.nworkers = G;
  /* one slot per worker + the reader's + the writer's + one to run ahead (a
   * bound that does not double with the worker count: 16 workers of 256 MB
   * chunks would otherwise pin 10 GB) */
  P.nslots = G + 3;
  if (P.nslots > MAX_SLOTS) P.nslots = MAX_SLOTS;
  bind_numa(o, ngpus, ndev);
  const int64_t cg_batch = o->cg_on ? o->cg_batch_size : 0;   /* --cg: bytes of FASTQ text per chaos-game call */
  worker_t W[MAX_WORKERS];
  memset(W, 0, sizeof(W));
  int rc = 0;
  for (int w = 0; w < G && rc == 0; ++w) {
    W[w].P = &P;
    W[w].p = p;
    W[w].w = w;
    W[w].device = (o->device + w % ngpus) % ndev;
    rc = worker_open(&W[w]);
  }
  /* a chunk holds --chunk-mb of text (with --cg: one chaos-game batch) */
  size_t chunk = (size_t)o->chunk_mb << 20;
  if (cg_batch > 0 && (size_t)cg_batch > chunk) chunk = (size_t)cg_batch;
  const double pinned_gb = (double)P.nslots * (double)P.nsides * (double)(chunk + MAX_CARRY) / 1e9;
  if (pinned_gb > 4.0)
    fprintf(stderr, "hpg-fastq: %d chunks of %zu MB: %.1f GB of page-locked host memory\n", P.nslots,
            (chunk + MAX_CARRY) >> 20, pinned_gb);
  for (int i = 0; i < P.nslots && rc == 0; ++i) {
    P.slot[i].cap = chunk + MAX_CARRY;
    rc = hpgq_host_alloc((void **)&P.slot[i].buf, P.slot[i].cap);
    if (rc == 0 && P.nsides == 2) rc = hpgq_host_alloc((void **)&P.slot[i].buf2, P.slot[i].cap);
  }
  if (rc == 0)
    rc = reader_open(&P.rd, in, P.nsides, P.nmates, chunk, cg_batch, o->num_threads, MAX_CARRY, SPLIT_MIN);
  const int writes = o->command != CMD_STATS;
  const int edit = o->command == CMD_EDIT;
  if (rc == 0 && writes) {
    /* passed.fq (edit.fq) and failed.fq (edit: with a filter only); paired input:
     * passed_1.fq / passed_2.fq (edit_1 / edit_2), failed_1.fq / failed_2.fq.
     * "w+": read + write, which a shared writable mapping needs (an O_WRONLY
     * descriptor cannot be mapped) */
    static const char *const suffix[3] = {"", "_1", "_2"};
    for (int i = 0; i < 2 * P.nmates; ++i) {
      char path[4096];
      if (i % 2 && edit && !o->filter_on) continue;
      snprintf(path, sizeof(path), "%s/%s%s.fq", o->out_dirname, i % 2 ? "failed" : edit ? "edit" : "passed",
               suffix[p->paired ? 1 + i / 2 : 0]);
      P.out[i] = fopen(path, "w+");
      if (!P.out[i]) rc = HPGQ_E_INVALID;
      else setvbuf(P.out[i], NULL, _IOFBF, 16 << 20);
    }
    /* --merge-overlap: the merged reads' own pair of files */
    for (int c = 0; c < 2 && rc == 0 && o->ovl_merge_on; ++c) {
      char path[4096];
      if (c && !o->filter_on) continue;
      snprintf(path, sizeof(path), "%s/%s_merged.fq", o->out_dirname, c ? "failed" : "edit");
      P.out[4 + c] = fopen(path, "w+");
      if (!P.out[4 + c]) rc = HPGQ_E_INVALID;
      else setvbuf(P.out[4 + c], NULL, _IOFBF, 16 << 20);
    }
    /* (paired output goes through the stream writer: the mapped path is two-output) */
    if (rc == 0 && !o->stream_writer && !p->paired) {   /* not mappable (1): the writer thread */
      const int m = map_outputs(&P, in[0].size);
      if (m < 0) rc = m;
    }
    res->writer = P.mmap_out ? 1 : 2;
    if (P.trace && P.mmap_out)
      fprintf(stderr, "hpg-fastq: writer: mapped output files, parallel copy (windows reserved by %s)\n",
              mapout_mode_name[__atomic_load_n(&P.mo.mode, __ATOMIC_RELAXED)]);
    else if (P.trace)
      fprintf(stderr, "hpg-fastq: writer: one stream writer thread\n");
  }
  if (rc) goto done;

  const double t0 = now_s();
  P.t0 = t0;
  if (P.mmap_out && (rc = start_copiers(&P))) goto done;
  pthread_t reader, writer;
  pthread_create(&reader, NULL, reader_main, &P);
  const int writer_thread = writes && !P.mmap_out;
  if (writer_thread) pthread_create(&writer, NULL, writer_main, &P);
  for (int w = 0; w < G; ++w) pthread_create(&W[w].th, NULL, worker_main, &W[w]);
  for (int w = 0; w < G; ++w) pthread_join(W[w].th, NULL);
  /* (a worker that stopped on an error left P.error set: reader and writer end) */
  pthread_mutex_lock(&P.mu);
  pthread_cond_broadcast(&P.cv);
  pthread_mutex_unlock(&P.mu);
  pthread_join(reader, NULL);
  if (writer_thread) pthread_join(writer, NULL);
  if (P.mmap_out) stop_copiers(&P);   /* every placed chunk is in the maps */
  for (int w = 0; w < G && rc == 0; ++w) rc = W[w].rc;
  /* (the reader's and writer's generic -1 is HPGQ_E_INVALID; a copier's or the
   * prefault threads' HPGQ_E_IO stays what it is) */
  if (rc == 0 && P.error)
    rc = P.error < 0 && P.error != HPGQ_E_FORMAT && P.error != HPGQ_E_IO && P.error != HPGQ_E_PAIRING
             ? HPGQ_E_INVALID
             : P.error;
  if (rc == HPGQ_E_PAIRING) {
    res->bad_pair = P.bad_pair;
    snprintf(res->pairing_msg, sizeof(res->pairing_msg), "%s", P.pairing_msg);
  }

  /* the read-sharded merge: device counters, k-mer and CGR tables summed over
   * the workers (u64; CGR u32, which wraps like the reference's tables).  The
   * counters and k-mer tables come at full length (the long-read tails,
   * hpgq_read_counters_ext / hpgq_kmers_read_ext): each worker's in the
   * layout of its own longest read, summed into the longest one's */
  const int nm = p->paired ? 2 : 1;
  int L = p->lmax, KP = 0;
  for (int w = 0; w < G && rc == 0; ++w) {
    int32_t lw = 0;
    rc = hpgq_read_counters_ext(W[w].ctx, NULL, 0, &lw);
    if (lw > L) L = lw;
    if (rc == 0 && o->kmers_on) rc = hpgq_kmers_read_ext(W[w].km, NULL, 0, &lw);
    if (o->kmers_on && lw > KP) KP = lw;
  }
  res->lmax = L;
  res->counters = rc == 0 ? calloc(hpgq_counters_len(L) * nm, sizeof(uint64_t)) : NULL;
  if (rc == 0 && !res->counters) rc = HPGQ_E_NOMEM;
  for (int w = 0; w < G && rc == 0; ++w) {
    int32_t lw = 0;
    rc = hpgq_read_counters_ext(W[w].ctx, NULL, 0, &lw);
    uint64_t *part = rc == 0 ? calloc(hpgq_counters_len(lw) * nm, sizeof(uint64_t)) : NULL;
    if (rc == 0 && !part) rc = HPGQ_E_NOMEM;
    if (rc == 0) rc = hpgq_read_counters_ext(W[w].ctx, part, hpgq_counters_len(lw) * nm, &lw);
    if (rc == 0) add_relayout(res->counters, L, part, lw, nm);
    free(part);
    res->num_reads += W[w].num_reads;
    res->fastq_bytes += W[w].fastq_bytes;
    res->cg_exact_calls += W[w].cg_exact_calls;
  }
  if (rc == 0 && o->kmers_on) {
    res->kmers_npos = KP;
    res->kmers = calloc((size_t)HPGQ_NUM_KMERS * KP + 1, sizeof(uint64_t));
    if (!res->kmers) rc = HPGQ_E_NOMEM;
    for (int w = 0; w < G && rc == 0; ++w) {
      int32_t pw = 0;
      rc = hpgq_kmers_read_ext(W[w].km, NULL, 0, &pw);
      uint64_t *kp = rc == 0 ? calloc((size_t)HPGQ_NUM_KMERS * pw + 1, sizeof(uint64_t)) : NULL;
      if (rc == 0 && !kp) rc = HPGQ_E_NOMEM;
      if (rc == 0) rc = hpgq_kmers_read_ext(W[w].km, kp, (size_t)HPGQ_NUM_KMERS * pw, &pw);
      for (int id = 0; rc == 0 && id < HPGQ_NUM_KMERS; ++id)
        for (int j = 0; j < pw; ++j) res->kmers[(size_t)id * KP + j] += kp[(size_t)id * pw + j];
      free(kp);
    }
  }
  /* --quality-dist: per mate, the workers' tables added into one of the
   * longest worker's rows (hpgq_qdist_add) */
  for (int m = 0; m < nm && rc == 0 && o->quality_dist_on; ++m) {
    int32_t np = 0;
    for (int w = 0; w < G && rc == 0; ++w) {
      int32_t pw = 0;
      rc = hpgq_qdist_read(W[w].qd[m], NULL, 0, &pw);
      if (pw > np) np = pw;
    }
    res->qdist_npos[m] = np;
    res->qdist[m] = rc == 0 ? calloc((size_t)HPGQ_QDIST_VALUES * np + 1, sizeof(uint64_t)) : NULL;
    if (rc == 0 && !res->qdist[m]) rc = HPGQ_E_NOMEM;
    uint64_t *part = rc == 0 ? calloc((size_t)HPGQ_QDIST_VALUES * np + 1, sizeof(uint64_t)) : NULL;
    if (rc == 0 && !part) rc = HPGQ_E_NOMEM;
    for (int w = 0; w < G && rc == 0; ++w) {
      int32_t pw = 0;
      rc = hpgq_qdist_read(W[w].qd[m], part, (size_t)HPGQ_QDIST_VALUES * np, &pw);
      if (rc == 0) rc = hpgq_qdist_add(res->qdist[m], np, part, pw);
    }
    free(part);
  }
  /* --clip-adapters: per mate, the workers' scalars added */
  for (int m = 0; m < nm && rc == 0 && o->clip_on; ++m) {
    res->clip_on = 1;
    for (int w = 0; w < G && rc == 0; ++w) {
      hpgq_clip_info_t info;
      rc = hpgq_clip_read(W[w].cl[m], &info);
      if (rc) break;
      res->clip[m].reads += info.reads;
      res->clip[m].clipped += info.clipped;
      res->clip[m].bases_removed += info.bases_removed;
      for (int a = 0; a < HPGQ_ADAPT_MAX_PROBES; ++a) res->clip[m].by_probe[a] += info.by_probe[a];
      res->clip[m].nprobes = info.nprobes;
      res->clip[m].min_overlap = info.min_overlap;
    }
  }
  /* --clip-overlap: the workers' scalars added */
  for (int w = 0; w < G && rc == 0 && o->ovl_on; ++w) {
    hpgq_ovl_info_t info;
    res->ovl_on = 1;
    rc = hpgq_ovl_read(W[w].ov, &info);
    if (rc) break;
    res->ovl.pairs += info.pairs;
    res->ovl.skipped += info.skipped;
    res->ovl.overlapping += info.overlapping;
    res->ovl.clipped += info.clipped;
    res->ovl.bases_removed[0] += info.bases_removed[0];
    res->ovl.bases_removed[1] += info.bases_removed[1];
    res->ovl.min_overlap = info.min_overlap;
    res->ovl.max_mismatches = info.max_mismatches;
  }
  /* --correct-overlap, --insert-size: the workers' scalars and histograms added */
  for (int w = 0; w < G && rc == 0 && o->ovl_fix_on; ++w) {
    hpgq_ovl_correct_info_t fix;
    res->ovl_fix_on = 1;
    rc = hpgq_ovl_read_correct(W[w].ov, &fix);
    if (rc) break;
    res->ovl_fix.corrected_pairs += fix.corrected_pairs;
    res->ovl_fix.corrected_bases[0] += fix.corrected_bases[0];
    res->ovl_fix.corrected_bases[1] += fix.corrected_bases[1];
    res->ovl_fix.on = fix.on;
    res->ovl_fix.phred = fix.phred;
    res->ovl_fix.high = fix.high;
    res->ovl_fix.low = fix.low;
  }
  /* --merge-overlap: the workers' four scalars added, and what their single-end ctxs counted */
  for (int w = 0; w < G && rc == 0 && o->ovl_merge_on; ++w) {
    hpgq_ovl_merge_info_t mi;
    res->ovl_merge_on = 1;
    rc = hpgq_ovl_read_merge(W[w].ov, &mi);
    if (rc) break;
    res->ovl_merge.merged_pairs += mi.merged_pairs;
    res->ovl_merge.merged_bases += mi.merged_bases;
    res->ovl_merge.resolved[0] += mi.resolved[0];
    res->ovl_merge.resolved[1] += mi.resolved[1];
    const size_t nc = hpgq_counters_size(W[w].ctx2);
    uint64_t *part = calloc(nc, sizeof(uint64_t));
    if (!part) rc = HPGQ_E_NOMEM;
    if (rc == 0) rc = hpgq_read_counters(W[w].ctx2, part, nc);
    if (rc == 0) {
      res->merged_passed += part[HPGQ_S_NUM_PASSED];
      res->merged_failed += part[HPGQ_S_NUM_FAILED];
    }
    free(part);
  }
  for (int w = 0; w < G && rc == 0 && o->ovl_insert_on; ++w) {
    uint64_t *hist = malloc(sizeof(uint64_t) * HPGQ_OVL_INSERT_BINS);
    res->ovl_insert_on = 1;
    rc = hist ? hpgq_ovl_read_inserts(W[w].ov, hist) : HPGQ_E_NOMEM;
    for (int f = 0; f < HPGQ_OVL_INSERT_BINS && rc == 0; ++f) res->ovl_inserts[f] += hist[f];
    free(hist);
  }
  /* --adapters: per mate, the workers' tables added at the longest worker's
   * positions (hpgq_adapt_add), and the two scalars added */
  for (int m = 0; m < nm && rc == 0 && o->adapters_on; ++m) {
    const size_t na = (size_t)o->adapter_n;
    int32_t np = 0;
    hpgq_adapt_info_t info;
    for (int w = 0; w < G && rc == 0; ++w) {
      rc = hpgq_adapt_read(W[w].ad[m], NULL, 0, &info);
      if (rc == 0 && info.npos > np) np = info.npos;
    }
    res->adapt_npos[m] = np;
    res->adapt[m] = rc == 0 ? calloc(na * (size_t)np + 1, sizeof(uint64_t)) : NULL;
    if (rc == 0 && !res->adapt[m]) rc = HPGQ_E_NOMEM;
    uint64_t *part = rc == 0 ? calloc(na * (size_t)np + 1, sizeof(uint64_t)) : NULL;
    if (rc == 0 && !part) rc = HPGQ_E_NOMEM;
    for (int w = 0; w < G && rc == 0; ++w) {
      rc = hpgq_adapt_read(W[w].ad[m], part, na * (size_t)np, &info);
      if (rc == 0) rc = hpgq_adapt_add(res->adapt[m], np, part, info.npos, (int)na);
      if (rc == 0) {
        res->adapt_reads[m] += info.reads;
        res->adapt_with_any[m] += info.with_any;
      }
    }
    free(part);
  }
  /* --duplication: per mate, every other worker's table exported and imported
   * into worker 0's (levels of shards cannot be added: one sequence may be in
   * several), then the levels, and for --duplication-out the table itself;
   * --overrepresented takes its list from the merged table (overrep_list) */
  for (int m = 0; m < nm && rc == 0 && (o->duplication_on || o->overrep_on); ++m) {
    /* (a representative that did not fit in a worker's arena: HPGQ_E_NOMEM here) */
    for (int w = 0; w < G && rc == 0 && o->overrep_on; ++w) {
      rc = hpgq_dup_sync(W[w].dp[m]);
      if (rc == HPGQ_E_NOMEM) res->overrep_error = 1;
    }
    for (int w = 1; w < G && rc == 0; ++w) rc = dup_move(W[0].dp[m], W[w].dp[m]);
    if (rc == 0) rc = hpgq_dup_levels(W[0].dp[m], &res->dup_levels[m]);
    if (rc == 0 && o->duplication_out)
      rc = dup_sorted(W[0].dp[m], &res->dup_keys[m], &res->dup_counts[m], &res->dup_n[m]);
    res->dup_on = rc == 0 && o->duplication_on;
    if (rc == 0 && o->overrep_on) rc = overrep_list(o, W, G, m, res);
    res->overrep_on = rc == 0 && o->overrep_on;
  }
  if (rc == 0 && o->cg_on) {
    const size_t cells = (size_t)1 << (2 * o->k_cg);
    res->cg_seq = calloc(cells, sizeof(uint32_t));
    res->cg_q = calloc(cells, sizeof(uint32_t));
    uint32_t *ts = calloc(cells, sizeof(uint32_t)), *tq = calloc(cells, sizeof(uint32_t));
    if (!res->cg_seq || !res->cg_q || !ts || !tq) rc = HPGQ_E_NOMEM;
    for (int w = 0; w < G && rc == 0; ++w) {
      uint32_t words = 0;
      rc = hpgq_cgr_read(W[w].cg, ts, tq, &words);
      for (size_t i = 0; rc == 0 && i < cells; ++i) {
        res->cg_seq[i] += ts[i];
        res->cg_q[i] += tq[i];
      }
      res->cg_words += words;
    }
    free(ts);
    free(tq);
  }
  if (P.mmap_out) unmap_outputs(&P, &rc);   /* the files at their final sizes (inside the clock) */
  res->seconds = now_s() - t0;
  res->num_gpus = G;
  for (int64_t k = 0; P.trace && k < P.chunks && k < TRACE_MAX; ++k)
    fprintf(stderr,
            "trace chunk %lld: read %.1f-%.1f ms, worker %d %.1f-%.1f (parsed %.1f, sync %.1f-%.1f, placed %.1f) ms\n",
            (long long)k, 1e3 * P.tr[k][0], 1e3 * P.tr[k][1], P.tw[k], 1e3 * P.tr[k][2], 1e3 * P.tr[k][4],
            1e3 * P.tr[k][5], 1e3 * P.tr[k][3], 1e3 * P.tr[k][6], 1e3 * P.tr[k][7]);
  if (rc == 0) {
    res->num_passed = res->counters[HPGQ_S_NUM_PASSED];
    res->num_failed = res->counters[HPGQ_S_NUM_FAILED];
    res->num_edited = res->counters[HPGQ_S_NUM_EDITED];
  }

done:
  if (P.ncopiers) stop_copiers(&P);
  if (P.mmap_out) unmap_outputs(&P, &rc);
  for (int i = 0; i < 6; ++i)
    if (P.out[i]) fclose(P.out[i]);
  for (int i = 0; i < P.nslots; ++i) {
    hpgq_host_free(P.slot[i].buf);
    hpgq_host_free(P.slot[i].buf2);
    free_results(&P.slot[i]);
    free(P.slot[i].parts);
    for (int c = 0; c < 6; ++c) free(P.slot[i].out[c]);
  }
  reader_close(P.rd);
  close_inputs(in);
  free(P.cq);
  for (int w = 0; w < G; ++w) worker_close(&W[w]);
  return rc;
}
