/*
 * hpgq_signature.c — `hpg-fastq signature`: the genomic-signature (GS) file of
 * a FASTA reference, the file `stats --cg --gs-filename` reads
 * (chaos_game_load_table_gs_direct, old/chaos_game.c:297-318).  The old tool's
 * README names such files `<reference>_k=<K>.fg`; its generator is absent, so
 * the rule is this build's (include/hpgq.h).
 *
 * One reader thread fills two page-locked buffers with --chunk-mb pieces of
 * the file, cut at any byte; the main thread hands each piece to
 * hpgq_gs_add_host while the next one is read.  One GPU.
 */
#include <errno.h>
#include <getopt.h>
#include <pthread.h>
#include <semaphore.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>

#include "hpgq_cli.h"

typedef struct {
  FILE *f;
  size_t chunk;
  char *buf[2];
  size_t len[2];
  int io_error;
  sem_t empty[2], full[2];
} sig_reader_t;

static void *sig_reader(void *arg) {
  sig_reader_t *r = arg;
  for (int i = 0;; i ^= 1) {
    sem_wait(&r->empty[i]);
    r->len[i] = fread(r->buf[i], 1, r->chunk, r->f);
    if (r->len[i] < r->chunk && ferror(r->f)) r->io_error = 1;
    const int last = r->len[i] == 0 || r->io_error;
    if (last) r->len[i] = 0;
    sem_post(&r->full[i]);
    if (last) break;
  }
  return NULL;
}

static void sig_usage(const char *exec_name) {
  printf("\nUsage: %s signature --fasta-file <ref.fa> [options]\n\n", exec_name);
  printf("  -f, --fasta-file=<file>         Input FASTA file (plain text)\n");
  printf("  -o, --outdir=<file>             Output directory name\n");
  printf("  --k=<int>                       Word size of the genomic signature, 1..12 (default 7)\n");
  printf("  --gs-filename=<file>            Output file (default <outdir>/<input name>_k=<k>.fg)\n");
  printf("  --gpu=<int>                     GPU to use (default 0)\n");
  printf("  --chunk-mb=<int>                FASTA text per piece (default 64)\n");
  printf("  --print-params                  Print k, the input and the output path and exit\n");
  printf("  --quiet                         Print nothing but errors\n");
  exit(-1);
}

static double sig_now(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int cli_signature(const char *exec_name, int argc, char **argv) {
  enum { S_K = 1000, S_GS, S_GPU, S_CHUNK, S_PRINT, S_QUIET };
  static const struct option longopts[] = {
      {"help", no_argument, 0, 'h'},
      {"fasta-file", required_argument, 0, 'f'},
      {"outdir", required_argument, 0, 'o'},
      {"k", required_argument, 0, S_K},
      {"gs-filename", required_argument, 0, S_GS},
      {"gpu", required_argument, 0, S_GPU},
      {"chunk-mb", required_argument, 0, S_CHUNK},
      {"print-params", no_argument, 0, S_PRINT},
      {"quiet", no_argument, 0, S_QUIET},
      {0, 0, 0, 0}};
  const char *in = NULL, *outdir = ".", *gs_name = NULL;
  int k = 7, device = 0, chunk_mb = 64, print_params = 0, quiet = 0;
  optind = 1;
  int c;
  while ((c = getopt_long(argc, argv, "hf:o:", longopts, NULL)) != -1) {
    switch (c) {
      case 'f': in = optarg; break;
      case 'o': outdir = optarg; break;
      case S_K: k = atoi(optarg); break;
      case S_GS: gs_name = optarg; break;
      case S_GPU: device = atoi(optarg); break;
      case S_CHUNK: chunk_mb = atoi(optarg); break;
      case S_PRINT: print_params = 1; break;
      case S_QUIET: quiet = 1; break;
      default: sig_usage(exec_name);
    }
  }
  if (!in) {
    printf("\nError: Input file name not found !\n");
    sig_usage(exec_name);
  }
  if (k < 1 || k > 12) {
    printf("\nError: --k must be in 1..12\n");
    return 1;
  }
  if (chunk_mb < 1 || chunk_mb > 1536) {
    printf("\nError: --chunk-mb must be in 1..1536\n");
    return 1;
  }
  char out[4096];
  if (gs_name) {
    snprintf(out, sizeof(out), "%s", gs_name);
  } else {
    const char *base = strrchr(in, '/');
    base = base ? base + 1 : in;
    snprintf(out, sizeof(out), "%s/%s_k=%d.fg", outdir, base, k);
  }
  if (print_params) {
    printf("k=%d input=%s output=%s\n", k, in, out);
    return 0;
  }
  FILE *f = fopen(in, "rb");
  if (!f) {
    printf("\nError: Input file name not found !\n");
    return 1;
  }
  if (!gs_name) (void)mkdir(outdir, 0777);   /* (an existing directory stays as it is) */

  const double t0 = sig_now();
  int rc = 0;
  hpgq_gs_t *gs = NULL;
  sig_reader_t r;
  memset(&r, 0, sizeof(r));
  r.f = f;
  r.chunk = (size_t)chunk_mb << 20;
  uint32_t *table = NULL;
  pthread_t th;
  int started = 0, sems = 0;
  double bytes = 0, secs = 0;
  hpgq_gs_info_t info;
  if ((rc = hpgq_gs_open(&gs, device, k, NULL)) != 0) goto done;
  for (int i = 0; i < 2; ++i)
    if ((rc = hpgq_host_alloc((void **)&r.buf[i], r.chunk)) != 0) goto done;
  for (int i = 0; i < 2; ++i) {
    sem_init(&r.empty[i], 0, 1);
    sem_init(&r.full[i], 0, 0);
  }
  sems = 1;
  if (pthread_create(&th, NULL, sig_reader, &r)) {
    rc = HPGQ_E_IO;
    goto done;
  }
  started = 1;
  for (int i = 0;; i ^= 1) {
    sem_wait(&r.full[i]);
    if (r.len[i] == 0) break;
    bytes += (double)r.len[i];
    /* after an error the remaining pieces are still drained, so the reader ends */
    if (!rc) rc = hpgq_gs_add_host(gs, r.buf[i], (int64_t)r.len[i]);
    sem_post(&r.empty[i]);
  }
  pthread_join(th, NULL);
  started = 0;
  if (!rc && r.io_error) rc = HPGQ_E_IO;
  if (rc) goto done;

  table = malloc((size_t)4 << (2 * k));
  if (!table) {
    rc = HPGQ_E_NOMEM;
    goto done;
  }
  if ((rc = hpgq_gs_read(gs, table, &info)) != 0) goto done;
  secs = sig_now() - t0;
  if (!quiet) {
    printf("\nGENOMIC SIGNATURE\n");
    printf("=================================================\n");
    printf("Input FASTA        : %s\n", in);
    printf("Word size (k)      : %d\n", k);
    printf("Num. sequences     : %llu\n", (unsigned long long)info.sequences);
    printf("Num. bases (ACGT)  : %llu\n", (unsigned long long)info.bases);
    printf("Num. N             : %llu\n", (unsigned long long)info.ns);
    printf("Num. words         : %llu\n", (unsigned long long)info.words);
  }
  if (info.words >= ((uint64_t)1 << 32)) {
    /* header_gs_t keeps the count in a u32, and so do the table's cells */
    fprintf(stderr,
            "\nError: %llu words do not fit the u32 ref_word_count field of header_gs_t "
            "(old/chaos_game.h:65-70); no file written\n",
            (unsigned long long)info.words);
    rc = HPGQ_E_INVALID;
    goto done;
  }
  if ((rc = hpgq_cgr_write_gs(out, k, table, (uint32_t)info.words)) != 0) goto done;
  if (!quiet) {
    printf("Signature file     : %s\n", out);
    printf("\nThroughput: %.3f GB of FASTA in %.3f s = %.2f GB/s\n", bytes / 1e9, secs,
           secs > 0 ? bytes / 1e9 / secs : 0.0);
    printf("=================================================\n");
  }

done:
  if (started) pthread_join(th, NULL);
  if (sems) {
    for (int i = 0; i < 2; ++i) {
      sem_destroy(&r.empty[i]);
      sem_destroy(&r.full[i]);
    }
  }
  if (rc) fprintf(stderr, "\nError: %s (%d)\n", hpgq_strerror(rc), rc);
  free(table);
  hpgq_gs_close(gs);
  for (int i = 0; i < 2; ++i)
    if (r.buf[i]) hpgq_host_free(r.buf[i]);
  fclose(f);
  return rc ? 1 : 0;
}
