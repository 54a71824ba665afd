/*
 * adapt_main.c — hpgq_adapt_find / _add / _default (csrc/hpgq_adapt_post.cpp),
 * the adapter-file parser and the report writer (host/hpgq_report_adapt.c)
 * under ASan + UBSan, no GPU.  Built and run by tests/test_adapt_cpu.py.
 *
 * argv[1]: a text file, one case per line:
 *   F hex probe want      hpgq_adapt_find over the bytes ("-": none) must give want
 *   P path                cli_adapters_load on the file; prints
 *                         "set <rc> <n> name_hex:probe ..." for the test
 *   R base reads with_any nprobes npos  name_hex_1 .. name_hex_nprobes  cell_1 .. cell_(nprobes*npos)
 *                         the table written to <argv[2]>/<base>.adapter.content.data
 * Every input is a heap block of its exact size, so an access past it is caught.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hpgq_cli.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "adapt_main: %s (case %ld)\n", what, line);
  return 1;
}

/* hex -> a heap block of exactly its length ("-": one byte, length 0) */
static unsigned char *unhex(const char *hex, size_t *len) {
  *len = strcmp(hex, "-") ? strlen(hex) / 2 : 0;
  unsigned char *b = malloc(*len ? *len : 1);
  for (size_t j = 0; b && j < *len; ++j) {
    unsigned v;
    if (sscanf(hex + 2 * j, "%2x", &v) != 1) return NULL;
    b[j] = (unsigned char)v;
  }
  return b;
}

int main(int argc, char **argv) {
  if (argc != 3) return fail("usage: adapt_main <cases.txt> <outdir>", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the cases", 0);
  long ncase = 0;
  char kind;
  char *word = malloc(1 << 20);
  if (!word) return fail("out of memory", 0);
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'F') {
      char probe[128];
      long long want;
      size_t n;
      if (fscanf(f, "%1048575s %127s %lld", word, probe, &want) != 3) return fail("bad find case", ncase);
      unsigned char *s = unhex(word, &n);
      char *p = malloc(strlen(probe) + 1);   /* (exact size: the NUL is its last byte) */
      if (!s || !p) return fail("bad bytes", ncase);
      strcpy(p, probe);
      if (hpgq_adapt_find(s, n, p) != want) return fail("wrong position", ncase);
      free(s);
      free(p);
    } else if (kind == 'P') {
      cli_options_t *o = calloc(1, sizeof(*o));
      if (!o || fscanf(f, "%1048575s", word) != 1) return fail("bad parser case", ncase);
      o->adapter_file = word;
      const int rc = cli_adapters_load(o);
      printf("set %d %d", rc, rc ? 0 : o->adapter_n);
      for (int a = 0; rc == 0 && a < o->adapter_n; ++a) {
        printf(" ");
        for (const char *c = o->adapter_names[a]; *c; ++c) printf("%02x", (unsigned char)*c);
        printf(":%s", o->adapter_probes[a]);
      }
      printf("\n");
      free(o);
    } else if (kind == 'R') {
      char base[256];
      uint64_t reads, with_any;
      int nprobes, npos;
      if (fscanf(f, "%255s %" SCNu64 " %" SCNu64 " %d %d", base, &reads, &with_any, &nprobes, &npos) != 5 ||
          nprobes < 0 || npos < 0)
        return fail("bad render case", ncase);
      char **names = malloc((nprobes ? (size_t)nprobes : 1) * sizeof(*names));
      const size_t cells = (size_t)nprobes * (size_t)npos;
      uint64_t *first = malloc((cells ? cells : 1) * sizeof(uint64_t));
      if (!names || !first) return fail("out of memory", ncase);
      for (int a = 0; a < nprobes; ++a) {
        size_t n;
        if (fscanf(f, "%1048575s", word) != 1) return fail("bad name", ncase);
        unsigned char *b = unhex(word, &n);
        names[a] = malloc(n + 1);
        if (!b || !names[a]) return fail("bad name bytes", ncase);
        memcpy(names[a], b, n);
        names[a][n] = 0;
        free(b);
      }
      for (size_t i = 0; i < cells; ++i)
        if (fscanf(f, "%" SCNu64, &first[i]) != 1) return fail("bad cell", ncase);
      cli_options_t *o = calloc(1, sizeof(*o));
      if (!o) return fail("out of memory", ncase);
      o->out_dirname = argv[2];
      if (cli_report_adapt(o, nprobes, (const char *const *)names, first, npos, reads, with_any, base))
        return fail("cli_report_adapt failed", ncase);
      free(o);
      for (int a = 0; a < nprobes; ++a) free(names[a]);
      free(names);
      free(first);
    } else {
      return fail("unknown case kind", ncase);
    }
    ++ncase;
  }
  fclose(f);
  free(word);
  if (!ncase) return fail("no cases", 0);

  /* hpgq_adapt_add: the rows have different lengths; the rest of dst untouched; a longer source rejected */
  const int na = 3, nd = 5, ns = 2;
  uint64_t *dst = malloc((size_t)na * nd * sizeof(uint64_t)), *src = malloc((size_t)na * ns * sizeof(uint64_t));
  if (!dst || !src) return fail("out of memory", -1);
  for (int i = 0; i < na * nd; ++i) dst[i] = (uint64_t)i;
  for (int i = 0; i < na * ns; ++i) src[i] = 1000u + (uint64_t)i;
  if (hpgq_adapt_add(dst, nd, src, ns, na) != HPGQ_OK) return fail("hpgq_adapt_add failed", -1);
  for (int a = 0; a < na; ++a)
    for (int p = 0; p < nd; ++p)
      if (dst[a * nd + p] != (uint64_t)(a * nd + p) + (p < ns ? 1000u + (uint64_t)(a * ns + p) : 0)) return fail("wrong sum", a);
  if (hpgq_adapt_add(src, ns, dst, nd, na) != HPGQ_E_INVALID) return fail("a longer source was accepted", -1);
  if (hpgq_adapt_add(dst, nd, src, 0, na) != HPGQ_OK || hpgq_adapt_add(NULL, 0, NULL, 0, na) != HPGQ_OK)
    return fail("the empty table was rejected", -1);
  free(dst);
  free(src);

  /* the default set: six probes that follow the rules */
  const char *name = NULL, *probe = NULL;
  const int nd6 = hpgq_adapt_default(-1, &name, &probe);
  if (nd6 != 6 || name || probe) return fail("wrong default count", -1);
  for (int i = 0; i < nd6; ++i) {
    if (hpgq_adapt_default(i, &name, &probe) != 6 || !name || !probe || strlen(probe) != 12 ||
        hpgq_adapt_find(probe, 12, probe) != 0)
      return fail("bad default probe", i);
  }
  printf("adapt_main: ok %ld cases\n", ncase);
  return 0;
}
