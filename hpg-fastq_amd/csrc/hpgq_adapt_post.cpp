// hpgq_adapt_post.cpp — host side of `stats --adapters`: the
// probe rules, the default set, one probe's first occurrence in a byte string,
// and merging tables.  HIP-free, no device.
//
// A table is first[a * npos + p] u64: counted reads in which probe a occurs
// for the first time at position p.
#include <cstdint>
#include <cstring>

#include "../../include/hpgq.h"

namespace {
// the probe's length, or -1 if it breaks the rules (8 .. 32 bytes, each A C G T)
int probe_len(const char *probe) {
  if (!probe) return -1;
  int k = 0;
  for (; probe[k]; ++k) {
    if (k == HPGQ_ADAPT_MAX_LEN) return -1;
    const char c = probe[k];
    if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return -1;
  }
  return k >= HPGQ_ADAPT_MIN_LEN ? k : -1;
}

struct Default { const char *name, *probe; };
// the first 12 bases of the adapters common QC tools look for
const Default kDefaults[] = {
    {"Illumina Universal Adapter", "AGATCGGAAGAG"},
    {"Illumina Small RNA 3' Adapter", "TGGAATTCTCGG"},
    {"Illumina Small RNA 5' Adapter", "GATCGTCGGACT"},
    {"Nextera Transposase Sequence", "CTGTCTCTTATA"},
    {"PolyA", "AAAAAAAAAAAA"},
    {"PolyG", "GGGGGGGGGGGG"},
};
constexpr int kNumDefaults = (int)(sizeof(kDefaults) / sizeof(kDefaults[0]));
}  // namespace

extern "C" {

int hpgq_adapt_add(uint64_t *dst, int npos_dst, const uint64_t *src, int npos_src, int nprobes) {
  if (npos_dst < 0 || npos_src < 0 || npos_src > npos_dst || nprobes < 0 || nprobes > HPGQ_ADAPT_MAX_PROBES)
    return HPGQ_E_INVALID;
  if (npos_src == 0 || nprobes == 0) return HPGQ_OK;
  if (!dst || !src) return HPGQ_E_INVALID;
  for (int a = 0; a < nprobes; ++a) {
    uint64_t *d = dst + (size_t)a * (size_t)npos_dst;
    const uint64_t *s = src + (size_t)a * (size_t)npos_src;
    for (int p = 0; p < npos_src; ++p) d[p] += s[p];
  }
  return HPGQ_OK;
}

int64_t hpgq_adapt_find(const void *s, size_t n, const char *probe) {
  const int k = probe_len(probe);
  if (k < 0) return -2;
  if (!s || n < (size_t)k) return -1;
  const unsigned char *b = static_cast<const unsigned char *>(s);
  for (size_t j = 0; j + (size_t)k <= n; ++j)
    if (b[j] == (unsigned char)probe[0] && std::memcmp(b + j, probe, (size_t)k) == 0) return (int64_t)j;
  return -1;
}

int hpgq_adapt_default(int i, const char **name, const char **probe) {
  if (i >= 0 && i < kNumDefaults) {
    if (name) *name = kDefaults[i].name;
    if (probe) *probe = kDefaults[i].probe;
  }
  return kNumDefaults;
}

}  // extern "C"
