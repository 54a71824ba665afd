// hpgq_clip_post.cpp — host side of `edit --clip-adapters`:
// the clip rule on one read.  HIP-free, no device.
//
// Probe a of K bytes matches at j of a read of n bytes iff, with m = min(K, n - j),
// the read's bytes [j, j + m) equal the probe's first m and m == K or
// m >= min_overlap.  c is the lowest j at which any probe matches (n: none), the
// winner the lowest probe that matches there.
#include <cstdint>
#include <cstring>

#include "../../include/hpgq.h"

extern "C" int64_t hpgq_clip_find(const void *s, size_t n, const char *const *probes, int nprobes, int min_overlap,
                                  int *probe) {
  if (probe) *probe = -1;
  if (!probes || nprobes < 1 || nprobes > HPGQ_ADAPT_MAX_PROBES || min_overlap < 1 || min_overlap > HPGQ_ADAPT_MAX_LEN)
    return -2;
  size_t len[HPGQ_ADAPT_MAX_PROBES];
  for (int a = 0; a < nprobes; ++a) {
    if (hpgq_adapt_find(nullptr, 0, probes[a]) == -2) return -2;   // the probe rules of §2.11
    len[a] = std::strlen(probes[a]);
  }
  if (!s) return (int64_t)n;
  const unsigned char *b = static_cast<const unsigned char *>(s);
  for (size_t j = 0; j < n; ++j)
    for (int a = 0; a < nprobes; ++a) {
      const size_t m = len[a] < n - j ? len[a] : n - j;
      if (m != len[a] && m < (size_t)min_overlap) continue;
      if (b[j] == (unsigned char)probes[a][0] && std::memcmp(b + j, probes[a], m) == 0) {
        if (probe) *probe = a;
        return (int64_t)j;
      }
    }
  return (int64_t)n;
}
