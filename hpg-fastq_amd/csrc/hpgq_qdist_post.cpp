// hpgq_qdist_post.cpp — host side of `stats --quality-dist`:
// merging tables and reading one as qualities.  HIP-free, no device.
//
// A table is hist[p * 256 + b] u64: bases with raw quality byte b at read
// position p.  It knows nothing of phred; quirk Q13 (signed char) applies only
// here, where a byte becomes the quality Q = (signed char)b - phred.
#include <cstdint>

#include "../../include/hpgq.h"

namespace {
// the byte at rank i of the ascending signed order: 128..255 (Q13: negative), then 0..127
inline int byte_at(int i) { return (i + 128) & 255; }

// max(1, ceil(num * c / den)), exact for every u64 c (num < den <= 10)
inline uint64_t rank_of(uint64_t c, unsigned num, unsigned den) {
  const unsigned __int128 x = (unsigned __int128)c * num + (den - 1);
  const uint64_t r = (uint64_t)(x / den);
  return r ? r : 1;
}
}  // namespace

extern "C" {

int hpgq_qdist_add(uint64_t *dst, int npos_dst, const uint64_t *src, int npos_src) {
  if (npos_dst < 0 || npos_src < 0 || npos_src > npos_dst) return HPGQ_E_INVALID;
  if (npos_src == 0) return HPGQ_OK;
  if (!dst || !src) return HPGQ_E_INVALID;
  const size_t n = (size_t)npos_src * HPGQ_QDIST_VALUES;
  for (size_t i = 0; i < n; ++i) dst[i] += src[i];
  return HPGQ_OK;
}

int hpgq_qdist_quantiles(const uint64_t *hist, int npos, int phred, hpgq_qdist_row_t *rows) {
  if (npos < 0 || (npos > 0 && (!hist || !rows))) return HPGQ_E_INVALID;
  static const unsigned kNum[5] = {1, 1, 1, 3, 9}, kDen[5] = {10, 4, 2, 4, 10};
  for (int p = 0; p < npos; ++p) {
    const uint64_t *h = hist + (size_t)p * HPGQ_QDIST_VALUES;
    hpgq_qdist_row_t r = {0, 0, 0, 0, 0, 0, 0, 0};
    // the row sum of counted bases fits u64 by construction; a table put
    // together by hand may not: the sum is taken in 128 bits and must fit
    unsigned __int128 c = 0;
    for (int b = 0; b < HPGQ_QDIST_VALUES; ++b) c += h[b];
    if (c >> 64) return HPGQ_E_INVALID;
    r.count = (uint64_t)c;
    if (r.count) {   // (c == 0: all zeros, quirk Q14's convention)
      int32_t q[5] = {0, 0, 0, 0, 0};
      uint64_t rk[5];
      for (int k = 0; k < 5; ++k) rk[k] = rank_of(r.count, kNum[k], kDen[k]);
      uint64_t cum = 0;
      int k = 0, first = 1;
      for (int i = 0; i < HPGQ_QDIST_VALUES; ++i) {
        const int b = byte_at(i);
        if (!h[b]) continue;
        const int32_t Q = (int32_t)(signed char)(unsigned char)b - phred;
        if (first) {
          r.min = Q;
          first = 0;
        }
        r.max = Q;
        cum += h[b];
        while (k < 5 && cum >= rk[k]) q[k++] = Q;   // (ranks ascend with k)
      }
      r.p10 = q[0];
      r.q1 = q[1];
      r.median = q[2];
      r.q3 = q[3];
      r.p90 = q[4];
    }
    rows[p] = r;
  }
  return HPGQ_OK;
}

}  // extern "C"
