// hpgq_dup_post.cpp — host side of `stats --duplication`: the
// fingerprint of one sequence and the levels of a list of counts, and of
// `stats --overrepresented` (§2.10): the most frequent of a list of (key, count)
// pairs.  HIP-free, no device.  The kernels (csrc/hpgq_dup.hip) compute the
// first two; hpgq_dup_top sorts its candidates with the third.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/hpgq.h"

namespace {
constexpr uint64_t kG = 0x9E3779B97F4A7C15ULL;
constexpr uint64_t kLo[HPGQ_DUP_LEVELS] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000};

inline uint64_t mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}
}  // namespace

extern "C" {

uint64_t hpgq_dup_fingerprint(const void *s, size_t n) {
  const unsigned char *p = static_cast<const unsigned char *>(s);
  uint64_t sum = 0;
  for (size_t j = 0; 8 * j < n; ++j) {
    const size_t here = n - 8 * j < 8 ? n - 8 * j : 8;
    unsigned char b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(b, p + 8 * j, here);
    uint64_t w = 0;   // little-endian whatever the host is
    for (int k = 7; k >= 0; --k) w = (w << 8) | b[k];
    sum += mix(w + (uint64_t)(j + 1) * kG);
  }
  const uint64_t fp = mix(sum ^ ((uint64_t)n * kG));
  return fp ? fp : 1;
}

uint64_t hpgq_dup_level_bound(int level) { return level < 0 || level >= HPGQ_DUP_LEVELS ? 0 : kLo[level]; }

int hpgq_dup_levels_of(const uint64_t *counts, size_t n, hpgq_dup_levels_t *out) {
  if (!out || (n > 0 && !counts)) return HPGQ_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  for (size_t i = 0; i < n; ++i) {
    const uint64_t c = counts[i];
    if (!c) continue;
    int lv = 0;
    while (lv + 1 < HPGQ_DUP_LEVELS && c >= kLo[lv + 1]) ++lv;
    out->distinct_at[lv] += 1;
    out->reads_at[lv] += c;
    out->distinct += 1;
    out->reads += c;
    if (c > out->max_count) out->max_count = c;
  }
  return HPGQ_OK;
}

int hpgq_dup_top_of(const uint64_t *keys, const uint64_t *counts, size_t n, uint64_t min_count, uint64_t *out_keys,
                    uint64_t *out_counts, size_t cap, size_t *total) {
  if (!total || min_count < 1 || (n > 0 && (!keys || !counts)) || (out_keys && !out_counts)) return HPGQ_E_INVALID;
  try {
    std::vector<std::pair<uint64_t, uint64_t>> hit;   // (count, key)
    for (size_t i = 0; i < n; ++i)
      if (keys[i] && counts[i] >= min_count) hit.emplace_back(counts[i], keys[i]);
    *total = hit.size();
    if (!out_keys) return HPGQ_OK;
    const size_t take = std::min(cap, hit.size());
    // count descending, ties by key ascending
    std::partial_sort(hit.begin(), hit.begin() + take, hit.end(),
                      [](const std::pair<uint64_t, uint64_t> &a, const std::pair<uint64_t, uint64_t> &b) {
                        return a.first != b.first ? a.first > b.first : a.second < b.second;
                      });
    for (size_t i = 0; i < take; ++i) {
      out_keys[i] = hit[i].second;
      out_counts[i] = hit[i].first;
    }
  } catch (const std::bad_alloc &) {
    return HPGQ_E_NOMEM;
  }
  return HPGQ_OK;
}

}  // extern "C"
