// hpgq_ovl_post.cpp — host side of `edit --clip-overlap`: the
// overlap rule on one pair, §2.14's correction of one pair and §2.15's merge of
// one pair.  HIP-free, no device.
//
// For a candidate insert length F, s1[k] faces s2[F - 1 - k] for k in
// [max(0, F - n2), min(n1, F)).  F is admissible iff that range holds at least
// min_overlap positions and at most max_mismatches of them are not an A C G T
// facing its complement.  The result is the greatest admissible F, 0 if none,
// -1 for a pair with a mate longer than HPGQ_OVL_MAX_LEN.
#include <cstdint>

#include "../../include/hpgq.h"

namespace {

// the byte that faces b in a match, 0 if b is no base (no byte matches 0: 0 is no base)
inline unsigned char comp(unsigned char b) {
  switch (b) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    default: return 0;
  }
}

}  // namespace

extern "C" int64_t hpgq_ovl_find(const void *s1, size_t n1, const void *s2, size_t n2, int min_overlap, int max_mismatches) {
  if (min_overlap < 8 || min_overlap > HPGQ_OVL_MAX_LEN || max_mismatches < 0 || max_mismatches > 255 ||
      max_mismatches >= min_overlap || (!s1 && n1) || (!s2 && n2))
    return -2;
  if (n1 > HPGQ_OVL_MAX_LEN || n2 > HPGQ_OVL_MAX_LEN) return -1;
  const unsigned char *a = static_cast<const unsigned char *>(s1), *b = static_cast<const unsigned char *>(s2);
  const int64_t N1 = (int64_t)n1, N2 = (int64_t)n2;
  for (int64_t F = N1 + N2 - min_overlap; F >= min_overlap; --F) {
    const int64_t lo = F > N2 ? F - N2 : 0, hi = N1 < F ? N1 : F;
    if (hi - lo < min_overlap) continue;
    int mism = 0;
    for (int64_t k = lo; k < hi && mism <= max_mismatches; ++k) {
      const unsigned char c = comp(a[k]);
      mism += !(c && b[F - 1 - k] == c);
    }
    if (mism <= max_mismatches) return F;
  }
  return 0;
}

// §2.14: at the facing positions of insert length F that do not match, the
// base of high quality over the one of low quality, quality byte with it.
extern "C" int64_t hpgq_ovl_correct(void *s1, void *q1, size_t n1, void *s2, void *q2, size_t n2, int64_t F, int phred,
                                    int high, int low, uint32_t changed[2]) {
  if (phred < 0 || phred > 255 || low < 0 || low >= high || high > 93 || ((!s1 || !q1) && n1) || ((!s2 || !q2) && n2))
    return -2;
  if (changed) changed[0] = changed[1] = 0;
  if (F <= 0) return 0;
  if (n1 > HPGQ_OVL_MAX_LEN || n2 > HPGQ_OVL_MAX_LEN) return -2;
  const int64_t N1 = (int64_t)n1, N2 = (int64_t)n2;
  const int64_t lo = F > N2 ? F - N2 : 0, hi = N1 < F ? N1 : F;
  if (hi - lo < 8) return -2;   // (no min_overlap admits this F)
  unsigned char *a = static_cast<unsigned char *>(s1), *b = static_cast<unsigned char *>(s2);
  unsigned char *qa = static_cast<unsigned char *>(q1), *qb = static_cast<unsigned char *>(q2);
  uint32_t done[2] = {0, 0};
  for (int64_t k = lo; k < hi; ++k) {
    const int64_t j = F - 1 - k;
    const unsigned char ca = comp(a[k]), cb = comp(b[j]);
    if (ca && b[j] == ca) continue;
    const int v1 = (int)qa[k] - phred, v2 = (int)qb[j] - phred;
    if (ca && v1 >= high && v2 <= low) {
      b[j] = ca;
      qb[j] = qa[k];
      ++done[1];
    } else if (cb && v2 >= high && v1 <= low) {
      a[k] = cb;
      qa[k] = qb[j];
      ++done[0];
    }
  }
  if (changed) {
    changed[0] = done[0];
    changed[1] = done[1];
  }
  return (int64_t)done[0] + done[1];
}

// §2.15: the pair as one read of F bases.  Mate 1 before the facing positions,
// the reverse complement of mate 2 behind them; at a facing position that does
// not match, the base of strictly higher quality byte, mate 1's on a tie.
extern "C" int64_t hpgq_ovl_merge(const void *s1, const void *q1, size_t n1, const void *s2, const void *q2, size_t n2,
                                  int64_t F, void *seq_out, void *qual_out, uint32_t resolved[2]) {
  if (((!s1 || !q1) && n1) || ((!s2 || !q2) && n2)) return -2;
  if (resolved) resolved[0] = resolved[1] = 0;
  if (F <= 0) return 0;
  if (n1 > HPGQ_OVL_MAX_LEN || n2 > HPGQ_OVL_MAX_LEN) return -2;
  const int64_t N1 = (int64_t)n1, N2 = (int64_t)n2;
  const int64_t lo = F > N2 ? F - N2 : 0, hi = N1 < F ? N1 : F;
  if (hi - lo < 8 || !seq_out || !qual_out) return -2;   // (no min_overlap admits this F)
  const unsigned char *a = static_cast<const unsigned char *>(s1), *b = static_cast<const unsigned char *>(s2);
  const unsigned char *qa = static_cast<const unsigned char *>(q1), *qb = static_cast<const unsigned char *>(q2);
  unsigned char *m = static_cast<unsigned char *>(seq_out), *qm = static_cast<unsigned char *>(qual_out);
  uint32_t done[2] = {0, 0};
  for (int64_t p = 0; p < F; ++p) {
    const int64_t j = F - 1 - p;
    if (p < lo) {
      m[p] = a[p];
      qm[p] = qa[p];
    } else if (p >= hi) {
      const unsigned char c = comp(b[j]);
      m[p] = c ? c : b[j];
      qm[p] = qb[j];
    } else {
      const unsigned char ca = comp(a[p]), cb = comp(b[j]);
      if (ca && b[j] == ca) {
        m[p] = a[p];
        qm[p] = qa[p] > qb[j] ? qa[p] : qb[j];
      } else if (cb && (!ca || qb[j] > qa[p])) {
        m[p] = cb;
        qm[p] = qb[j];
        ++done[1];
      } else {
        m[p] = a[p];
        qm[p] = qa[p];
        ++done[0];
      }
    }
  }
  if (resolved) {
    resolved[0] = done[0];
    resolved[1] = done[1];
  }
  return F;
}
