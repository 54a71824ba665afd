// hpgq_probes.h — a set of probes on the device, and the step that finds where
// one of them may start (hpgq_adapt.hip, hpgq_clip.hip).
// Internal.  The device side is inlined and wave-uniform but the lane's bytes.
//
// A step: lane l takes the read's bytes p0 + 4l .. p0 + 4l + 3 (lane_load8 and
// lane_bytes of hpgq_reads.h: those past the read's end are zero) and packs
// them into four 2-bit base codes ((b >> 1) & 3: A 0, C 1, T 2, G 3) and four
// validity bits (pack4).  2-bit codes alias (a, N and 250 other values share
// them), so a window matches only if the codes are equal AND its bases are all
// valid.  Bytes past the read's end -- the next read's bases, the slack -- are
// invalid, so no window reaches over it.
//
// Windows cross lanes.  Each lane builds the codes and validity bits of the
// bases of lanes l .. l + H by doubling with ds_bpermute (codes and validity
// packed into one word while they fit): H = 3 and two permutes give 16 bases in
// a 32-bit window for probes of up to kNarrowMax bases (window); H = 8 and three
// more give 36 bases in a 64 + 8 bit window for probes of up to 32 (pull_wide).
// The last H lanes of a step only supply bases: a step covers the starts
// p0 .. p0 + S - 1, S = 4 (64 - H), and the next step starts at p0 + S.
//
// Prefilter: every probe has at least kPrefix = 8 bases, so the workgroup keeps
// a 65,536 bit map of the set's 8-base prefixes (16 code bits) in LDS
// (fill_bitmap); a start is a candidate iff its next 8 bases are valid and their
// bit is set: one ds_read and a few VALU per start.  The lane's own 16 bases
// decide that, whatever the probes' lengths.  Almost every step of real data
// ends there.
#pragma once
#include "hpgq_reads.h"

#include <algorithm>
#include <cstring>

namespace hpgq {
namespace probes {

constexpr int kMaxProbes = HPGQ_ADAPT_MAX_PROBES;
constexpr int kNarrowMax = 13;        // longest probe of the 32-bit window: 16 bases less the 3 a start may skip
constexpr int kPrefix = 8;            // bases of the prefilter
constexpr int kBitmapWords = 65536 / 32;   // one bit per 8-base prefix (16 code bits)
using reads::v2u;
static_assert(kMaxProbes == 32, "a probe per lane of half a wave, a found-mask of one 32-bit word");
static_assert(kPrefix == HPGQ_ADAPT_MIN_LEN, "every probe has the prefilter's bases");

// the probe set as a kernel takes it (by value: scalar loads)
struct Probes {
  uint64_t code[kMaxProbes];   // base j at bits 2j .. 2j + 1
  uint32_t len[kMaxProbes];
  int32_t n, kmin;
};

// the 2-bit code of an A C G T byte
__host__ __device__ inline uint32_t code_of(uint32_t b) { return (b >> 1) & 3u; }

// The set from n strings that passed the probe rules (hpgq_adapt_find == -2
// names the ones that do not).  -> a probe is longer than kNarrowMax.
inline bool encode(Probes &pr, const char *const *probes, int n) {
  std::memset(&pr, 0, sizeof(pr));
  pr.n = n;
  pr.kmin = HPGQ_ADAPT_MAX_LEN;
  int kmax = 0;
  for (int a = 0; a < n; ++a) {
    const int k = (int)std::strlen(probes[a]);
    for (int j = 0; j < k; ++j) pr.code[a] |= (uint64_t)code_of((unsigned char)probes[a][j]) << (2 * j);
    pr.len[a] = (uint32_t)k;
    pr.kmin = std::min(pr.kmin, k);
    kmax = std::max(kmax, k);
  }
  return kmax > kNarrowMax;
}

__device__ __forceinline__ uint32_t pull(uint32_t v, int lane, int d) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(((lane + d) & 63) * 4, (int)v);
}

// bm[kBitmapWords] in LDS, by a workgroup of WG threads: bit i is set iff some
// probe's first 8 bases have the code bits i.  Two barriers; whatever LDS the
// kernel zeroed before the call is zero for every thread after it.
template <int WG>
__device__ __forceinline__ void fill_bitmap(uint32_t *bm, const Probes &pr) {
  for (int i = threadIdx.x; i < kBitmapWords; i += WG) bm[i] = 0;
  __syncthreads();
  if ((int)threadIdx.x < pr.n) {
    const uint32_t ix8 = (uint32_t)pr.code[threadIdx.x] & 0xFFFFu;
    atomicOr(&bm[ix8 >> 5], 1u << (ix8 & 31u));
  }
  __syncthreads();
}

// Lane a holds probe a: its code's halves and its length (v_readlane, or a
// compare in lane a: no scalar load in the loops).
struct LaneProbe {
  uint32_t lo, hi, len;
};
__device__ __forceinline__ LaneProbe lane_probe(const Probes &pr, int lane) {
  const int pa = lane < pr.n ? lane : 0;
  return LaneProbe{(uint32_t)pr.code[pa], (uint32_t)(pr.code[pa] >> 32), pr.len[pa]};
}

// A lane's view of a step: the 16 bases from its first on, and which of its
// four starts are candidates.
struct Window {
  uint32_t c4, ok4;   // codes (base j at bits 2j .. 2j + 1) and validity (bit j) of the bases of lanes l .. l + 3
  uint32_t x1;        // the lane's own four: codes | validity << 8
  uint32_t cand;      // bit k: start k passes the prefilter
};

// w: the step's load (lane_load8) at st of the descriptor, rem bytes of the read from there on
__device__ __forceinline__ Window window(v2u w, uint32_t st, int rem, int lane, const uint32_t *bm) {
  Window s;
  uint32_t c, ok;
  reads::pack4(reads::lane_bytes(w, st, rem, lane), c, ok);
  s.x1 = c | ok << 8;
  const uint32_t y1 = pull(s.x1, lane, 1);
  const uint32_t c2 = c | (y1 & 0xFFu) << 8, ok2 = ok | (y1 >> 8 & 0xFu) << 4;
  const uint32_t y2 = pull(c2 | ok2 << 16, lane, 2);
  s.c4 = c2 | y2 << 16;
  s.ok4 = ok2 | (y2 >> 16 & 0xFFu) << 8;
  // r8 bit k: the 8 bases from start k on are valid (ok4 folded three times)
  const uint32_t r2 = s.ok4 & s.ok4 >> 1, r4 = r2 & r2 >> 2, r8 = r4 & r4 >> 4;
  s.cand = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t ix8 = s.c4 >> (2 * k) & 0xFFFFu;
    s.cand |= (bm[ix8 >> 5] >> (ix8 & 31u) & r8 >> k & 1u) << k;
  }
  return s;
}

// The wide case: the bases of lanes l + 4 .. l + 8 behind the window's 16.
struct Wide {
  uint32_t c8_hi, ok8_hi;   // lanes l + 4 .. l + 7: 16 codes, 16 validity bits
  uint32_t y9;              // lane l + 8: codes | validity << 8
};
__device__ __forceinline__ Wide pull_wide(const Window &s, int lane) {
  return Wide{pull(s.c4, lane, 4), pull(s.ok4, lane, 4), pull(s.x1, lane, 8)};
}

}  // namespace probes
}  // namespace hpgq
