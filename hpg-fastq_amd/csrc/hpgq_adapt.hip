// hpgq_adapt.hip — `stats --adapters`: per probe the counted reads whose first
// occurrence of the probe starts at each read position, first[p][a] u64 on the
// device.  Build-defined: the reference has nothing
// like it.
//
// One kernel.  It reads the sequence bytes, the offsets and the mask and
// nothing else (L + 4 + 1 bytes per read).  Read-major: a wave takes kR = 16
// consecutive reads per step (one coalesced load of their 17 offsets and 16
// mask bytes: hpgq_reads.h) and scans them one after the other, four
// reads' first loads in flight, because "first occurrence" is a property of
// the whole read: the found-mask of a read (one bit per probe, wave-uniform)
// lives across the steps of a long read.
//
// The step -- the lane's four bases as 2-bit codes and validity bits, the
// windows across lanes (H = 3 lanes behind its own for NARROW, the default set;
// H = 8 for WIDE, a probe of more than 13 bases), the workgroup's bitmap of the
// set's 8-base prefixes that ends almost every step of real data after one
// ballot -- is hpgq_probes.h's, shared with hpgq_clip.hip.  A step covers
// S = 4 (64 - H) = 244 or 224 starts: 150 and 250 bp reads with the default set
// take one.  (DESIGN.md 4.13 has the times with and without the bitmap:
// without it the default set took 1.6 - 2 x as long on reads without adapters,
// 32 probes 2.7 - 5 x.)
//
// A step with a candidate walks the probes: one masked compare per start
// ((window & mask_a) == code_a, and the valid run from the start >= K_a, one
// v_ffbl of the inverted validity bits), then one ballot per probe; the lowest
// lane and its lowest start are the first occurrence.  The probes' codes and
// lengths sit in lanes 0 .. 31 of three VGPRs (v_readlane, no scalar load in
// the loop).  A probe once found is skipped for the rest of the read, and a
// read with every probe found ends early.
//
// Counts: first occurrences below kP = 256 go to an LDS table [nprobes][256]
// u32 (1 KB per probe, dynamic LDS; one ds_add by one lane per read and probe
// found), flushed once per workgroup with no-return u64 atomics on the nonzero
// cells; later positions go to global no-return u64 atomics directly.  reads,
// with_any, the longest counted read and the counted reads longer than the
// rows take one add per workgroup.  A counted read longer than the rows is not
// scanned.
#include "hpgq_accum.h"
#include "hpgq_probes.h"
#include "hpgq_reads.h"

#include <algorithm>
#include <vector>

namespace hpgq {
namespace adapt {

constexpr int kP = 256;     // positions whose counts stay on chip
constexpr int kWG = 512;
constexpr int kWaves = kWG / 64;
constexpr int kR = 16;      // reads per wave step
constexpr int kPre = 4;     // of them with their first load in flight
constexpr int kGroup = kWaves * kR;   // reads per workgroup step
using probes::kBitmapWords;
using probes::kMaxProbes;
using probes::Probes;
using reads::v2u;

// One counted read of len <= rows bytes at st0 (from the descriptor's base);
// w0: its first step's load; lp: lane a's probe a.  Everything but the lane's
// bytes is wave-uniform.
template <bool WIDE>
__device__ __forceinline__ uint32_t scan_read(const __amdgpu_buffer_rsrc_t rq, const Probes &pr, int lane, uint32_t st0,
                                              int len, v2u w0, const probes::LaneProbe lp, uint32_t *t,
                                              const uint32_t *bm, unsigned long long *first) {
  constexpr int H = WIDE ? 8 : 3;          // lanes after its own a lane's windows reach into
  constexpr int S = 4 * (64 - H);          // starts per step
  const uint32_t all = pr.n == kMaxProbes ? 0xFFFFFFFFu : (1u << pr.n) - 1u;
  uint32_t found = 0;
  for (int p0 = 0; p0 + pr.kmin <= len; p0 += S) {
    const int rem = len - p0;
    const uint32_t st = st0 + (uint32_t)p0;
    const v2u w = p0 == 0 ? w0 : reads::lane_load8(rq, st, rem, lane);
    // positions p0 + 4 lane + [0, 4): 16 bases from lanes l .. l + 3 (codes 32 bits, validity 16) and the prefilter
    const probes::Window s = probes::window(w, st, rem, lane, bm);
    uint64_t win[4];    // the bases from start k on (WIDE: 32 of them, else 16 - k)
    uint32_t val[4];    // their validity bits (WIDE: 32, else 16 - k)
    if (WIDE) {
      const probes::Wide x = probes::pull_wide(s, lane);
      const uint64_t c8 = (uint64_t)s.c4 | (uint64_t)x.c8_hi << 32;
      const uint32_t ok8 = s.ok4 | x.ok8_hi << 16;
      const uint64_t c9 = x.y9 & 0xFFu;
      const uint32_t ok9 = x.y9 >> 8 & 0xFu;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        win[k] = k ? c8 >> (2 * k) | c9 << (64 - 2 * k) : c8;
        val[k] = k ? ok8 >> k | ok9 << (32 - k) : ok8;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        win[k] = s.c4 >> (2 * k);
        val[k] = s.ok4 >> k;
      }
    }
    const bool starts = lane < 64 - H;   // the last H lanes only supply bases
    if (!__ballot(starts && s.cand != 0)) continue;   // no probe starts in this step: most steps of real data end here
    uint32_t run[4];    // valid bases from start k on, as far as the window goes
#pragma unroll
    for (int k = 0; k < 4; ++k) run[k] = (uint32_t)__builtin_ctzll(~(uint64_t)val[k]);   // (WIDE: 32 when all are valid)
    for (int a = 0; a < pr.n; ++a) {
      if (found >> a & 1u) continue;
      // probe a's length and code from lane a of lp (no scalar load in the loop)
      const uint32_t K = (uint32_t)__builtin_amdgcn_readlane((int)lp.len, a);
      const uint32_t code_lo = (uint32_t)__builtin_amdgcn_readlane((int)lp.lo, a);
      uint32_t m = 0;
      if (WIDE) {
        const uint64_t code = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)lp.hi, a) << 32 | code_lo;
        const uint64_t mask = K == 32 ? ~0ull : (1ull << (2 * K)) - 1ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= ((win[k] & mask) == code && run[k] >= K ? 1u : 0u) << k;
      } else {
        const uint32_t code = code_lo, mask = (1u << (2 * K)) - 1u;
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= (((uint32_t)win[k] & mask) == code && run[k] >= K ? 1u : 0u) << k;
      }
      if (!starts) m = 0;
      const unsigned long long hit = __ballot(m != 0);
      if (!hit) continue;
      const int l0 = __builtin_ctzll(hit);
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_readlane((int)m, l0);
      const int pos = p0 + 4 * l0 + __builtin_ctz(m0);
      found |= 1u << a;
      if (lane == 0) {
        if (pos < kP) atomicAdd(&t[a * kP + pos], 1u);
        else atomicAdd(&first[(size_t)pos * kMaxProbes + a], 1ull);
      }
    }
    if (found == all) break;
  }
  return found;
}

// MASK: mask is not null; WIDE: a probe longer than kNarrowMax (compile-time choices)
template <bool MASK, bool WIDE>
__global__ void __launch_bounds__(kWG) adapt_kernel(const char *seq, const int32_t *idx, int64_t n, const uint8_t *mask,
                                                    int rows, const Probes pr, unsigned long long *first,
                                                    unsigned long long *scal, uint32_t *flags) {
  extern __shared__ uint32_t t[];           // [probe][position], pr.n probes
  __shared__ uint32_t red[4 * kWaves];
  __shared__ uint32_t bm[kBitmapWords];     // bit i: some probe's first 8 bases have the code bits i
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < pr.n * kP; i += kWG) t[i] = 0;
  probes::fill_bitmap<kWG>(bm, pr);   // (its first barrier covers t)
  const reads::Batch rd = reads::open<MASK>(seq, idx, n, mask);
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  const probes::LaneProbe lp = probes::lane_probe(pr, lane);
  // over this wave's counted reads (wave-uniform)
  int longest = 0;
  uint32_t clipped = 0, nreads = 0, nany = 0;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t rb = g * kGroup + wave * kR;
    if (rb >= n) continue;
    int32_t ix;
    uint32_t mk;
    reads::step_reads<kR, MASK>(rd, rb, n, lane, ix, mk);
    auto counted = [&](int i) { return (uint32_t)__builtin_amdgcn_readlane((int)mk, i) == 1u; };
    reads::walk_reads<kR, kPre>(
        rd, ix, lane,
        // scanned: counted, inside the rows, long enough
        [&](int i, int32_t len) { return counted(i) && len <= rows && len >= pr.kmin; },
        [&](int i, int32_t a, int32_t len, v2u w) {
          if (!counted(i)) return;   // (wave-uniform)
          ++nreads;
          longest = max(longest, len);
          clipped += len > rows ? 1u : 0u;   // (a sum, not a branch of its own: the counters stay in registers)
          if (len <= rows && scan_read<WIDE>(rd.bytes, pr, lane, (uint32_t)a + rd.shift, len, w, lp, t, bm, first)) ++nany;
        });
  }
  __syncthreads();
  // flush: consecutive lanes take consecutive positions of one probe (a
  // counted position is below the read's length, so below the rows)
  for (int i = threadIdx.x; i < pr.n * kP; i += kWG) {
    const uint32_t c = t[i];
    if (c) atomicAdd(&first[(size_t)(i % kP) * kMaxProbes + i / kP], (unsigned long long)c);
  }
  if (lane == 0) {
    red[wave] = (uint32_t)longest;
    red[kWaves + wave] = clipped;
    red[2 * kWaves + wave] = nreads;
    red[3 * kWaves + wave] = nany;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t lg = 0, cl = 0, nr = 0, na = 0;
    for (int w2 = 0; w2 < kWaves; ++w2) {
      lg = max(lg, red[w2]);
      cl += red[kWaves + w2];
      nr += red[2 * kWaves + w2];
      na += red[3 * kWaves + w2];
    }
    if (lg) atomicMax(&flags[0], lg);
    if (cl) atomicAdd(&flags[1], cl);
    if (nr) atomicAdd(&scal[0], (unsigned long long)nr);
    if (na) atomicAdd(&scal[1], (unsigned long long)na);
  }
}

}  // namespace adapt
}  // namespace hpgq

// the table: first[rows][32]; the scalars: [reads, with_any]
struct hpgq_adapt : hpgq::accum::Positions {
  hpgq::adapt::Probes pr;
  bool wide = false;
};

namespace {
constexpr size_t kRowBytes = (size_t)HPGQ_ADAPT_MAX_PROBES * 8;
}  // namespace

extern "C" {

int hpgq_adapt_open(hpgq_adapt_t **ad, int device, const char *const *probes, int nprobes, int rows, void *stream) {
  if (!ad) return HPGQ_E_INVALID;
  *ad = nullptr;
  if (!probes || nprobes < 1 || nprobes > HPGQ_ADAPT_MAX_PROBES || rows < 1) return HPGQ_E_INVALID;
  for (int a = 0; a < nprobes; ++a)
    if (hpgq_adapt_find(nullptr, 0, probes[a]) == -2) return HPGQ_E_INVALID;   // the probe rules
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_adapt *q = new hpgq_adapt;
  q->wide = hpgq::probes::encode(q->pr, probes, nprobes);
  if ((rc = q->open(device, stream, rows, kRowBytes, 2)) != HPGQ_OK) {
    hpgq_adapt_close(q);
    return rc;
  }
  *ad = q;
  return HPGQ_OK;
}

void hpgq_adapt_close(hpgq_adapt_t *q) {
  if (!q) return;
  q->close();
  delete q;
}

int hpgq_adapt_reserve_length(hpgq_adapt_t *q, int64_t max_len) {
  return q ? q->reserve_length(max_len) : HPGQ_E_INVALID;
}

int hpgq_adapt_count_device(hpgq_adapt_t *q, const hpgq_batch_t *b, const uint8_t *mask) {
  if (!q || !b || b->num_reads < 0) return HPGQ_E_INVALID;
  if (b->num_reads == 0) return HPGQ_OK;
  if (!b->seq || !b->data_indices) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  using namespace hpgq::adapt;
  return hpgq::accum::for_parts(b, mask, [&](const int32_t *ix, const uint8_t *mk, int64_t n) {
    // as many workgroups per CU as stay resident (four of 512 threads, fewer
    // where the LDS -- 1 KB per probe, the 8 KB bitmap -- admits fewer of the
    // 160 KB)
    const size_t lds = (size_t)q->pr.n * kP * 4 + kBitmapWords * 4 + 512;
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (160 * 1024) / (int64_t)lds));
    const dim3 grid(q->grid(per_cu, (n + kGroup - 1) / kGroup));
    auto *k = mk ? (q->wide ? adapt_kernel<true, true> : adapt_kernel<true, false>)
                 : (q->wide ? adapt_kernel<false, true> : adapt_kernel<false, false>);
    hipLaunchKernelGGL(k, grid, dim3(kWG), (size_t)q->pr.n * kP * 4, q->stream, b->seq, ix, n, mk, (int)q->rows, q->pr,
                       q->d_table, q->d_scal, q->d_flags);
  });
}

int hpgq_adapt_sync(hpgq_adapt_t *q) { return q ? q->settle() : HPGQ_E_INVALID; }

int hpgq_adapt_reset(hpgq_adapt_t *q) { return q ? q->reset() : HPGQ_E_INVALID; }

int hpgq_adapt_read(hpgq_adapt_t *q, uint64_t *first, size_t n, hpgq_adapt_info_t *info) {
  if (!q || (!first && !info)) return HPGQ_E_INVALID;
  int rc = q->settle();
  if (rc) return rc;
  const size_t np = q->h_flags()[0];   // (<= rows: nothing clipped)
  const size_t na = (size_t)q->pr.n;
  if (info) {
    info->reads = q->h_scal[0];
    info->with_any = q->h_scal[1];
    info->nprobes = (int32_t)na;
    info->npos = (int32_t)np;
  }
  if (!first) return HPGQ_OK;
  if (n < na * np) return HPGQ_E_INVALID;
  if (!np) return HPGQ_OK;
  // the device's rows are positions: transposed here into first[a * npos + p]
  std::vector<uint64_t> tmp(np * HPGQ_ADAPT_MAX_PROBES);
  if ((rc = q->read_rows(tmp.data(), np)) != HPGQ_OK) return rc;
  for (size_t a = 0; a < na; ++a)
    for (size_t p = 0; p < np; ++p) first[a * np + p] = tmp[p * HPGQ_ADAPT_MAX_PROBES + a];
  return HPGQ_OK;
}

int hpgq_adapt_debug_set_max_workgroups(hpgq_adapt_t *q, int max_wg) {
  return q ? q->set_max_workgroups(max_wg) : HPGQ_E_INVALID;
}

}  // extern "C"

