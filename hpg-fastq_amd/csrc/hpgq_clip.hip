// hpgq_clip.hip — `edit --clip-adapters`: cut every read at the lowest position
// at which a probe matches, whole or running off the read's end (DESIGN.md
// §2.12, §4.15).  Build-defined: the reference has nothing like it.
//
// Three launches on the handle's stream, none of which waits on another
// workgroup:
//
//   clip_find_kernel   per read the clip position c, the winning probe, and the
//                      four scalars.  It reads the sequence bytes and the
//                      offsets (L + 4 bytes per read).
//   hipcub inclusive sum of the c into idx_out[1 .. n], idx_out[0] = 0
//   clip_copy_kernel   sequence and quality [idx[i], idx[i] + c_i) to
//                      [idx_out[i], idx_out[i + 1]).
//
// Find.  A wave takes kR = 16 reads, one after the other (hpgq_reads.h); the
// step -- codes and validity bits, the windows across lanes, the bitmap of the
// set's 8-base prefixes that ends most steps after one ballot -- is
// hpgq_probes.h's, shared with hpgq_adapt.hip.  What differs from adapt:
//   * a read ends at its first hit.  A step with candidates walks them, lowest
//     start first: the start's window goes to every lane (v_readlane), lane a
//     compares probe a (the probe parameters already sit in lanes 0 .. 31), and
//     one ballot gives the lowest probe that matches there.  No found-mask lives
//     across steps, there is no table, and a probe longer than 13 bases costs
//     its three extra ds_bpermute only in a step that has a candidate.
//   * a probe also matches where the read ends inside it.  With m = min(K, n - j)
//     bases compared, the start passes the prefilter whenever m >= 8 (the bytes
//     past the read's end are zeroed, so invalid: the valid run from j ends at
//     the read's end), and the compare is under the mask of m bases.
//   * matches of fewer than 8 bases (min_overlap < 8 only) start in the read's
//     last 7 positions, behind every start the steps can hit.  A read without a
//     hit gets one more load of its last 7 bytes; lane a compares probe a, one
//     ballot per start.
//
// Scan and copy, and what the handle owns beyond its own state: hpgq_cut.h,
// shared with hpgq_ovl.hip.
#include "hpgq_accum.h"
#include "hpgq_cut.h"
#include "hpgq_probes.h"
#include "hpgq_reads.h"

#include <algorithm>

namespace hpgq {
namespace clip {

constexpr int kWG = 512;
constexpr int kWaves = kWG / 64;
constexpr int kR = 16;      // reads per wave step
constexpr int kPre = 4;     // of them with their first load in flight
constexpr int kGroup = kWaves * kR;   // reads per workgroup step
using probes::kBitmapWords;
using probes::kMaxProbes;
using probes::kPrefix;
using probes::Probes;
using reads::v2u;
constexpr int kScalars = 3 + kMaxProbes;   // reads, clipped, bases_removed, by_probe[32]

// One read of len bytes at st0 (from the descriptor's base); w0: its first
// step's load; lp: lane a's probe a.  Everything but the lane's bytes is
// wave-uniform.  -> c, and the winning probe in `who` (0xFF: none).
template <bool WIDE>
__device__ __forceinline__ int find_read(const __amdgpu_buffer_rsrc_t rq, const Probes &pr, int min_ov, int lane,
                                         uint32_t st0, int len, v2u w0, const probes::LaneProbe lp, const uint32_t *bm,
                                         uint32_t &who) {
  constexpr int H = WIDE ? 8 : 3;          // lanes after its own a lane's windows reach into
  constexpr int S = 4 * (64 - H);          // starts per step
  // the fewest bases a match of the steps compares: a whole probe, or an overlap that passes the prefilter
  const int least = min(pr.kmin, max(min_ov, kPrefix));
  for (int p0 = 0; p0 + least <= len; p0 += S) {
    const int rem = len - p0;
    const uint32_t st = st0 + (uint32_t)p0;
    const v2u w = p0 == 0 ? w0 : reads::lane_load8(rq, st, rem, lane);
    // 16 bases from lanes l .. l + 3 and the prefilter: a match of the steps
    // compares at least 8 bases, so it starts at a candidate
    const probes::Window s = probes::window(w, st, rem, lane, bm);
    const bool starts = lane < 64 - H;   // the last H lanes only supply bases
    unsigned long long lanes = __ballot(starts && s.cand != 0);
    if (!lanes) continue;   // nothing starts in this step
    // WIDE: the bases of lanes l + 4 .. l + 8 behind the lane's 16 (only a step with a candidate needs them)
    probes::Wide x{0, 0, 0};
    if (WIDE) x = probes::pull_wide(s, lane);
    // The candidates, lowest first: the window of one start goes to every lane,
    // lane a compares probe a, and one ballot gives the lowest probe that matches
    // there.  The first start with a match is c.
    do {
      const int l0 = __builtin_ctzll(lanes);
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)s.c4, l0);
      const uint32_t vlo = (uint32_t)__builtin_amdgcn_readlane((int)s.ok4, l0);
      uint64_t base = lo;          // the bases from the lane's first on, 2 bits each (WIDE: 32 and 4 more in over)
      uint32_t valid = vlo, over = 0, vover = 0;
      if (WIDE) {
        base |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)x.c8_hi, l0) << 32;
        valid |= (uint32_t)__builtin_amdgcn_readlane((int)x.ok8_hi, l0) << 16;
        const uint32_t y = (uint32_t)__builtin_amdgcn_readlane((int)x.y9, l0);
        over = y & 0xFFu;
        vover = y >> 8 & 0xFu;
      }
      for (uint32_t ks = (uint32_t)__builtin_amdgcn_readlane((int)s.cand, l0); ks; ks &= ks - 1u) {
        const int k0 = __builtin_ctz(ks);
        const uint64_t win = WIDE && k0 ? base >> (2 * k0) | (uint64_t)over << (64 - 2 * k0) : base >> (2 * k0);
        const uint32_t val = WIDE && k0 ? valid >> k0 | vover << (32 - k0) : valid >> k0;
        // the valid bases from the start on, as far as the window goes, and the
        // read's bases from it on (bytes past the read's end are invalid: run <= left)
        const uint32_t run = (uint32_t)__builtin_ctzll(~(uint64_t)val);
        const uint32_t left = (uint32_t)min(rem - 4 * l0 - k0, 32);
        // lane a: probe a's whole length, or what the read has left of it (8 or more: the start is a candidate)
        const uint32_t cmp = min(lp.len, left);
        bool eq;
        if (WIDE) {
          const uint64_t mask = cmp >= 32u ? ~0ull : (1ull << (2 * cmp)) - 1ull;
          eq = ((win ^ ((uint64_t)lp.hi << 32 | lp.lo)) & mask) == 0;
        } else {
          eq = (((uint32_t)win ^ lp.lo) & ((1u << (2 * cmp)) - 1u)) == 0;
        }
        const unsigned long long hit =
            __ballot(lane < pr.n && eq && run >= cmp && (cmp == lp.len || cmp >= (uint32_t)min_ov));
        if (hit) {
          who = (uint32_t)__builtin_ctzll(hit);
          return p0 + 4 * l0 + k0;
        }
      }
      lanes &= lanes - 1ull;
    } while (lanes);
  }
  // Overlaps of fewer than 8 bases: the read's last tn <= 7 bytes, all of which
  // lie behind every start the steps above can hit.  Lane a holds probe a.
  if (min_ov < kPrefix && len >= min_ov) {
    const int ts = max(len - (kPrefix - 1), 0), tn = len - ts;
    const uint32_t st = st0 + (uint32_t)ts;
    uint32_t c, ok;
    reads::pack4(reads::lane_bytes(reads::lane_load8(rq, st, tn, lane), st, tn, lane), c, ok);
    const uint32_t tc = (uint32_t)__builtin_amdgcn_readlane((int)c, 0) | (uint32_t)__builtin_amdgcn_readlane((int)c, 1) << 8;
    const uint32_t tok = (uint32_t)__builtin_amdgcn_readlane((int)ok, 0) | (uint32_t)__builtin_amdgcn_readlane((int)ok, 1) << 4;
    for (int d = 0; tn - d >= min_ov; ++d) {
      const int m = tn - d;   // 1 .. 7 bases, fewer than any probe has
      const uint32_t vm = (1u << m) - 1u, cm = (1u << (2 * m)) - 1u;
      const bool eq = lane < pr.n && (tok >> d & vm) == vm && ((tc >> (2 * d) ^ lp.lo) & cm) == 0;
      const unsigned long long hit = __ballot(eq);
      if (hit) {
        who = (uint32_t)__builtin_ctzll(hit);
        return ts + d;
      }
    }
  }
  who = 0xFFu;
  return len;
}

// WIDE: a probe longer than kNarrowMax (a compile-time choice)
template <bool WIDE>
__global__ void __launch_bounds__(kWG) clip_find_kernel(const char *seq, const int32_t *idx, int64_t n, const Probes pr,
                                                        int min_ov, uint32_t *pos_out, uint8_t *probe_out,
                                                        unsigned long long *scal) {
  __shared__ uint32_t bm[kBitmapWords];     // bit i: some probe's first 8 bases have the code bits i
  __shared__ uint32_t won[kMaxProbes];      // reads won per probe
  __shared__ unsigned long long red[3 * kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kMaxProbes) won[threadIdx.x] = 0;
  probes::fill_bitmap<kWG>(bm, pr);   // (its first barrier covers won)
  const reads::Batch rd = reads::open<false>(seq, idx, n, nullptr);
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  const probes::LaneProbe lp = probes::lane_probe(pr, lane);
  const int shortest = min(pr.kmin, min_ov);   // a shorter read has no match
  // over this wave's reads (wave-uniform; a launch has at most 2^28 reads and 2^31 bytes)
  uint32_t nreads = 0, nclipped = 0, removed = 0;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t rb = g * kGroup + wave * kR;
    if (rb >= n) continue;
    int32_t ix;
    uint32_t mk;
    reads::step_reads<kR, false>(rd, rb, n, lane, ix, mk);
    nreads += (uint32_t)(n - rb < kR ? n - rb : kR);
    // lane i: read i's result.  A read without a hit keeps its length and no
    // winner, so only a hit costs the wave anything here.
    int my_c = (int)probes::pull((uint32_t)ix, lane, 1) - ix, my_who = 0xFF;
    auto on = [&](int i) { return (uint32_t)__builtin_amdgcn_readlane((int)mk, i) == 1u; };
    reads::walk_reads<kR, kPre>(
        rd, ix, lane, [&](int i, int32_t len) { return on(i) && len >= shortest; },
        [&](int i, int32_t a, int32_t len, v2u w) {
          if (!on(i)) return;   // past the batch (wave-uniform)
          uint32_t who = 0xFFu;
          int c = len;
          if (len >= shortest) c = find_read<WIDE>(rd.bytes, pr, min_ov, lane, (uint32_t)a + rd.shift, len, w, lp, bm, who);
          if (c < len) {
            ++nclipped;
            removed += (uint32_t)(len - c);
            if (lane == 0) atomicAdd(&won[who], 1u);
            if (lane == i) {
              my_c = c;
              my_who = (int)who;
            }
          }
        });
    if (lane < kR && rb + lane < n) {
      pos_out[rb + lane] = (uint32_t)my_c;
      if (probe_out) probe_out[rb + lane] = (uint8_t)my_who;
    }
  }
  if (lane == 0) {
    red[wave] = nreads;
    red[kWaves + wave] = nclipped;
    red[2 * kWaves + wave] = removed;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long s = 0;
    for (int w2 = 0; w2 < kWaves; ++w2) s += red[threadIdx.x * kWaves + w2];
    if (s) atomicAdd(&scal[threadIdx.x], s);
  } else if (threadIdx.x >= 64 && (int)threadIdx.x < 64 + pr.n) {
    const uint32_t s = won[threadIdx.x - 64];
    if (s) atomicAdd(&scal[3 + threadIdx.x - 64], (unsigned long long)s);
  }
}

}  // namespace clip
}  // namespace hpgq

// the scalars: [reads, clipped, bases_removed, by_probe[32]]
struct hpgq_clip : hpgq::cut::Cutter {
  hpgq::probes::Probes pr;
  bool wide = false;
  int min_ov = 0;
  hpgq::cut::Positions pos;                 // positions when the caller wants none
  hpgq::cut::Kept kept;                     // hpgq_clip_batch_device's outputs
};

namespace {

using namespace hpgq::clip;
using hpgq::cut::batch_ok;

// the find pass over b, async: positions to pos (never null), probes to probe (may be null)
int find(hpgq_clip *q, const hpgq_batch_t *b, uint32_t *pos, uint8_t *probe) {
  return hpgq::accum::for_parts(b, nullptr, [&](const int32_t *ix, const uint8_t *, int64_t n) {
    const int64_t lo = ix - b->data_indices;
    // four workgroups of 512 threads per CU stay resident (8.6 KB of LDS each)
    const dim3 grid(q->grid(4, (n + kGroup - 1) / kGroup));
    auto *k = q->wide ? clip_find_kernel<true> : clip_find_kernel<false>;
    hipLaunchKernelGGL(k, grid, dim3(kWG), 0, q->stream, b->seq, ix, n, q->pr, q->min_ov, pos + lo,
                       probe ? probe + lo : nullptr, q->d_scal);
  });
}

}  // namespace

extern "C" {

int hpgq_clip_open(hpgq_clip_t **cl, int device, const char *const *probes, int nprobes, int min_overlap, void *stream) {
  if (!cl) return HPGQ_E_INVALID;
  *cl = nullptr;
  if (hpgq_clip_find(nullptr, 0, probes, nprobes, min_overlap, nullptr) == -2) return HPGQ_E_INVALID;   // the rules of §2.12
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_clip *q = new hpgq_clip;
  q->wide = hpgq::probes::encode(q->pr, probes, nprobes);
  q->min_ov = min_overlap;
  if ((rc = q->open(device, stream, kScalars)) != HPGQ_OK) {
    hpgq_clip_close(q);
    return rc;
  }
  *cl = q;
  return HPGQ_OK;
}

void hpgq_clip_close(hpgq_clip_t *q) {
  if (!q) return;
  q->close();
  q->pos.free();
  q->kept.free();
  delete q;
}

int hpgq_clip_find_device(hpgq_clip_t *q, const hpgq_batch_t *b, uint32_t *pos_out, uint8_t *probe_out) {
  if (!q || !batch_ok(b)) return HPGQ_E_INVALID;
  if (b->num_reads == 0) return HPGQ_OK;
  if (!pos_out) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  return find(q, b, pos_out, probe_out);
}

int hpgq_clip_device(hpgq_clip_t *q, const hpgq_batch_t *b, char *seq_out, char *qual_out, int32_t *idx_out,
                     uint32_t *pos_out, uint8_t *probe_out) {
  if (!q || !batch_ok(b) || !idx_out) return HPGQ_E_INVALID;
  if (b->num_reads && (!b->quality || !seq_out || !qual_out)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  if (!pos_out && b->num_reads) {
    const int rc = q->pos.need(*q, b->num_reads);
    if (rc) return rc;
    pos_out = q->pos.d;
  }
  const int rc = b->num_reads ? find(q, b, pos_out, probe_out) : HPGQ_OK;
  return rc ? rc : hpgq::cut::scan_and_copy(*q, b, pos_out, seq_out, qual_out, idx_out);
}

int hpgq_clip_batch_device(hpgq_clip_t *q, const hpgq_batch_t *in, hpgq_batch_t *out) {
  if (!q || !batch_ok(in) || !out || (in->num_reads && !in->quality)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  const hpgq_batch_t b = *in;   // (in and out may be the same struct)
  int rc = q->kept.reserve(*q, b);
  if (rc) return rc;
  rc = hpgq_clip_device(q, &b, q->kept.o_seq, q->kept.o_qual, q->kept.o_idx, nullptr, nullptr);
  if (rc) return rc;
  q->kept.give(out, b.num_reads);
  return HPGQ_OK;
}

int hpgq_clip_sync(hpgq_clip_t *q) { return q ? q->settle() : HPGQ_E_INVALID; }

int hpgq_clip_reset(hpgq_clip_t *q) { return q ? q->reset() : HPGQ_E_INVALID; }

int hpgq_clip_read(hpgq_clip_t *q, hpgq_clip_info_t *info) {
  if (!q || !info) return HPGQ_E_INVALID;
  const int rc = q->settle();
  if (rc) return rc;
  info->reads = q->h_scal[0];
  info->clipped = q->h_scal[1];
  info->bases_removed = q->h_scal[2];
  for (int a = 0; a < kMaxProbes; ++a) info->by_probe[a] = q->h_scal[3 + a];
  info->nprobes = q->pr.n;
  info->min_overlap = q->min_ov;
  return HPGQ_OK;
}

int hpgq_clip_debug_set_max_workgroups(hpgq_clip_t *q, int max_wg) {
  return q ? q->set_max_workgroups(max_wg) : HPGQ_E_INVALID;
}

}  // extern "C"
