// hpgq_ovl.hip — `edit --clip-overlap`: the insert length of a pair from the
// overlap of mate 1 with the reverse complement of mate 2, and both mates cut
// there.  Build-defined: the reference has nothing like
// it.
//
//   ovl_find_kernel    per pair F* (0: none, -1: skipped), the bytes each mate
//                      keeps, and the six scalars.  It reads both mates'
//                      sequence bytes and offsets.
//   scan and copy      hpgq_cut.h, once per mate: the kept reads back to back.
//
// What the handle owns beyond its own state (stream, scalars, replaced buffers,
// grid limits, the scan's storage) is hpgq_cut.h's Cutter, shared with
// hpgq_clip.hip.
//
// Find.  A wave takes kR = 16 pairs, one after the other (the read step of
// hpgq_reads.h on both batches).  A pair with a mate of fewer than min_overlap
// bases has no candidate and costs nothing more.  Otherwise lane l packs the
// bytes 4 l .. 4 l + 3 and 256 + 4 l .. of each mate into 2-bit codes and
// validity bits (pack4) and stores them as bytes of the wave's packed pair in
// LDS: mate 1 forwards, mate 2 complemented and backwards (hpgq_ovl_lane.h), so
// the reversal costs nothing but the byte's address.  Then the candidates go in
// blocks of 64 from the greatest F down, one lane per F: per word of mate 2
// (one address for all lanes: a broadcast) the lane takes the 64 bits of mate 1
// that face it (two ds_read_b64 at most three words apart across the wave, a
// funnel shift), XORs, folds the bit pairs, ANDs the two validity words and
// counts.  One ballot per block: the lowest set lane is the greatest admissible
// F and ends the pair.  No lane ever waits on another wave.
#include "hpgq_accum.h"
#include "hpgq_cut.h"
#include "hpgq_ovl_lane.h"
#include "hpgq_reads.h"

#include <algorithm>

namespace hpgq {
namespace ovl {

constexpr int kWG = 512;
constexpr int kWaves = kWG / 64;
constexpr int kR = 16;                // pairs per wave step
constexpr int kGroup = kWaves * kR;   // pairs per workgroup step
constexpr int kScalars = 6;           // pairs, skipped, overlapping, clipped, bases_removed[2]
using reads::v2u;
static_assert(kMaxLen == HPGQ_OVL_MAX_LEN, "the packed pair holds the longest analysed mate");
static_assert(kMaxLen == 2 * 4 * 64, "two steps of 4 bytes per lane cover a mate");

// the four bases 256 s + 4 lane .. + 3 of a read of len bytes at st0 of its descriptor
__device__ __forceinline__ void lane_pack(const __amdgpu_buffer_rsrc_t rq, uint32_t st0, int len, int s, int lane, uint32_t &c,
                                          uint32_t &ok) {
  const int rem = len - 256 * s;
  const uint32_t st = st0 + 256u * (uint32_t)s;
  uint32_t v = 0;
  if (rem > 0) v = reads::lane_bytes(reads::lane_load8(rq, st, rem, lane), st, rem, lane);   // (wave-uniform)
  reads::pack4(v, c, ok);
}

// One pair, both mates of min_ov .. kMaxLen bytes: F*.  Everything but the
// lane's bytes and its candidate is wave-uniform.
__device__ __forceinline__ int find_pair(const reads::Batch &r1, const reads::Batch &r2, int32_t a1, int n1, int32_t a2, int n2,
                                         uint64_t *pair, int lane, int min_ov, int max_mm) {
  uint8_t *pb = reinterpret_cast<uint8_t *>(pair);
#pragma unroll
  for (int s = 0; s < 2; ++s) {   // (both steps always: the bytes of the pair before are overwritten)
    uint32_t c, ok;
    lane_pack(r1.bytes, (uint32_t)a1 + r1.shift, n1, s, lane, c, ok);
    put_mate1(pb, 64 * s + lane, c, ok);
    lane_pack(r2.bytes, (uint32_t)a2 + r2.shift, n2, s, lane, c, ok);
    put_mate2(pb, 64 * s + lane, c, ok);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();   // other lanes read them (LDS is in order per wave)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  int best = 0;
  for (int fb = n1 + n2 - min_ov; fb >= min_ov; fb -= 64) {
    const Block b = block_of(n1, n2, min_ov, fb);
    const bool mine = fb - lane >= min_ov;
    const int F = mine ? fb - lane : b.fmin;   // (a lane past the last candidate computes the last one again)
    const int ov = ov_of(n1, n2, F);
    const int m = matches_of(pair, F, b.wlo, b.whi);
    const unsigned long long hit = __ballot(mine && ov >= min_ov && ov - m <= max_mm);
    if (hit) {
      best = fb - (int)__builtin_ctzll(hit);
      break;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();   // the next pair's bytes go over these
  return best;
}

__global__ void __launch_bounds__(kWG) ovl_find_kernel(const char *seq1, const int32_t *idx1, const char *seq2,
                                                       const int32_t *idx2, int64_t n, int min_ov, int max_mm,
                                                       int32_t *insert_out, uint32_t *pos1_out, uint32_t *pos2_out,
                                                       unsigned long long *scal) {
  __shared__ uint64_t packed[kWaves][kPairWords];
  __shared__ unsigned long long red[kScalars * kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint64_t *pair = packed[wave];
  for (int i = lane; i < kPairWords; i += 64) pair[i] = 0;   // (the words round mate 1 stay zero)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const reads::Batch r1 = reads::open<false>(seq1, idx1, n, nullptr);
  const reads::Batch r2 = reads::open<false>(seq2, idx2, n, nullptr);
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  // over this wave's pairs (wave-uniform; a launch has at most 2^28 pairs and 2^31 bytes per mate)
  uint32_t cnt[kScalars] = {0, 0, 0, 0, 0, 0};
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t rb = g * kGroup + wave * kR;
    if (rb >= n) continue;
    int32_t ix1, ix2;
    uint32_t mk, mk2;
    reads::step_reads<kR, false>(r1, rb, n, lane, ix1, mk);
    reads::step_reads<kR, false>(r2, rb, n, lane, ix2, mk2);
    // lane i: pair i's results.  A pair that is not cut keeps its lengths.
    int my_f = 0;
    int my_c1 = __builtin_amdgcn_ds_bpermute(((lane + 1) & 63) * 4, ix1) - ix1;
    int my_c2 = __builtin_amdgcn_ds_bpermute(((lane + 1) & 63) * 4, ix2) - ix2;
    for (int i = 0; i < kR; ++i) {
      if ((uint32_t)__builtin_amdgcn_readlane((int)mk, i) != 1u) break;   // past the batch (wave-uniform)
      const int32_t a1 = __builtin_amdgcn_readlane(ix1, i), a2 = __builtin_amdgcn_readlane(ix2, i);
      const int n1 = __builtin_amdgcn_readlane(ix1, i + 1) - a1, n2 = __builtin_amdgcn_readlane(ix2, i + 1) - a2;
      ++cnt[0];
      int f = 0;
      if ((uint32_t)n1 > (uint32_t)kMaxLen || (uint32_t)n2 > (uint32_t)kMaxLen) {
        f = -1;
        ++cnt[1];
      } else if (min(n1, n2) >= min_ov) {   // (a shorter mate: no F has min_ov positions)
        f = find_pair(r1, r2, a1, n1, a2, n2, pair, lane, min_ov, max_mm);
      }
      if (f == 0) continue;
      if (lane == i) my_f = f;
      if (f < 0) continue;
      ++cnt[2];
      const int c1 = min(n1, f), c2 = min(n2, f);
      if (c1 == n1 && c2 == n2) continue;   // the mates overlap, nothing behind the insert
      ++cnt[3];
      cnt[4] += (uint32_t)(n1 - c1);
      cnt[5] += (uint32_t)(n2 - c2);
      if (lane == i) {
        my_c1 = c1;
        my_c2 = c2;
      }
    }
    if (lane < kR && rb + lane < n) {
      if (insert_out) insert_out[rb + lane] = my_f;
      if (pos1_out) pos1_out[rb + lane] = (uint32_t)my_c1;
      if (pos2_out) pos2_out[rb + lane] = (uint32_t)my_c2;
    }
  }
  if (lane == 0)
    for (int k = 0; k < kScalars; ++k) red[k * kWaves + wave] = cnt[k];
  __syncthreads();
  if (threadIdx.x < kScalars) {
    unsigned long long s = 0;
    for (int w2 = 0; w2 < kWaves; ++w2) s += red[threadIdx.x * kWaves + w2];
    if (s) atomicAdd(&scal[threadIdx.x], s);
  }
}

}  // namespace ovl
}  // namespace hpgq

// the scalars: [pairs, skipped, overlapping, clipped, bases_removed[2]]
struct hpgq_ovl : hpgq::cut::Cutter {
  int min_ov = 0, max_mm = 0;
  hpgq::cut::Positions pos[2];              // hpgq_ovl_batch_device's positions, per mate
  hpgq::cut::Kept kept[2];                  // and its outputs
};

namespace {

using namespace hpgq::ovl;
using hpgq::cut::batch_ok;

bool pair_ok(const hpgq_batch_t *m1, const hpgq_batch_t *m2) {
  return batch_ok(m1) && batch_ok(m2) && m1->num_reads == m2->num_reads;
}

// the find pass over the pairs, async; every output may be null
int find(hpgq_ovl *q, const hpgq_batch_t *m1, const hpgq_batch_t *m2, int32_t *ins, uint32_t *pos1, uint32_t *pos2) {
  return hpgq::accum::for_parts(m1, nullptr, [&](const int32_t *ix1, const uint8_t *, int64_t n) {
    const int64_t lo = ix1 - m1->data_indices;
    // four workgroups of 512 threads per CU stay resident (5.5 KB of LDS each)
    const dim3 grid(q->grid(4, (n + kGroup - 1) / kGroup));
    hipLaunchKernelGGL(ovl_find_kernel, grid, dim3(kWG), 0, q->stream, m1->seq, ix1, m2->seq, m2->data_indices + lo, n,
                       q->min_ov, q->max_mm, ins ? ins + lo : nullptr, pos1 ? pos1 + lo : nullptr,
                       pos2 ? pos2 + lo : nullptr, q->d_scal);
  });
}

}  // namespace

extern "C" {

int hpgq_ovl_open(hpgq_ovl_t **ov, int device, int min_overlap, int max_mismatches, void *stream) {
  if (!ov) return HPGQ_E_INVALID;
  *ov = nullptr;
  if (hpgq_ovl_find(nullptr, 0, nullptr, 0, min_overlap, max_mismatches) == -2) return HPGQ_E_INVALID;   // the rules of §2.13
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_ovl *q = new hpgq_ovl;
  q->min_ov = min_overlap;
  q->max_mm = max_mismatches;
  if ((rc = q->open(device, stream, kScalars)) != HPGQ_OK) {
    hpgq_ovl_close(q);
    return rc;
  }
  *ov = q;
  return HPGQ_OK;
}

void hpgq_ovl_close(hpgq_ovl_t *q) {
  if (!q) return;
  q->close();
  for (int m = 0; m < 2; ++m) {
    q->pos[m].free();
    q->kept[m].free();
  }
  delete q;
}

int hpgq_ovl_find_device(hpgq_ovl_t *q, const hpgq_batch_t *m1, const hpgq_batch_t *m2, int32_t *insert_out,
                         uint32_t *pos1_out, uint32_t *pos2_out) {
  if (!q || !pair_ok(m1, m2)) return HPGQ_E_INVALID;
  if (m1->num_reads == 0) return HPGQ_OK;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  return find(q, m1, m2, insert_out, pos1_out, pos2_out);
}

int hpgq_ovl_batch_device(hpgq_ovl_t *q, const hpgq_batch_t *m1, const hpgq_batch_t *m2, hpgq_batch_t *out1,
                          hpgq_batch_t *out2) {
  if (!q || !pair_ok(m1, m2) || !out1 || !out2 || out1 == out2) return HPGQ_E_INVALID;
  if (m1->num_reads && (!m1->quality || !m2->quality)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  const hpgq_batch_t b[2] = {*m1, *m2};   // (an input and an output may be the same struct)
  hpgq_batch_t *const out[2] = {out1, out2};
  const int64_t n = b[0].num_reads;
  for (int m = 0; m < 2; ++m) {
    int rc = q->kept[m].reserve(*q, b[m]);
    if (rc == HPGQ_OK && n) rc = q->pos[m].need(*q, n);
    if (rc) return rc;
  }
  int rc = n ? find(q, &b[0], &b[1], nullptr, q->pos[0].d, q->pos[1].d) : HPGQ_OK;
  for (int m = 0; m < 2 && rc == HPGQ_OK; ++m)
    rc = hpgq::cut::scan_and_copy(*q, &b[m], q->pos[m].d, q->kept[m].o_seq, q->kept[m].o_qual, q->kept[m].o_idx);
  if (rc) return rc;
  for (int m = 0; m < 2; ++m) q->kept[m].give(out[m], n);
  return HPGQ_OK;
}

int hpgq_ovl_sync(hpgq_ovl_t *q) { return q ? q->settle() : HPGQ_E_INVALID; }

int hpgq_ovl_reset(hpgq_ovl_t *q) { return q ? q->reset() : HPGQ_E_INVALID; }

int hpgq_ovl_read(hpgq_ovl_t *q, hpgq_ovl_info_t *info) {
  if (!q || !info) return HPGQ_E_INVALID;
  const int rc = q->settle();
  if (rc) return rc;
  info->pairs = q->h_scal[0];
  info->skipped = q->h_scal[1];
  info->overlapping = q->h_scal[2];
  info->clipped = q->h_scal[3];
  info->bases_removed[0] = q->h_scal[4];
  info->bases_removed[1] = q->h_scal[5];
  info->min_overlap = q->min_ov;
  info->max_mismatches = q->max_mm;
  return HPGQ_OK;
}

int hpgq_ovl_debug_set_max_workgroups(hpgq_ovl_t *q, int max_wg) {
  return q ? q->set_max_workgroups(max_wg) : HPGQ_E_INVALID;
}

}  // extern "C"
