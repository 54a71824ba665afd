// hpgq_ovl.hip — `edit --clip-overlap`: the insert length of a pair from the
// overlap of mate 1 with the reverse complement of mate 2, and both mates cut
// there.  Build-defined: the reference has nothing like
// it.
//
//   ovl_find_kernel    per pair F* (0: none, -1: skipped), the bytes each mate
//                      keeps, and the six scalars.  It reads both mates'
//                      sequence bytes and offsets.
//   scan and copy      hpgq_cut.h, once per mate: the kept reads back to back.
//   ovl_fix_kernel     (--correct-overlap, §2.14) the facing bases of the kept
//                      reads that disagree, the better quality's copied over
//                      the worse, in place in the handle's kept buffers.
//   ovl_hist_kernel    (--insert-size, §2.14) the F* of a part into the
//                      handle's histogram.
//   ovl_plan_kernel, ovl_compact_kernel, ovl_merge_kernel
//                      (--merge-overlap, §2.15, §4.18) the pairs with F* > 0 as
//                      one read each in a third kept batch, the others uncut
//                      in the two kept batches, all three compacted.
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
constexpr int kFixScalars = 3;        // behind them: corrected_pairs, corrected_bases[2]
constexpr int kMergeScalars = 4;      // behind those: merged_pairs, merged_bases, resolved[2]
constexpr int kBins = HPGQ_OVL_INSERT_BINS;
static_assert(2 * kMaxLen - 8 < kBins, "every F* has a bin");
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

// the byte that faces b in a match, 0 if b is no base
__device__ __forceinline__ uint32_t comp_of(uint32_t b) {
  return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : 0u;
}

// The four bytes at at .. at + 3 of a descriptor (at >= -3, any alignment) in
// the opposite order: byte t of the result is the byte at at + 3 - t.  The two
// dwords that hold them; the one below offset 0 is not loaded, its bytes are 0.
__device__ __forceinline__ uint32_t load4_backwards(const __amdgpu_buffer_rsrc_t rq, int32_t at, bool need) {
  const int32_t al = at & ~3;   // (two's complement: -3 .. -1 -> -4)
  const uint32_t w0 = __builtin_amdgcn_raw_buffer_load_b32(rq, need && al >= 0 ? (uint32_t)al : reads::kNone, 0, 0);
  const uint32_t w1 = __builtin_amdgcn_raw_buffer_load_b32(rq, need ? (uint32_t)(al + 4) : reads::kNone, 0, 0);
  return __builtin_bswap32(__builtin_amdgcn_alignbyte(w1, w0, (uint32_t)at & 3u));
}

// §2.14's correction on the kept reads of a part, in place.  seq1 .. idx2: the
// handle's kept batches (idx: the part's n + 1 offsets), ins: the part's F*.
// Read-major like the find: a wave takes kR pairs one after the other, a pair
// with F* <= 0 costs nothing more.  With lo = F - c2 and hi = c1 (the kept
// lengths: §2.14), lane l of step s holds k = 256 s + 4 l .. + 3 of mate 1 (one
// dword of sequence, one of quality) and the four bytes of mate 2 that face
// them, j = F - 1 - k down to F - 4 - k: contiguous, backwards.  Positions
// outside [lo, hi) are masked.  A byte is stored only where a rule fires, as a
// byte, by the one lane that holds its position; no dword is ever written.
__global__ void __launch_bounds__(kWG) ovl_fix_kernel(char *seq1, char *qual1, const int32_t *idx1, char *seq2, char *qual2,
                                                      const int32_t *idx2, const int32_t *ins, int64_t n, int phred, int high,
                                                      int low, unsigned long long *scal) {
  __shared__ unsigned long long red[kFixScalars * kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const reads::Batch s1 = reads::open<false>(seq1, idx1, n, nullptr);
  const reads::Batch q1 = reads::open<false>(qual1, idx1, n, nullptr);
  const reads::Batch s2 = reads::open<false>(seq2, idx2, n, nullptr);
  const reads::Batch q2 = reads::open<false>(qual2, idx2, n, nullptr);
  const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc((void *)ins, (short)0, (uint32_t)(n * 4), 0x00020000);
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  uint32_t cnt[kFixScalars] = {0, 0, 0};   // over this wave's pairs (wave-uniform)
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t rb = g * kGroup + wave * kR;
    if (rb >= n) continue;
    int32_t ix1, ix2;
    uint32_t mk, mk2;
    reads::step_reads<kR, false>(s1, rb, n, lane, ix1, mk);
    reads::step_reads<kR, false>(s2, rb, n, lane, ix2, mk2);
    const int32_t fv = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(
        rf, rb + lane < n && lane < kR ? (uint32_t)(rb + lane) * 4u : reads::kNone, 0, 0);
    for (int i = 0; i < kR; ++i) {
      if ((uint32_t)__builtin_amdgcn_readlane((int)mk, i) != 1u) break;   // past the batch (wave-uniform)
      const int F = __builtin_amdgcn_readlane(fv, i);
      if (F <= 0) continue;
      const int32_t a1 = __builtin_amdgcn_readlane(ix1, i), a2 = __builtin_amdgcn_readlane(ix2, i);
      const int c1 = __builtin_amdgcn_readlane(ix1, i + 1) - a1, c2 = __builtin_amdgcn_readlane(ix2, i + 1) - a2;
      const int lo = F - c2, hi = min(c1, kMaxLen);
      if (lo < 0 || hi > F || lo >= hi) continue;   // (not what the find and the cut leave: nothing is touched)
      uint32_t fixed1 = 0, fixed2 = 0;   // the lane's corrected bases of this pair
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int k0 = 256 * s;
        if (k0 >= hi || k0 + 256 <= lo) continue;   // (wave-uniform)
        const int k = k0 + 4 * lane;
        const bool mine = k + 3 >= lo && k < hi;
        const int rem = mine ? hi - k0 : 0;
        const uint32_t st1 = (uint32_t)a1 + s1.shift + (uint32_t)k0, sq1 = (uint32_t)a1 + q1.shift + (uint32_t)k0;
        const uint32_t b1 = reads::lane_bytes(reads::lane_load8(s1.bytes, st1, rem, lane), st1, rem, lane);
        const uint32_t p1 = reads::lane_bytes(reads::lane_load8(q1.bytes, sq1, rem, lane), sq1, rem, lane);
        const int j3 = F - 4 - k;   // the lowest of the four facing positions: -3 at least where the lane is `mine`
        const uint32_t b2 = load4_backwards(s2.bytes, a2 + (int32_t)s2.shift + j3, mine);
        const uint32_t p2 = load4_backwards(q2.bytes, a2 + (int32_t)q2.shift + j3, mine);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int kt = k + t;
          const uint32_t x1 = b1 >> (8 * t) & 255u, x2 = b2 >> (8 * t) & 255u;
          const uint32_t y1 = p1 >> (8 * t) & 255u, y2 = p2 >> (8 * t) & 255u;
          const uint32_t m1 = comp_of(x1), m2 = comp_of(x2);
          const bool open = mine && kt >= lo && kt < hi && !(m1 != 0u && x2 == m1);
          const int v1 = (int)y1 - phred, v2 = (int)y2 - phred;
          const bool to2 = open && m1 != 0u && v1 >= high && v2 <= low;
          const bool to1 = open && !to2 && m2 != 0u && v2 >= high && v1 <= low;
          if (to2) {
            const int64_t at = (int64_t)a2 + (F - 1 - kt);
            reinterpret_cast<uint8_t *>(seq2)[at] = (uint8_t)m1;
            reinterpret_cast<uint8_t *>(qual2)[at] = (uint8_t)y1;
            ++fixed2;
          }
          if (to1) {
            const int64_t at = (int64_t)a1 + kt;
            reinterpret_cast<uint8_t *>(seq1)[at] = (uint8_t)m2;
            reinterpret_cast<uint8_t *>(qual1)[at] = (uint8_t)y2;
            ++fixed1;
          }
        }
      }
      if (__ballot((fixed1 | fixed2) != 0u) == 0ull) continue;
      ++cnt[0];
#pragma unroll
      for (int b = 0; b < 4; ++b) {   // (a lane corrects 0 .. 8 bases per mate)
        cnt[1] += (uint32_t)__popcll(__ballot((fixed1 >> b & 1u) != 0u)) << b;
        cnt[2] += (uint32_t)__popcll(__ballot((fixed2 >> b & 1u) != 0u)) << b;
      }
    }
  }
  if (lane == 0)
    for (int k = 0; k < kFixScalars; ++k) red[k * kWaves + wave] = cnt[k];
  __syncthreads();
  if (threadIdx.x < kFixScalars) {
    unsigned long long s = 0;
    for (int w2 = 0; w2 < kWaves; ++w2) s += red[threadIdx.x * kWaves + w2];
    if (s) atomicAdd(&scal[kScalars + threadIdx.x], s);
  }
}

// hist[F*] += 1 over a part's pairs, -1 (skipped) in no bin: a table per
// workgroup in LDS, then one u64 atomic per cell that counted (a workgroup
// sees at most a part's 2^28 pairs: the u32 cells hold them).
__global__ void __launch_bounds__(kWG) ovl_hist_kernel(const int32_t *ins, int64_t n, unsigned long long *hist) {
  __shared__ uint32_t table[kBins];
  for (int c = threadIdx.x; c < kBins; c += kWG) table[c] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWG) {
    const int32_t f = ins[i];
    if ((uint32_t)f < (uint32_t)kBins) atomicAdd(&table[f], 1u);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < kBins; c += kWG) {
    const uint32_t v = table[c];
    if (v) atomicAdd(&hist[c], (unsigned long long)v);
  }
}

// §2.15's plan of a part: per pair the bytes each mate keeps as an unmerged
// pair (everything, or nothing where the pair merges), the merged read's bytes
// and the merged flag; mlen and flag are then summed in place.
__global__ void __launch_bounds__(256) ovl_plan_kernel(const int32_t *idx1, const int32_t *idx2, const int32_t *ins, int64_t n,
                                                       uint32_t *pos1, uint32_t *pos2, int32_t *mlen, int32_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int32_t f = ins[i];
    const bool merges = f > 0;
    pos1[i] = merges ? 0u : (uint32_t)(idx1[i + 1] - idx1[i]);
    pos2[i] = merges ? 0u : (uint32_t)(idx2[i + 1] - idx2[i]);
    mlen[i] = merges ? f : 0;
    flag[i] = merges ? 1 : 0;
  }
}

// The three uncompacted offset arrays of a part (u1, u2, um: n + 1 offsets, a
// pair that is not in an output has no bytes there) into the three compacted
// data_indices, by rank: rank[i] counts the merged pairs up to and with pair i
// of the whole batch, `first` is the part's first pair.  The part that ends the
// batch (tail) writes the three totals behind the last entries.
__global__ void __launch_bounds__(256) ovl_compact_kernel(const int32_t *u1, const int32_t *u2, const int32_t *um,
                                                          const int32_t *rank, const int32_t *ins, int64_t n, int64_t first,
                                                          int tail, int32_t *c1, int32_t *c2, int32_t *cm) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = rank[i];
    const bool merges = ins[i] > 0;
    if (merges) {
      cm[r - 1] = um[i];
    } else {
      c1[first + i - r] = u1[i];
      c2[first + i - r] = u2[i];
    }
    if (tail && i == n - 1) {
      cm[r] = um[n];
      c1[first + n - r] = u1[n];
      c2[first + n - r] = u2[n];
    }
  }
}

// §2.15's merged reads of a part.  seq1 .. idx2: the inputs (idx: the part's
// n + 1 offsets), ins: the part's F*, moff: the part's uncompacted merged
// offsets (pair i's read at [moff[i], moff[i] + F*) of seq_out / qual_out,
// which hipMalloc aligned).  Read-major like the fix: a wave takes kR pairs one
// after the other, a pair with F* <= 0 costs nothing more.  In a step of 256
// positions lane l holds p = 256 s + 4 l .. + 3: mate 1's dword of sequence and
// of quality where p < hi, the four bytes of mate 2 that face them (backwards)
// where p + 3 >= lo.  §2.15 on those four positions is merge4 (hpgq_ovl_lane.h):
// dword arithmetic without a compare.  The lane's four merged bytes are then moved by the output
// offset's residue (the lane below's dword; lane 0: lane 63's of the step
// before) so that every lane holds one aligned output dword; it is stored as a
// dword where it lies whole inside the read's range and byte by byte where it
// does not: hpgq_cut.h's rule, no dword is read, modified and written.
__global__ void __launch_bounds__(kWG) ovl_merge_kernel(const char *seq1, const char *qual1, const int32_t *idx1,
                                                        const char *seq2, const char *qual2, const int32_t *idx2,
                                                        const int32_t *ins, const int32_t *moff, int64_t n, char *seq_out,
                                                        char *qual_out, unsigned long long *scal) {
  __shared__ unsigned long long red[kMergeScalars];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const reads::Batch s1 = reads::open<false>(seq1, idx1, n, nullptr);
  const reads::Batch q1 = reads::open<false>(qual1, idx1, n, nullptr);
  const reads::Batch s2 = reads::open<false>(seq2, idx2, n, nullptr);
  const reads::Batch q2 = reads::open<false>(qual2, idx2, n, nullptr);
  const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc((void *)ins, (short)0, (uint32_t)(n * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void *)moff, (short)0, (uint32_t)(n * 4), 0x00020000);
  const int nn = (int)n, ngroups = (nn + kGroup - 1) / kGroup;   // (a part: at most 2^28 pairs)
  // over this wave's pairs, in the lanes' own registers: the pairs and their bases the same in every lane
  // (lane 0's count), the resolved bases each lane's own
  uint32_t pairs = 0, won1 = 0, won2 = 0;
  unsigned long long bases = 0;
  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int rb = g * kGroup + wave * kR;
    if (rb >= nn) continue;
    int32_t ix1, ix2;
    uint32_t mk, mk2;
    reads::step_reads<kR, false>(s1, rb, n, lane, ix1, mk);
    reads::step_reads<kR, false>(s2, rb, n, lane, ix2, mk2);
    const uint32_t mine_at = rb + lane < nn && lane < kR ? (uint32_t)(rb + lane) * 4u : reads::kNone;
    const int32_t fv = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rf, mine_at, 0, 0);
    const int32_t ov = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ro, mine_at, 0, 0);
#pragma nounroll
    for (int i = 0; i < kR; ++i) {
      if ((uint32_t)__builtin_amdgcn_readlane((int)mk, i) != 1u) break;   // past the batch (wave-uniform)
      const int F = __builtin_amdgcn_readlane(fv, i);
      if (F <= 0) continue;
      const int32_t a1 = __builtin_amdgcn_readlane(ix1, i), a2 = __builtin_amdgcn_readlane(ix2, i);
      const int n1 = __builtin_amdgcn_readlane(ix1, i + 1) - a1, n2 = __builtin_amdgcn_readlane(ix2, i + 1) - a2;
      const int32_t o = __builtin_amdgcn_readlane(ov, i);
      const int lo = max(0, F - n2), hi = min(n1, F);
      if ((uint32_t)n1 > (uint32_t)kMaxLen || (uint32_t)n2 > (uint32_t)kMaxLen || lo >= hi || o < 0)
        continue;   // (not what the find and the plan leave: nothing is touched)
      ++pairs;
      bases += (unsigned long long)F;
      const uint32_t sh = (uint32_t)o & 3u;
      uint32_t last_s = 0, last_q = 0;   // the merged bytes of the step before (lane 63's are lane 0's lower dword)
#pragma nounroll
      for (int p0 = 0; p0 < F + (int)sh; p0 += 256) {   // (F <= 1016: four steps at most)
        const int p = p0 + 4 * lane;
        const int rem = hi - p0;         // mate 1's bytes from p0 on (none: nothing is loaded)
        const uint32_t st1 = (uint32_t)a1 + s1.shift + (uint32_t)p0, sq1 = (uint32_t)a1 + q1.shift + (uint32_t)p0;
        const uint32_t b1 = reads::lane_bytes(reads::lane_load8(s1.bytes, st1, rem, lane), st1, rem, lane);
        const uint32_t p1 = reads::lane_bytes(reads::lane_load8(q1.bytes, sq1, rem, lane), sq1, rem, lane);
        const bool faces = p + 3 >= lo && p < F;
        const int j3 = F - 4 - p;        // the lowest of the four facing positions: -3 at least where the lane `faces`
        const uint32_t b2 = load4_backwards(s2.bytes, a2 + (int32_t)s2.shift + j3, faces);
        const uint32_t p2 = load4_backwards(q2.bytes, a2 + (int32_t)q2.shift + j3, faces);
        const Merged4 m4 = merge4(b1, p1, b2, p2, hi - p, lo - p);
        const uint32_t ms = m4.seq, mq = m4.qual;
        won1 += m4.won1;
        won2 += m4.won2;
        // the aligned output dword at position pa: the last sh bytes of the lane below, the lane's first 4 - sh
        const uint32_t us = (uint32_t)__builtin_amdgcn_ds_bpermute(((lane - 1) & 63) * 4, (int)(lane == 63 ? last_s : ms));
        const uint32_t uq = (uint32_t)__builtin_amdgcn_ds_bpermute(((lane - 1) & 63) * 4, (int)(lane == 63 ? last_q : mq));
        last_s = ms;
        last_q = mq;
        const uint32_t ds = sh ? __builtin_amdgcn_alignbyte(ms, us, 4u - sh) : ms;
        const uint32_t dq = sh ? __builtin_amdgcn_alignbyte(mq, uq, 4u - sh) : mq;
        const int pa = p - (int)sh;
        char *const os = seq_out + ((int64_t)o + pa), *const oq = qual_out + ((int64_t)o + pa);
        if (pa >= 0 && pa + 4 <= F) {
          *reinterpret_cast<uint32_t *>(os) = ds;
          *reinterpret_cast<uint32_t *>(oq) = dq;
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if ((uint32_t)(pa + t) < (uint32_t)F) {
              reinterpret_cast<uint8_t *>(os)[t] = (uint8_t)(ds >> (8 * t));
              reinterpret_cast<uint8_t *>(oq)[t] = (uint8_t)(dq >> (8 * t));
            }
        }
      }
    }
  }
  // the workgroup's four sums in LDS (u64: a lane's resolved bases stay below 2^32 in a part of 2^28 pairs of at
  // most 12 facing positions per lane; the bases are summed as u64 from the start), then one u64 atomic per
  // nonzero scalar
  if (threadIdx.x < kMergeScalars) red[threadIdx.x] = 0;
  __syncthreads();
  if (lane == 0 && pairs) {
    atomicAdd(&red[0], (unsigned long long)pairs);
    atomicAdd(&red[1], bases);
  }
  if (won1) atomicAdd(&red[2], (unsigned long long)won1);
  if (won2) atomicAdd(&red[3], (unsigned long long)won2);
  __syncthreads();
  if (threadIdx.x < kMergeScalars) {
    const unsigned long long s = red[threadIdx.x];
    if (s) atomicAdd(&scal[kScalars + kFixScalars + threadIdx.x], s);
  }
}

}  // namespace ovl
}  // namespace hpgq

// the scalars: [pairs, skipped, overlapping, clipped, bases_removed[2], corrected_pairs, corrected_bases[2],
// merged_pairs, merged_bases, resolved[2]]
struct hpgq_ovl : hpgq::cut::Cutter {
  int min_ov = 0, max_mm = 0;
  hpgq::cut::Positions pos[2];              // hpgq_ovl_batch_device's positions, per mate
  hpgq::cut::Kept kept[2];                  // and its outputs
  // §2.14, nothing of it allocated while both switches are off
  bool fix_on = false, hist_on = false;
  int phred = HPGQ_PHRED33, high = 30, low = 14;
  hpgq::cut::Positions ins;                 // F* (int32) where the caller keeps none
  const int32_t *last_ins = nullptr;        // hpgq_ovl_batch_device's, while a switch was on (hpgq_ovl_last_inserts)
  unsigned long long *d_hist = nullptr;     // [HPGQ_OVL_INSERT_BINS]
  // §2.15, nothing of it allocated before the first hpgq_ovl_merge_device
  hpgq::cut::Kept merged;                   // the merged reads
  hpgq::cut::Positions uidx[2];             // the unmerged outputs' uncompacted offsets (int32 [n + 1])
  hpgq::cut::Positions moff, rank;          // the merged reads' (int32 [n + 1]); the merged pairs up to each pair (int32 [n])
};

namespace {

using namespace hpgq::ovl;
using hpgq::cut::batch_ok;

bool pair_ok(const hpgq_batch_t *m1, const hpgq_batch_t *m2) {
  return batch_ok(m1) && batch_ok(m2) && m1->num_reads == m2->num_reads;
}

// the find pass over the pairs, async; every output may be null.  While the
// inserts are counted, F* goes to the handle's own buffer where the caller
// keeps none, and every part's into the histogram.
int find(hpgq_ovl *q, const hpgq_batch_t *m1, const hpgq_batch_t *m2, int32_t *ins, uint32_t *pos1, uint32_t *pos2) {
  if (!ins && q->hist_on) {
    const int rc = q->ins.need(*q, m1->num_reads);
    if (rc) return rc;
    ins = reinterpret_cast<int32_t *>(q->ins.d);
  }
  return hpgq::accum::for_parts(m1, nullptr, [&](const int32_t *ix1, const uint8_t *, int64_t n) {
    const int64_t lo = ix1 - m1->data_indices;
    // four workgroups of 512 threads per CU stay resident (5.5 KB of LDS each)
    const dim3 grid(q->grid(4, (n + kGroup - 1) / kGroup));
    hipLaunchKernelGGL(ovl_find_kernel, grid, dim3(kWG), 0, q->stream, m1->seq, ix1, m2->seq, m2->data_indices + lo, n,
                       q->min_ov, q->max_mm, ins ? ins + lo : nullptr, pos1 ? pos1 + lo : nullptr,
                       pos2 ? pos2 + lo : nullptr, q->d_scal);
    if (q->hist_on)
      hipLaunchKernelGGL(ovl_hist_kernel, dim3(q->grid(4, (n + kWG - 1) / kWG)), dim3(kWG), 0, q->stream, ins + lo, n,
                         q->d_hist);
  });
}

// §2.14's correction of the kept batches, async: after both copies
int fix(hpgq_ovl *q, int64_t n) {
  hpgq_batch_t k1;
  q->kept[0].give(&k1, n);
  const hpgq::cut::Kept &o1 = q->kept[0], &o2 = q->kept[1];
  return hpgq::accum::for_parts(&k1, nullptr, [&](const int32_t *ix1, const uint8_t *, int64_t np) {
    const int64_t lo = ix1 - o1.o_idx;
    const dim3 grid(q->grid(4, (np + kGroup - 1) / kGroup));
    hipLaunchKernelGGL(ovl_fix_kernel, grid, dim3(kWG), 0, q->stream, o1.o_seq, o1.o_qual, ix1, o2.o_seq, o2.o_qual,
                       o2.o_idx + lo, reinterpret_cast<const int32_t *>(q->ins.d) + lo, np, q->phred, q->high, q->low,
                       q->d_scal);
  });
}

// data[0, b's reads) into its inclusive sums, in place, async (the scan's storage: cut::scan_room)
int sum_in_place(hpgq_ovl *q, const hpgq_batch_t *b, int32_t *data) {
  int sum_rc = HPGQ_OK;
  const int rc = hpgq::accum::for_parts(b, nullptr, [&](const int32_t *ix, const uint8_t *, int64_t n) {
    const int64_t lo = ix - b->data_indices;
    size_t bytes = q->scan.tmp_bytes;
    if (hipcub::DeviceScan::InclusiveSum(q->scan.d_tmp, bytes, data + lo, data + lo, (int)n, q->stream) != hipSuccess)
      sum_rc = HPGQ_E_HIP;
    if (lo) hipLaunchKernelGGL(hpgq::cut::clip_carry_kernel, dim3(1024), dim3(256), 0, q->stream, data + lo, n, data + lo - 1);
  });
  return rc ? rc : sum_rc;
}

// §2.15 behind the find, async but for one wait: the plan, M, both unmerged
// copies, the three compacted data_indices, the merged reads
int merge(hpgq_ovl *q, const hpgq_batch_t b[2], int64_t *num_merged) {
  const int64_t n = b[0].num_reads;
  const int32_t *ins = reinterpret_cast<const int32_t *>(q->ins.d);
  int32_t *const u1 = reinterpret_cast<int32_t *>(q->uidx[0].d), *const u2 = reinterpret_cast<int32_t *>(q->uidx[1].d);
  int32_t *const um = reinterpret_cast<int32_t *>(q->moff.d), *const rank = reinterpret_cast<int32_t *>(q->rank.d);
  int rc = hpgq::accum::for_parts(&b[0], nullptr, [&](const int32_t *ix1, const uint8_t *, int64_t np) {
    const int64_t lo = ix1 - b[0].data_indices;
    hipLaunchKernelGGL(ovl_plan_kernel, dim3(q->grid(8, (np + 255) / 256)), dim3(256), 0, q->stream, ix1,
                       b[1].data_indices + lo, ins + lo, np, q->pos[0].d + lo, q->pos[1].d + lo, um + 1 + lo, rank + lo);
  });
  if (rc) return rc;
  HPGQ_HIP_TRY(hipMemsetAsync(um, 0, 4, q->stream));
  if ((rc = sum_in_place(q, &b[0], um + 1)) != HPGQ_OK || (rc = sum_in_place(q, &b[0], rank)) != HPGQ_OK) return rc;
  int32_t *const h_m = static_cast<int32_t *>(q->h_extra());
  HPGQ_HIP_TRY(hipMemcpyAsync(h_m, rank + n - 1, 4, hipMemcpyDeviceToHost, q->stream));
  HPGQ_HIP_TRY(hipStreamSynchronize(q->stream));
  const int64_t M = *h_m;
  if (M < 0 || M > n) return HPGQ_E_HIP;
  for (int m = 0; m < 2; ++m) {
    rc = hpgq::cut::scan_and_copy(*q, &b[m], q->pos[m].d, q->kept[m].o_seq, q->kept[m].o_qual, m ? u2 : u1);
    if (rc) return rc;
  }
  rc = hpgq::accum::for_parts(&b[0], nullptr, [&](const int32_t *ix1, const uint8_t *, int64_t np) {
    const int64_t lo = ix1 - b[0].data_indices;
    hipLaunchKernelGGL(ovl_compact_kernel, dim3(q->grid(8, (np + 255) / 256)), dim3(256), 0, q->stream, u1 + lo, u2 + lo,
                       um + lo, rank + lo, ins + lo, np, lo, lo + np == n ? 1 : 0, q->kept[0].o_idx, q->kept[1].o_idx,
                       q->merged.o_idx);
    if (M)
      hipLaunchKernelGGL(ovl_merge_kernel, dim3(q->grid(4, (np + kGroup - 1) / kGroup)), dim3(kWG), 0, q->stream, b[0].seq,
                         b[0].quality, ix1, b[1].seq, b[1].quality, b[1].data_indices + lo, ins + lo, um + lo, np,
                         q->merged.o_seq, q->merged.o_qual, q->d_scal);
  });
  *num_merged = M;
  return rc;
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
  if ((rc = q->open(device, stream, kScalars + kFixScalars + kMergeScalars)) != HPGQ_OK) {
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
  q->ins.free();
  (void)hipFree(q->d_hist);
  q->merged.free();
  for (int m = 0; m < 2; ++m) q->uidx[m].free();
  q->moff.free();
  q->rank.free();
  delete q;
}

int hpgq_ovl_find_device(hpgq_ovl_t *q, const hpgq_batch_t *m1, const hpgq_batch_t *m2, int32_t *insert_out,
                         uint32_t *pos1_out, uint32_t *pos2_out) {
  if (!q || !pair_ok(m1, m2)) return HPGQ_E_INVALID;
  if (m1->num_reads == 0) return HPGQ_OK;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  q->last_ins = nullptr;
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
  const bool fixes = q->fix_on && n;
  int rc = fixes ? q->ins.need(*q, n) : HPGQ_OK;
  if (rc) return rc;
  if (n) rc = find(q, &b[0], &b[1], fixes ? reinterpret_cast<int32_t *>(q->ins.d) : nullptr, q->pos[0].d, q->pos[1].d);
  for (int m = 0; m < 2 && rc == HPGQ_OK; ++m)
    rc = hpgq::cut::scan_and_copy(*q, &b[m], q->pos[m].d, q->kept[m].o_seq, q->kept[m].o_qual, q->kept[m].o_idx);
  if (rc == HPGQ_OK && fixes) rc = fix(q, n);
  if (rc) return rc;
  q->last_ins = n && (q->fix_on || q->hist_on) ? reinterpret_cast<const int32_t *>(q->ins.d) : nullptr;
  for (int m = 0; m < 2; ++m) q->kept[m].give(out[m], n);
  return HPGQ_OK;
}

int hpgq_ovl_merge_device(hpgq_ovl_t *q, const hpgq_batch_t *m1, const hpgq_batch_t *m2, hpgq_batch_t *out1,
                          hpgq_batch_t *out2, hpgq_batch_t *merged) {
  if (!q || !pair_ok(m1, m2) || !out1 || !out2 || !merged || out1 == out2 || merged == out1 || merged == out2)
    return HPGQ_E_INVALID;
  if (m1->num_reads && (!m1->quality || !m2->quality)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  const hpgq_batch_t b[2] = {*m1, *m2};   // (an input and an output may be the same struct)
  const int64_t n = b[0].num_reads;
  size_t held[2] = {0, 0};
  for (int m = 0; m < 2; ++m) {
    const int rc = hpgq::cut::Kept::held(*q, b[m], &held[m]);
    if (rc) return rc;
  }
  if (held[0] + held[1] > (size_t)INT32_MAX) return HPGQ_E_INVALID;   // (the merged offsets are int32)
  // a merged read has fewer bytes than its mates together
  int rc = q->merged.room(*q, held[0] + held[1], n);
  for (int m = 0; m < 2 && rc == HPGQ_OK; ++m) {
    rc = q->kept[m].room(*q, held[m], n);
    if (rc == HPGQ_OK && n) rc = q->pos[m].need(*q, n);
    if (rc == HPGQ_OK && n) rc = q->uidx[m].need(*q, n + 1);
  }
  if (rc == HPGQ_OK && n) rc = q->moff.need(*q, n + 1);
  if (rc == HPGQ_OK && n) rc = q->rank.need(*q, n);
  if (rc == HPGQ_OK && n) rc = q->ins.need(*q, n);
  if (rc == HPGQ_OK && n) rc = hpgq::cut::scan_room(*q, n);
  if (rc) return rc;
  int64_t M = 0;
  if (n) {
    rc = find(q, &b[0], &b[1], reinterpret_cast<int32_t *>(q->ins.d), nullptr, nullptr);
    if (rc == HPGQ_OK) rc = merge(q, b, &M);
    if (rc) return rc;
  } else {
    for (hpgq::cut::Kept *k : {&q->kept[0], &q->kept[1], &q->merged}) HPGQ_HIP_TRY(hipMemsetAsync(k->o_idx, 0, 4, q->stream));
  }
  q->last_ins = n ? reinterpret_cast<const int32_t *>(q->ins.d) : nullptr;
  q->kept[0].give(out1, n - M);
  q->kept[1].give(out2, n - M);
  q->merged.give(merged, M);
  return HPGQ_OK;
}

int hpgq_ovl_sync(hpgq_ovl_t *q) { return q ? q->settle() : HPGQ_E_INVALID; }

int hpgq_ovl_reset(hpgq_ovl_t *q) {
  if (!q) return HPGQ_E_INVALID;
  const int rc = q->reset();
  if (rc) return rc;
  if (q->d_hist) HPGQ_HIP_TRY(hipMemsetAsync(q->d_hist, 0, sizeof(uint64_t) * kBins, q->stream));
  return HPGQ_OK;
}

int hpgq_ovl_set_correct(hpgq_ovl_t *q, int on, int phred, int high, int low) {
  if (!q) return HPGQ_E_INVALID;
  if (on) {
    uint32_t none[2];
    if (hpgq_ovl_correct(nullptr, nullptr, 0, nullptr, nullptr, 0, 0, phred, high, low, none) == -2) return HPGQ_E_INVALID;   // the rules of §2.14
    q->phred = phred;
    q->high = high;
    q->low = low;
  }
  q->fix_on = on != 0;
  return HPGQ_OK;
}

int hpgq_ovl_count_inserts(hpgq_ovl_t *q, int on) {
  if (!q) return HPGQ_E_INVALID;
  if (on && !q->d_hist) {
    HPGQ_HIP_TRY(hipSetDevice(q->device));
    if (hipMalloc(&q->d_hist, sizeof(uint64_t) * kBins) != hipSuccess) return HPGQ_E_NOMEM;
    HPGQ_HIP_TRY(hipMemsetAsync(q->d_hist, 0, sizeof(uint64_t) * kBins, q->stream));
  }
  q->hist_on = on != 0;
  return HPGQ_OK;
}

int hpgq_ovl_last_inserts(hpgq_ovl_t *q, const int32_t **inserts) {
  if (!q || !inserts) return HPGQ_E_INVALID;
  *inserts = q->last_ins;
  return HPGQ_OK;
}

int hpgq_ovl_read_correct(hpgq_ovl_t *q, hpgq_ovl_correct_info_t *info) {
  if (!q || !info) return HPGQ_E_INVALID;
  const int rc = q->settle();
  if (rc) return rc;
  info->corrected_pairs = q->h_scal[kScalars];
  info->corrected_bases[0] = q->h_scal[kScalars + 1];
  info->corrected_bases[1] = q->h_scal[kScalars + 2];
  info->on = q->fix_on;
  info->phred = q->phred;
  info->high = q->high;
  info->low = q->low;
  return HPGQ_OK;
}

int hpgq_ovl_read_merge(hpgq_ovl_t *q, hpgq_ovl_merge_info_t *info) {
  if (!q || !info) return HPGQ_E_INVALID;
  const int rc = q->settle();
  if (rc) return rc;
  const unsigned long long *s = q->h_scal + kScalars + kFixScalars;
  info->merged_pairs = s[0];
  info->merged_bases = s[1];
  info->resolved[0] = s[2];
  info->resolved[1] = s[3];
  return HPGQ_OK;
}

int hpgq_ovl_read_inserts(hpgq_ovl_t *q, uint64_t hist[HPGQ_OVL_INSERT_BINS]) {
  if (!q || !hist) return HPGQ_E_INVALID;
  const int rc = q->settle();
  if (rc) return rc;
  if (!q->d_hist) {
    std::fill(hist, hist + kBins, (uint64_t)0);
    return HPGQ_OK;
  }
  HPGQ_HIP_TRY(hipMemcpy(hist, q->d_hist, sizeof(uint64_t) * kBins, hipMemcpyDeviceToHost));
  return HPGQ_OK;
}

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
