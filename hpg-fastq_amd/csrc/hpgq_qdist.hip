// hpgq_qdist.hip — `stats --quality-dist`: bases per (read position, raw
// quality byte), hist[p][b] u64.  Build-defined: the
// reference reports a mean per position only.
//
// One kernel.  It reads the quality bytes, the offsets and the mask and
// nothing else (L + 4 + 1 bytes per read).  A workgroup keeps a tile of kP =
// 256 positions x a window of kWin = 64 consecutive byte values [base, base +
// 64) in LDS as u32 ([64][256] = 64 KB, two workgroups per CU) for the whole
// call and adds the nonzero cells to hist once, at the end, with no-return u64
// global atomics.  Bytes outside the window go to hist directly (rare: real
// files use <= 64 values and the CLI passes phred as base); the result is
// exact for all 256 values either way.
//
// A wave takes kR = 16 consecutive reads per step: one coalesced load of their
// 17 offsets and 16 mask bytes, then one 8-byte load per read and lane, lane l
// dwords l and l+1 counted from the dword at or below the read's first byte
// (dword-aligned, coalesced along the read; the 16 loads are in flight
// together).  The read's bytes 4l..4l+3 are cut out of the two dwords by
// v_alignbyte, so lane l holds positions 4l..4l+3 and everything before the
// read's first and after its last byte is masked out.
//
// Layout [value][permuted position]: cell (v, p) at word v * 256 + (p & 3) *
// 64 + (p >> 2).  The ds_add_u32 of byte k of every lane goes to word v * 256
// + k * 64 + lane: a b32 access banks as word mod 32 within each 32-lane
// group, v * 256 and k * 64 are multiples of 32, so a group's 32 lanes sit on
// 32 banks whatever their values are.  (Position-major [p][v] would put every
// lane with the same value on one bank: stride 256 words.)
//
// Reads longer than a tile: the workgroup walks its read groups again for the
// next 256 positions (zero, count, flush per tile) while any of ITS counted
// reads reaches them, so 150 and 250 bp batches take one walk and one flush.
// The longest counted read goes to flags[0] (atomicMax, one per workgroup);
// a counted read longer than the table's rows has only its positions below the
// rows counted and adds 1 to flags[1] (hpgq_qdist_sync: HPGQ_E_READ_TOO_LONG).
#include "hpgq_accum.h"
#include "hpgq_reads.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace hpgq {
namespace qdist {

constexpr int kP = 256;     // positions per tile: 64 lanes x 4 bytes
constexpr int kWin = 64;    // byte values on chip
constexpr int kWG = 512;
constexpr int kWaves = kWG / 64;
constexpr int kR = 16;      // reads per wave step
constexpr int kGroup = kWaves * kR;   // reads per workgroup step
using reads::v2u;
static_assert((kP / 4) % 32 == 0, "a 32-lane group must span the 32 banks");
static_assert(kP == 4 * 64, "lane l holds positions 4l..4l+3 of the tile");
static_assert(kWin * kP * 4 == 65536, "the table is the whole static LDS");

// MASK: mask is not null (a compile-time choice: hpgq_reads.h)
template <bool MASK>
__global__ void __launch_bounds__(kWG) qdist_kernel(const char *qual, const int32_t *idx, int64_t n,
                                                    const uint8_t *mask, int rows, int base,
                                                    unsigned long long *hist, uint32_t *flags) {
  __shared__ uint32_t t[kWin * kP];   // [value - base][permuted position]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const reads::Batch rd = reads::open<MASK>(qual, idx, n, mask);
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  int longest = 0;          // over this wave's counted reads (wave-uniform)
  uint32_t clipped = 0;     // its counted reads longer than the table
  int wg_longest = 0;
  for (int p0 = 0;; p0 += kP) {
    for (int i = threadIdx.x; i < kWin * kP; i += kWG) t[i] = 0;
    __syncthreads();
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
      const int64_t rb = g * kGroup + wave * kR;
      if (rb >= n) continue;
      int32_t ix;
      uint32_t mk;
      reads::step_reads<kR, MASK>(rd, rb, n, lane, ix, mk);
      v2u w[kR];
      uint32_t st[kR];   // the tile's first byte of read i, from the descriptor's base (wave-uniform)
      int rem[kR];       // its positions in this tile and after (<= 0: none; wave-uniform)
#pragma unroll
      for (int i = 0; i < kR; ++i) {
        const int32_t a = __builtin_amdgcn_readlane(ix, i);
        const int32_t len = __builtin_amdgcn_readlane(ix, i + 1) - a;
        const bool cnt = (uint32_t)__builtin_amdgcn_readlane((int)mk, i) == 1u;
        if (p0 == 0 && cnt) {
          longest = max(longest, len);
          clipped += len > rows ? 1u : 0u;
        }
        rem[i] = cnt ? min(len, rows) - p0 : 0;
        st[i] = (uint32_t)a + rd.shift + (uint32_t)p0;
        // (handing the neighbour's dword over by ds_bpermute instead of loading
        // it was a fifth LDS instruction per read in a kernel the LDS atomics bound)
        w[i] = reads::lane_load8(rd.bytes, st[i], rem[i], lane);
      }
#pragma unroll
      for (int i = 0; i < kR; ++i) {
        if (rem[i] <= 0) continue;   // (wave-uniform)
        const uint32_t v = __builtin_amdgcn_alignbyte(w[i][1], w[i][0], st[i] & 3u);   // positions p0 + 4 lane + [0, 4)
        // (a branch-free form -- every lane adds 0 or 1, the bytes outside the
        // window collected for one wave-uniform branch -- measured 9 % slower:
        // DESIGN.md 4.10)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int p = 4 * lane + k;
          if (p >= rem[i]) continue;
          const uint32_t b = (v >> (8 * k)) & 255u;
          const uint32_t d = b - (uint32_t)base;
          if (d < (uint32_t)kWin)
            atomicAdd(&t[d * kP + k * (kP / 4) + lane], 1u);
          else   // outside the window (rare): straight to the table
            atomicAdd(&hist[(size_t)(p0 + p) * HPGQ_QDIST_VALUES + b], 1ull);
        }
      }
    }
    __syncthreads();
    // flush: a wave per position, lane = value, so a wave's 64 u64 adds are
    // 512 contiguous bytes of hist (the LDS reads of one position are a
    // 32-way bank conflict; once per tile)
    const int here = min(kP, rows - p0);
    for (int p = wave; p < here; p += kWaves) {
      const uint32_t c = t[lane * kP + (p & 3) * (kP / 4) + (p >> 2)];
      if (c) atomicAdd(&hist[(size_t)(p0 + p) * HPGQ_QDIST_VALUES + base + lane], (unsigned long long)c);
    }
    __syncthreads();
    if (p0 == 0) {   // the workgroup's longest counted read and clipped reads (the table is free)
      if (lane == 0) {
        t[wave] = (uint32_t)longest;
        t[kWaves + wave] = clipped;
      }
      __syncthreads();
      uint32_t cl = 0;
      for (int w2 = 0; w2 < kWaves; ++w2) {
        wg_longest = max(wg_longest, (int)t[w2]);
        cl += t[kWaves + w2];
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        if (wg_longest) atomicMax(&flags[0], (uint32_t)wg_longest);
        if (cl) atomicAdd(&flags[1], cl);
      }
    }
    if (min(wg_longest, rows) <= p0 + kP) break;
  }
}

}  // namespace qdist
}  // namespace hpgq

// the table: hist[rows][256]
struct hpgq_qdist : hpgq::accum::Positions {
  int base = 0;
};

namespace {
constexpr size_t kRowBytes = (size_t)HPGQ_QDIST_VALUES * 8;
}  // namespace

extern "C" {

int hpgq_qdist_open(hpgq_qdist_t **qd, int device, int rows, int base, void *stream) {
  if (!qd || rows < 1 || base < 0 || base > HPGQ_QDIST_VALUES - hpgq::qdist::kWin) return HPGQ_E_INVALID;
  *qd = nullptr;
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_qdist *q = new hpgq_qdist;
  q->base = base;
  if ((rc = q->open(device, stream, rows, kRowBytes, 0)) != HPGQ_OK) {
    hpgq_qdist_close(q);
    return rc;
  }
  *qd = q;
  return HPGQ_OK;
}

void hpgq_qdist_close(hpgq_qdist_t *q) {
  if (!q) return;
  q->close();
  delete q;
}

int hpgq_qdist_reserve_length(hpgq_qdist_t *q, int64_t max_len) {
  return q ? q->reserve_length(max_len) : HPGQ_E_INVALID;
}

int hpgq_qdist_count_device(hpgq_qdist_t *q, const hpgq_batch_t *b, const uint8_t *mask) {
  if (!q || !b || b->num_reads < 0) return HPGQ_E_INVALID;
  if (b->num_reads == 0) return HPGQ_OK;
  if (!b->quality || !b->data_indices) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(q->device));
  using namespace hpgq::qdist;
  return hpgq::accum::for_parts(b, mask, [&](const int32_t *ix, const uint8_t *mk, int64_t n) {
    // two workgroups per CU (64 KB of LDS each)
    const dim3 grid(q->grid(2, (n + kGroup - 1) / kGroup));
    hipLaunchKernelGGL(mk ? qdist_kernel<true> : qdist_kernel<false>, grid, dim3(kWG), 0, q->stream, b->quality, ix, n,
                       mk, (int)q->rows, q->base, q->d_table, q->d_flags);
  });
}

int hpgq_qdist_sync(hpgq_qdist_t *q) { return q ? q->settle() : HPGQ_E_INVALID; }

int hpgq_qdist_reset(hpgq_qdist_t *q) { return q ? q->reset() : HPGQ_E_INVALID; }

int hpgq_qdist_read(hpgq_qdist_t *q, uint64_t *hist, size_t n, int32_t *npos) {
  if (!q || !npos) return HPGQ_E_INVALID;
  const int rc = q->settle();
  if (rc) return rc;
  const size_t np = q->h_flags()[0];   // (<= rows: nothing clipped)
  *npos = (int32_t)np;
  if (!hist) return HPGQ_OK;
  if (n < np * HPGQ_QDIST_VALUES) return HPGQ_E_INVALID;
  return q->read_rows(hist, np);
}

int hpgq_qdist_debug_set_max_workgroups(hpgq_qdist_t *q, int max_wg) {
  return q ? q->set_max_workgroups(max_wg) : HPGQ_E_INVALID;
}

}  // extern "C"

