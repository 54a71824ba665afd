// hpgq_cut.h — cut positions -> a kept batch, for every handle that cuts reads
// at their end (hpgq_clip.hip, hpgq_ovl.hip).  Internal.
//
// Given per read the number of bytes it keeps (pos[i] <= its length), on the
// handle's stream and without waiting on another workgroup:
//
//   hipcub inclusive sum of the pos into idx_out[1 .. n], idx_out[0] = 0
//   clip_copy_kernel   sequence and quality [idx[i], idx[i] + pos[i]) to
//                      [idx_out[i], idx_out[i + 1]).
//
// Copy.  Read-major, kR reads per wave step.  Source and destination have any
// byte alignment, and reads of 0 .. 3 kept bases make several reads share one
// output dword, so no partial dword is ever read, modified and written: the
// dwords that lie whole inside a read's output range are assembled with
// v_alignbyte from two source dwords and stored as dwords; the up to three bytes
// before and after them are stored as bytes.  Every store is a vector store
// inside [idx_out[i], idx_out[i + 1]) of its read.
//
// The kernels are static: every handle's translation unit holds its own copy of
// the code, none of them a second implementation.
//
// The handles derive from Cutter: the stream, the replaced buffers, the
// scalars and the grid limits are accum::Handle's (hpgq_accum.h, DESIGN.md
// §4.14), as for the counters per read position.
#pragma once
#include "hpgq_accum.h"
#include "hpgq_reads.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace hpgq {
namespace cut {

constexpr int kWG = 512;
constexpr int kWaves = kWG / 64;
constexpr int kR = 16;                // reads per wave step
constexpr int kGroup = kWaves * kR;   // reads per workgroup step
using reads::v2u;

// The dwords that lie whole inside the output range [dst, dst + len) of one
// read, from s0 of the source descriptor on (any alignment, both; wave-uniform
// arguments): each is assembled from the two source dwords that hold its bytes
// (the last byte at most 3 past the range's: the slack) and stored as a dword.
__device__ __forceinline__ void copy_dwords(const __amdgpu_buffer_rsrc_t src, uint32_t s0, char *dst, int len, int lane) {
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (uintptr_t)len;
  const uintptr_t a0 = (d0 + 3) & ~(uintptr_t)3, a1 = d1 & ~(uintptr_t)3;   // the whole dwords: [a0, a1), none if a0 >= a1
  if (a0 >= a1) return;
  const int ndw = (int)((a1 - a0) >> 2);
  const uint32_t sa0 = s0 + (uint32_t)(a0 - d0);   // the source byte of a0
  for (int w = lane; w < ndw; w += 64) {
    const uint32_t sa = sa0 + 4u * (uint32_t)w;
    const v2u q = __builtin_amdgcn_raw_buffer_load_b64(src, sa & ~3u, 0, 0);
    *reinterpret_cast<uint32_t *>(a0 + 4u * (uintptr_t)w) = __builtin_amdgcn_alignbyte(q[1], q[0], sa & 3u);
  }
}

// The up to three bytes before and the up to three behind the whole dwords of a
// read's output range, of both streams at once: lanes 0 .. 2 and 3 .. 5 the
// sequence's, 6 .. 8 and 9 .. 11 the quality's.  A range that ends before its
// first dword boundary is all "before".  Byte loads inside the read, byte
// stores inside the range.
__device__ __forceinline__ void copy_edges(const char *seq, const char *qual, char *seq_out, char *qual_out, int len, int lane) {
  if (lane >= 12) return;
  const bool q = lane >= 6;
  const int e = q ? lane - 6 : lane;
  const char *src = q ? qual : seq;
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(q ? qual_out : seq_out), d1 = d0 + (uintptr_t)len;
  const uintptr_t a0 = (d0 + 3) & ~(uintptr_t)3, a1 = d1 & ~(uintptr_t)3;
  const uintptr_t at = e < 3 ? d0 + (uintptr_t)e : (a0 > a1 ? a0 : a1) + (uintptr_t)(e - 3);
  const bool mine = e < 3 ? at < (a0 < d1 ? a0 : d1) : at < d1;
  if (mine) *reinterpret_cast<uint8_t *>(at) = (uint8_t)src[at - d0];
}

static __global__ void __launch_bounds__(kWG) clip_copy_kernel(const char *seq, const char *qual, const int32_t *idx,
                                                               const int32_t *idx_out, int64_t n, char *seq_out,
                                                               char *qual_out) {
  const int lane = threadIdx.x & 63;
  // (the wave's number through an SGPR: the descriptors and offsets below stay scalar)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const reads::Batch rs = reads::open<false>(seq, idx, n, nullptr);
  const reads::Batch rq = reads::open<false>(qual, idx, n, nullptr);
  const __amdgpu_buffer_rsrc_t ro = reads::idx_rsrc(idx_out, n);
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t rb = g * kGroup + wave * kR;
    if (rb >= n) continue;
    int32_t ix;
    uint32_t mk;
    reads::step_reads<kR, false>(rs, rb, n, lane, ix, mk);
    const int64_t r = rb + lane;
    const int32_t ox =
        (int32_t)__builtin_amdgcn_raw_buffer_load_b32(ro, r <= n && lane <= kR ? (uint32_t)r * 4u : reads::kNone, 0, 0);
    for (int i = 0; i < kR; ++i) {
      if ((uint32_t)__builtin_amdgcn_readlane((int)mk, i) != 1u) break;   // past the batch (wave-uniform)
      const int32_t a = __builtin_amdgcn_readlane(ix, i);
      const int32_t o = __builtin_amdgcn_readlane(ox, i);
      const int32_t keep = __builtin_amdgcn_readlane(ox, i + 1) - o;
      if (keep <= 0) continue;
      copy_dwords(rs.bytes, (uint32_t)a + rs.shift, seq_out + o, keep, lane);
      copy_dwords(rq.bytes, (uint32_t)a + rq.shift, qual_out + o, keep, lane);
      copy_edges(seq + a, qual + a, seq_out + o, qual_out + o, keep, lane);
    }
  }
}

// out[i] += *carry: the running offset of the parts before this one
static __global__ void clip_carry_kernel(int32_t *out, int64_t n, const int32_t *carry) {
  const int32_t c = *carry;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] += c;
}

// a device buffer of at least `want` units in place of *p, the old one retired
template <class T>
int grow(accum::Handle &h, T **p, size_t unit, size_t want, bool zero) {
  T *d = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&d), want * unit) != hipSuccess) return HPGQ_E_NOMEM;
  if (zero) HPGQ_HIP_TRY(hipMemsetAsync(d, 0, want * unit, h.stream));
  if (*p) h.retired.add(*p);
  *p = d;
  return HPGQ_OK;
}

// the scan's temporary storage
struct Scan {
  char *d_tmp = nullptr;
  size_t tmp_bytes = 0;
  void free() { (void)hipFree(d_tmp); }
};

// What every handle that cuts owns: accum::Handle's (its pinned extra word:
// the two offsets Kept::reserve fetches) and the scan's storage.
struct Cutter : accum::Handle {
  Scan scan;
  void close() {
    accum::Handle::close();
    scan.free();
  }
};

inline bool batch_ok(const hpgq_batch_t *b) {
  return b && b->num_reads >= 0 && (b->num_reads == 0 || (b->seq && b->data_indices));
}

// positions a handle keeps for a caller that wants none: [cap]
struct Positions {
  uint32_t *d = nullptr;
  int64_t cap = 0;
  int need(accum::Handle &h, int64_t n) {
    if (n <= cap) return HPGQ_OK;
    const int64_t want = std::max<int64_t>(n, cap + cap / 2);
    const int rc = grow(h, &d, 4, (size_t)want, false);
    if (rc == HPGQ_OK) cap = want;
    return rc;
  }
  void free() { (void)hipFree(d); }
};

// the scan's storage for the inclusive sums of a batch of num_reads, part by part
inline int scan_room(Cutter &c, int64_t num_reads) {
  Scan &s = c.scan;
  const int first = (int)std::min<int64_t>(num_reads, accum::kPart);
  size_t tb = 0;
  HPGQ_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb, static_cast<const int32_t *>(nullptr),
                                                static_cast<int32_t *>(nullptr), first, c.stream));
  if (tb > s.tmp_bytes) {
    const int rc = grow(c, &s.d_tmp, 1, tb, false);
    if (rc) return rc;
    s.tmp_bytes = tb;
  }
  return HPGQ_OK;
}

// idx_out[0] = 0, idx_out[i + 1] = idx_out[i] + pos[i], then the copy; async
inline int scan_and_copy(Cutter &c, const hpgq_batch_t *b, const uint32_t *pos, char *seq_out, char *qual_out,
                         int32_t *idx_out) {
  Scan &s = c.scan;
  HPGQ_HIP_TRY(hipMemsetAsync(idx_out, 0, 4, c.stream));
  if (b->num_reads == 0) return HPGQ_OK;
  const int rc = scan_room(c, b->num_reads);
  if (rc) return rc;
  return accum::for_parts(b, nullptr, [&](const int32_t *ix, const uint8_t *, int64_t n) {
    const int64_t lo = ix - b->data_indices;
    size_t bytes = s.tmp_bytes;
    (void)hipcub::DeviceScan::InclusiveSum(s.d_tmp, bytes, reinterpret_cast<const int32_t *>(pos + lo), idx_out + lo + 1,
                                           (int)n, c.stream);
    if (lo) hipLaunchKernelGGL(clip_carry_kernel, dim3(1024), dim3(256), 0, c.stream, idx_out + lo + 1, n, idx_out + lo);
    const dim3 grid(c.grid(4, (n + kGroup - 1) / kGroup));
    hipLaunchKernelGGL(clip_copy_kernel, grid, dim3(kWG), 0, c.stream, b->seq, b->quality, ix, idx_out + lo, n, seq_out,
                       qual_out);
  });
}

// A kept batch in buffers the handle owns, grown as needed, HPGQ_DEVICE_SLACK
// readable bytes behind the data.
struct Kept {
  char *o_seq = nullptr, *o_qual = nullptr;
  int32_t *o_idx = nullptr;
  size_t o_bytes = 0;
  int64_t o_reads = -1;

  // Room for what b can keep at most: its bytes (its first and last offset live
  // on the device: fetched through the handle's pinned extra word, one wait for
  // the stream) and its reads.
  int reserve(accum::Handle &c, const hpgq_batch_t &b) {
    size_t bytes = 0;
    const int rc = held(c, b, &bytes);
    return rc ? rc : room(c, bytes, b.num_reads);
  }

  // the bytes b holds (one wait for the stream)
  static int held(accum::Handle &c, const hpgq_batch_t &b, size_t *bytes) {
    int32_t *const ends = static_cast<int32_t *>(c.h_extra());
    *bytes = 0;
    if (b.num_reads) {
      HPGQ_HIP_TRY(hipMemcpyAsync(ends, b.data_indices, 4, hipMemcpyDeviceToHost, c.stream));
      HPGQ_HIP_TRY(hipMemcpyAsync(ends + 1, b.data_indices + b.num_reads, 4, hipMemcpyDeviceToHost, c.stream));
      HPGQ_HIP_TRY(hipStreamSynchronize(c.stream));
      if (ends[1] < ends[0]) return HPGQ_E_INVALID;
      *bytes = (size_t)(ends[1] - ends[0]);
    }
    return HPGQ_OK;
  }

  // room for `bytes` bytes (and the slack) and `reads` reads
  int room(accum::Handle &c, size_t bytes, int64_t reads) {
    if (!o_seq || bytes > o_bytes) {
      const size_t cap = std::max(bytes, o_bytes + o_bytes / 2);
      int rc = grow(c, &o_seq, 1, cap + HPGQ_DEVICE_SLACK, true);
      if (rc == HPGQ_OK) rc = grow(c, &o_qual, 1, cap + HPGQ_DEVICE_SLACK, true);
      if (rc) return rc;
      o_bytes = cap;
    }
    if (reads > o_reads) {
      const int64_t cap = std::max<int64_t>(reads, o_reads + o_reads / 2);
      const int rc = grow(c, &o_idx, 4, (size_t)cap + 1, false);
      if (rc) return rc;
      o_reads = cap;
    }
    return HPGQ_OK;
  }

  void give(hpgq_batch_t *out, int64_t n) const {
    out->num_reads = n;
    out->seq = o_seq;
    out->quality = o_qual;
    out->data_indices = o_idx;
  }

  void free() {
    (void)hipFree(o_seq);
    (void)hipFree(o_qual);
    (void)hipFree(o_idx);
  }
};

}  // namespace cut
}  // namespace hpgq
