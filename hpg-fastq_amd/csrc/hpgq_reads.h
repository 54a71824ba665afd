// hpgq_reads.h — how a wave gets at the reads of a step (device side of the
// per-read kernels: hpgq_qdist.hip, hpgq_adapt.hip, hpgq_dup.hip, hpgq_clip.hip,
// hpgq_ovl.hip, hpgq_cut.h and the descriptors of hpgq_kmers.hip).  Everything here is inlined
// and wave-uniform but the lane's own offset, so the descriptors stay in SGPRs.
//
// What is readable.  A batch is n reads back to back in `bytes` (seq or
// quality), read r at [idx[r], idx[r + 1]), with HPGQ_DEVICE_SLACK readable
// bytes after idx[n].  The bytes go through a descriptor whose base is the
// dword at or below `bytes` and whose range ends with the slack, so a lane may
// load, dword-aligned, the bytes of the first dword before `bytes`, the bytes
// between and inside other reads and the slack past the last one; anything
// further -- kNone above all -- reads 0 and moves nothing.  The offsets and the
// mask bytes go through descriptors of exactly (n + 1) * 4 and n bytes (no
// mask: 0 bytes), so past the batch both read 0.
#pragma once
#include "hpgq_common.h"

namespace hpgq {
namespace reads {

typedef unsigned v2u __attribute__((ext_vector_type(2)));

constexpr uint32_t kNone = 0xFFFFFFF0u;   // an offset past every descriptor: reads 0, no traffic

// the n + 1 offsets of a batch
__device__ __forceinline__ __amdgpu_buffer_rsrc_t idx_rsrc(const int32_t *idx, int64_t n) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)idx, (short)0, (uint32_t)((n + 1) * 4), 0x00020000);
}

// its n mask bytes; have: mask is not null
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mask_rsrc(const uint8_t *mask, int64_t n, bool have) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)mask, (short)0, have ? (uint32_t)n : 0u, 0x00020000);
}

// A batch as a wave reads it.  A byte at offset o of `bytes` is at o + shift of
// the descriptor, which holds `limit` bytes.
struct Batch {
  __amdgpu_buffer_rsrc_t bytes, idx, mask;
  uint32_t shift, limit;
};

// MASK: mask is not null (a compile-time choice, as in kmer_tile_kernel)
template <bool MASK>
__device__ __forceinline__ Batch open(const char *bytes, const int32_t *idx, int64_t n, const uint8_t *mask) {
  Batch b;
  b.shift = (uint32_t)(reinterpret_cast<uintptr_t>(bytes) & 3u);
  const int32_t data_end = __builtin_amdgcn_readfirstlane(idx[n]);
  b.bytes = __builtin_amdgcn_make_buffer_rsrc((void *)(bytes - b.shift), (short)0,
                                              (uint32_t)data_end + b.shift + HPGQ_DEVICE_SLACK, 0x00020000);
  b.idx = idx_rsrc(idx, n);
  b.mask = mask_rsrc(mask, n, MASK);
  b.limit = (uint32_t)data_end + b.shift + HPGQ_DEVICE_SLACK;
  return b;
}

// A step's R reads from read `first` on, one coalesced load each: lane l takes
// the offset of read first + l (l <= R: R + 1 of them) into ix and the read's
// mask byte (l < R; no mask: 1) into mk.  Past the batch both read 0.
template <int R, bool MASK>
__device__ __forceinline__ void step_reads(const Batch &b, int64_t first, int64_t n, int lane, int32_t &ix,
                                           uint32_t &mk) {
  const int64_t r = first + lane;
  ix = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(b.idx, r <= n && lane <= R ? (uint32_t)r * 4u : kNone, 0, 0);
  const bool on = r < n && lane < R;
  mk = MASK ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(b.mask, on ? (uint32_t)r : kNone, 0, 0) : (on ? 1u : 0u);
}

// The 8 bytes of lane `lane` in a step of 4 bytes per lane: dwords l and l + 1
// from the dword at or below byte st of the descriptor; rem: the read's bytes
// from st on (a lane with none of them loads nothing).  v_alignbyte(w[1], w[0],
// st & 3) is then the read's bytes st + 4l .. st + 4l + 3.  Neighbours overlap
// by a dword, which the L1 serves.  The last byte is at most 6 past the read's
// end: inside the slack.
__device__ __forceinline__ v2u lane_load8(const __amdgpu_buffer_rsrc_t bytes, uint32_t st, int rem, int lane) {
  const bool need = 4 * lane < rem;
  return __builtin_amdgcn_raw_buffer_load_b64(bytes, need ? (st & ~3u) + 4u * (uint32_t)lane : kNone, 0, 0);
}

// A step's R reads one after the other, PRE of their first loads (lane_load8
// of the read's first 256 bytes) in flight; ix: step_reads' offsets.
// scanned(i, len): read i of len bytes is looked at (otherwise its load moves
// nothing); each(i, a, len, w): read i at a of `bytes`, w its first load.
// Both are wave-uniform but w.
template <int R, int PRE, class Scanned, class Each>
__device__ __forceinline__ void walk_reads(const Batch &b, int32_t ix, int lane, Scanned scanned, Each each) {
  static_assert(R % PRE == 0, "the reads of a wave step go in blocks of PRE");
  auto first_load = [&](int i) {
    const int32_t a = __builtin_amdgcn_readlane(ix, i);
    const int32_t len = __builtin_amdgcn_readlane(ix, i + 1) - a;
    return lane_load8(b.bytes, (uint32_t)a + b.shift, scanned(i, len) ? len : 0, lane);
  };
  v2u wq[PRE];
#pragma unroll
  for (int j = 0; j < PRE; ++j) wq[j] = first_load(j);
  for (int i0 = 0; i0 < R; i0 += PRE) {
#pragma unroll
    for (int j = 0; j < PRE; ++j) {
      const int i = i0 + j;
      const int32_t a = __builtin_amdgcn_readlane(ix, i);
      const int32_t len = __builtin_amdgcn_readlane(ix, i + 1) - a;
      const v2u w = wq[j];
      if (i0 + PRE < R) wq[j] = first_load(i + PRE);
      each(i, a, len, w);
    }
  }
}

// The lane's four bytes v (those past the read's end zeroed) as four 2-bit
// codes c (base j at bits 2j .. 2j + 1) and four validity bits ok (base j at bit
// j): the byte is exactly the one base with its code.  The four bytes at once:
// x the code of each byte ((b >> 1) & 3: A 0, C 1, T 2, G 3), d its difference
// from the one byte with that code that is a base (0x41 + 2 code, and T = 0x54
// for code 2), z bit 7 of every byte where d is 0 (the zero-byte test).
__device__ __forceinline__ void pack4(uint32_t v, uint32_t &c, uint32_t &ok) {
  const uint32_t x = v >> 1 & 0x03030303u;
  const uint32_t isT = x >> 1 & ~x & 0x01010101u;
  const uint32_t d = v ^ (0x41414141u + 2u * x + 15u * isT);
  const uint32_t z = ~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
  c = (x | x >> 6 | x >> 12 | x >> 18) & 0xFFu;
  ok = (z >> 7 | z >> 14 | z >> 21 | z >> 28) & 0xFu;
}

// the lane's bytes st + 4 lane .. + 3 of a read with rem bytes from st on
__device__ __forceinline__ uint32_t lane_bytes(v2u w, uint32_t st, int rem, int lane) {
  const int nb = rem - 4 * lane;
  const uint32_t raw = __builtin_amdgcn_alignbyte(w[1], w[0], st & 3u);
  return nb >= 4 ? raw : nb <= 0 ? 0u : raw & ((1u << (8 * nb)) - 1u);
}

}  // namespace reads
}  // namespace hpgq
