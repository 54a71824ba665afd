// hpgq_dup.hip — `stats --duplication`: how often every sequence occurs, exactly
// (DESIGN.md §2.9, §4.11).  Build-defined: comparable tools estimate it from a
// sample of truncated reads.
//
// Two kernels per batch, on one stream.
//
// fp_kernel reads the sequence bytes, the offsets and the mask (L + 4 + 1 bytes
// per read) and writes one 64-bit fingerprint per read (0 for a read the mask
// leaves out).  A lane owns kLane = 16 bytes (two words of §2.9's sum), a
// segment of kSeg = 10 lanes one read, so a wave takes kSegs = 6 consecutive
// reads per step and a 150-base read fills its segment in one pass; a longer
// read walks its segment along (160 bytes per pass), a read longer than
// kWaveRead takes the whole wave (1024 bytes per pass).  A lane's 16 bytes
// start anywhere: it loads the five dwords that cover them (one 16-byte and one
// 4-byte load, dword-aligned, coalesced along the read) and cuts its four out
// with v_alignbyte; the bytes past the read's end are masked to 0.  The terms
// commute, so the segment adds them up in any order (four shuffle steps).
//
// insert_kernel takes one key per lane (64 independent probe chains per wave
// in flight): home slot key & (cap - 1), linear probing, the slot claimed by a
// returning 64-bit compare-and-swap 0 -> key, the count raised by a no-return
// u64 add on the same 16-byte slot.  The same kernel is the import (keys and
// counts from the host) and the rehash into a larger table (keys and counts
// are the old slots, stride 2).  One kernel with the fingerprint pass would
// leave 6 lanes of 64 probing; two cost 16 bytes per read of extra traffic.
// The reads' fingerprints are first summed per workgroup in a small LDS table,
// so a sequence that holds a large share of the reads is one global atomic per
// workgroup, not one per read on one address.
//
// No loop is unbounded: a chain ends after `cap` probes and sets the error
// word (hpgq_dup_sync: HPGQ_E_STATE).  The host keeps the table at most half
// full before every launch from an upper bound on the occupied slots, so that
// never happens.  Claimers count the occupied slots, one atomic per wave.
//
// `stats --overrepresented` adds a third kernel per
// batch, only for a table in keeping mode: keep_kernel looks every read's key
// up again and copies the bytes of a read whose key has reached the threshold
// and has no representative yet into the table's arena, once per key.
// select_kernel compacts the slots at or above a count for hpgq_dup_top.
#include "hpgq_accum.h"
#include "hpgq_reads.h"

#include <algorithm>
#include <vector>

namespace hpgq {
namespace dup {

constexpr int kWG = 256;
constexpr int kWaves = kWG / 64;
constexpr int kLane = 16;                 // bytes a lane owns per pass
constexpr int kSeg = 10;                  // lanes per read
constexpr int kSegs = 6;                  // reads per wave step
constexpr int kStep = kSeg * kLane;       // bytes of a read per pass of its segment
constexpr int kGroup = kWaves * kSegs;    // reads per workgroup step
constexpr int kWaveRead = 2048;           // a longer read takes the whole wave
constexpr int kLds = 1024;                // slots of insert_kernel's table in LDS (16 KB: 8 workgroups per CU)
constexpr int kLdsProbes = 4;
using reads::kNone;
constexpr uint64_t kG = 0x9E3779B97F4A7C15ULL;
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;
static_assert(kSegs * kSeg <= 64 && kSegs + 1 <= 64, "a wave holds its segments and their offsets");

// state words on the device (kError: bit 0 a full table, bit 1 a full arena)
enum { kOccupied = 0, kError = 1, kCursor = 2, kArena = 3, kKeptSeqs = 4, kKeptBytes = 5, kFound = 6, kStateWords = 8 };
constexpr u64 kErrFull = 1, kErrArena = 2;
// a slot's representative word (keeping mode): none, claimed by
// a lane of keep_kernel, or kRepFirst + (arena offset of its header) / 16
constexpr u64 kRepNone = 0, kRepBusy = 1, kRepFirst = 2;
constexpr int kRepHeader = 16;            // {length, key} before the bytes, which start 16-byte aligned
// result words of levels_kernel
enum { kMax = 2 * HPGQ_DUP_LEVELS, kLevelWords = 2 * HPGQ_DUP_LEVELS + 1 };

__device__ inline u64 shfl_down64(u64 v, int d) {
  const unsigned lo = __shfl_down((unsigned)v, d), hi = __shfl_down((unsigned)(v >> 32), d);
  return ((u64)hi << 32) | lo;
}

// The five dwords from the dword-aligned byte `al` of the descriptor (`limit`
// bytes): they cover any 16 bytes that start in the first of them.  (Not
// reads::lane_load8: a lane here takes 20 bytes, which may end further past
// the read's end than the slack reaches, so it checks `limit` itself.)
__device__ inline void lane_dwords(const __amdgpu_buffer_rsrc_t rs, uint32_t limit, uint32_t al, uint32_t &d0,
                                   uint32_t &d1, uint32_t &d2, uint32_t &d3, uint32_t &d4) {
  if (al + 20u <= limit) {
    const v4u q = __builtin_amdgcn_raw_buffer_load_b128(rs, al, 0, 0);
    d4 = __builtin_amdgcn_raw_buffer_load_b32(rs, al + 16u, 0, 0);
    d0 = q[0];
    d1 = q[1];
    d2 = q[2];
    d3 = q[3];
  } else {   // the batch's last bytes: dword by dword, each inside the slack
    d0 = __builtin_amdgcn_raw_buffer_load_b32(rs, al + 4u <= limit ? al : kNone, 0, 0);
    d1 = __builtin_amdgcn_raw_buffer_load_b32(rs, al + 8u <= limit ? al + 4u : kNone, 0, 0);
    d2 = __builtin_amdgcn_raw_buffer_load_b32(rs, al + 12u <= limit ? al + 8u : kNone, 0, 0);
    d3 = __builtin_amdgcn_raw_buffer_load_b32(rs, al + 16u <= limit ? al + 12u : kNone, 0, 0);
    d4 = 0;   // (al + 20 > limit: no byte of a read is there)
  }
}

// The terms of the (at most two) words that begin in the `rem` bytes from byte
// `p` of the descriptor, the first of them word j of its read, jg = (j + 1) G
// (the callers step it by additions: a 64-bit multiply is a dozen quarter-rate
// instructions).  `limit`: the descriptor's bytes.  No dword that begins past the read's end + 3 is asked
// for beyond `limit`, whatever the hardware's range check would do with it.
__device__ inline u64 lane_terms(const __amdgpu_buffer_rsrc_t rs, uint32_t limit, uint32_t p, int rem, u64 jg) {
  if (rem <= 0) return 0;
  const uint32_t sh = p & 3u;
  uint32_t d0, d1, d2, d3, d4;
  lane_dwords(rs, limit, p & ~3u, d0, d1, d2, d3, d4);
  u64 w = ((u64)__builtin_amdgcn_alignbyte(d2, d1, sh) << 32) | __builtin_amdgcn_alignbyte(d1, d0, sh);
  if (rem < 8) w &= (1ull << (8 * rem)) - 1ull;
  u64 s = mix64(w + jg);
  if (rem > 8) {
    w = ((u64)__builtin_amdgcn_alignbyte(d4, d3, sh) << 32) | __builtin_amdgcn_alignbyte(d3, d2, sh);
    if (rem < 16) w &= (1ull << (8 * (rem - 8))) - 1ull;
    s += mix64(w + jg + kG);
  }
  return s;
}

// MASK: mask is not null (a compile-time choice: hpgq_reads.h)
template <bool MASK>
__global__ void __launch_bounds__(kWG) fp_kernel(const char *seq, const int32_t *idx, int64_t n, const uint8_t *mask,
                                                 u64 *out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = lane / kSeg, pos = lane - seg * kSeg;   // (lanes 60..63: segment 6, no read)
  const reads::Batch rd = reads::open<MASK>(seq, idx, n, mask);
  const __amdgpu_buffer_rsrc_t rs = rd.bytes;
  const uint32_t shift = rd.shift, limit = rd.limit;
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  // (j + 1) G of the lane's first word in the first pass of its segment / of the whole wave
  const u64 seg_jg = (u64)(kLane / 8 * pos + 1) * kG, wave_jg = (u64)(kLane / 8 * lane + 1) * kG;
  // the offsets and mask bytes of workgroup step g
  auto offsets = [&](int64_t g, int32_t &ix, uint32_t &mk) {
    reads::step_reads<kSegs, MASK>(rd, g * kGroup + wave * kSegs, n, lane, ix, mk);
  };
  int32_t ix = 0, ix_next = 0;
  uint32_t mk = 0, mk_next = 0;
  if ((int64_t)blockIdx.x < ngroups) offsets(blockIdx.x, ix, mk);
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x, ix = ix_next, mk = mk_next) {
    // the next step's offsets are on their way while this step's bytes are loaded and mixed:
    // one memory round trip per step on the critical path, not two
    if (g + gridDim.x < ngroups) offsets(g + gridDim.x, ix_next, mk_next);
    const int64_t rb = g * kGroup + wave * kSegs;   // (a wave past the batch: every lane off, nothing loaded or stored)
    // the lane's own read
    const int32_t a = __shfl(ix, seg), e = __shfl(ix, seg + 1);
    const bool cnt = seg < kSegs && __shfl((int)mk, seg) == 1;
    const int len = cnt ? e - a : 0;
    const int slen = len > kWaveRead ? 0 : len;   // what the segment adds itself
    const uint32_t p0 = (uint32_t)a + shift;
    u64 sum = 0, jg = seg_jg;
    for (int off = kLane * pos; __any(off < slen); off += kStep, jg += (u64)(kStep / 8) * kG)
      sum += lane_terms(rs, limit, p0 + (uint32_t)off, slen - off, jg);
    u64 t = shfl_down64(sum, 8);
    if (pos < 2) sum += t;
    t = shfl_down64(sum, 4);
    if (pos < 4) sum += t;
    t = shfl_down64(sum, 2);
    if (pos < 2) sum += t;
    t = shfl_down64(sum, 1);
    if (pos < 1) sum += t;
#pragma unroll
    for (int s = 0; s < kSegs; ++s) {   // the long reads of the step, one after the other (wave-uniform)
      const int32_t as = __builtin_amdgcn_readlane(ix, s);
      const int32_t ls = __builtin_amdgcn_readlane(ix, s + 1) - as;
      if ((uint32_t)__builtin_amdgcn_readlane((int)mk, s) != 1u || ls <= kWaveRead) continue;
      u64 ws = 0, wg = wave_jg;
      for (int base = 0; base < ls; base += 64 * kLane, wg += (u64)(64 * kLane / 8) * kG) {
        const int off = base + kLane * lane;
        ws += lane_terms(rs, limit, (uint32_t)as + shift + (uint32_t)off, ls - off, wg);
      }
      for (int d = 32; d >= 1; d >>= 1) ws += shfl_down64(ws, d);   // (lane 0 holds the sum)
      const unsigned lo = __shfl((unsigned)ws, 0), hi = __shfl((unsigned)(ws >> 32), 0);
      if (lane == s * kSeg) sum = ((u64)hi << 32) | lo;
    }
    if (seg < kSegs && pos == 0 && rb + seg < n) {
      u64 fp = 0;   // a read the mask leaves out: no key
      if (cnt) {
        fp = mix64(sum ^ ((u64)(uint32_t)len * kG));
        fp = fp ? fp : 1ull;
      }
      out[rb + seg] = fp;
    }
  }
}

// key with count c into tab: at most `cap` probes.  claimed: +1 if this call claimed the slot.
__device__ inline bool table_add(u64 *tab, u64 capmask, u64 key, u64 c, uint32_t &claimed) {
  u64 s = key & capmask;
  for (u64 probe = 0; probe <= capmask; ++probe) {
    // (a key never changes once set: a stale 0 goes to the compare-and-swap, which decides)
    u64 k = __hip_atomic_load(&tab[2 * s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) {
      k = atomicCAS(&tab[2 * s], 0ull, key);
      if (k == 0) {
        ++claimed;
        k = key;
      }
    }
    if (k == key) {
      atomicAdd(&tab[2 * s + 1], c);
      return true;
    }
    s = (s + 1) & capmask;
  }
  return false;   // the table is full
}

// keys[i * stride] (0: nothing) with counts[i * stride] (counts == NULL: 1) into tab.
// AGG (the reads' fingerprints): a key first looks for itself in a small table
// in LDS (kLds slots, kLdsProbes probes from bits of the key the home slot does
// not use) and is added there if it is there or finds a free slot, else it goes
// to `tab` directly; the workgroup adds its LDS table to `tab` once, at the end.
// A sequence that makes up a large share of the reads is then one global atomic
// per workgroup, not one per read on one address (22 ms per 10 M
// reads with one sequence in ten without this).  Keys that are all different
// (import, rehash) skip it.
template <bool AGG>
__global__ void __launch_bounds__(kWG) insert_kernel(const u64 *keys, const u64 *counts, int64_t n, int stride, u64 *tab,
                                                     u64 capmask, u64 *state) {
  __shared__ u64 lk[AGG ? kLds : 1], lc[AGG ? kLds : 1];
  if (AGG) {
    for (int i = threadIdx.x; i < kLds; i += kWG) lk[i] = lc[i] = 0;
    __syncthreads();
  }
  uint32_t claimed = 0;
  bool full = false;
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWG) {
    const u64 key = keys[i * stride];
    if (!key) continue;
    const u64 c = counts ? counts[i * stride] : 1ull;
    bool here = false;
    if (AGG) {
      uint32_t h = (uint32_t)(key >> 40) & (kLds - 1);
      for (int p = 0; p < kLdsProbes && !here; ++p) {
        u64 k = __hip_atomic_load(&lk[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == 0) {
          k = atomicCAS(&lk[h], 0ull, key);
          if (k == 0) k = key;
        }
        if (k == key) {
          atomicAdd(&lc[h], c);
          here = true;
        }
        h = (h + 1) & (kLds - 1);
      }
    }
    if (!here && !table_add(tab, capmask, key, c, claimed)) full = true;
  }
  if (AGG) {
    __syncthreads();
    for (int i = threadIdx.x; i < kLds; i += kWG)
      if (lk[i] && !table_add(tab, capmask, lk[i], lc[i], claimed)) full = true;
  }
  for (int d = 32; d >= 1; d >>= 1) claimed += __shfl_xor(claimed, d);
  const bool any_full = __any(full);
  if ((threadIdx.x & 63) == 0) {
    if (claimed) atomicAdd(&state[kOccupied], (u64)claimed);
    if (any_full) atomicOr(&state[kError], 1ull);
  }
}

__device__ inline int level_of(u64 c) {
  const u64 lo[HPGQ_DUP_LEVELS] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000};
  int lv = 0;
#pragma unroll
  for (int i = 1; i < HPGQ_DUP_LEVELS; ++i) lv += c >= lo[i] ? 1 : 0;
  return lv;
}

// res[lv] += sequences at level lv, res[16 + lv] += their reads, res[32] = max count
__global__ void __launch_bounds__(kWG) levels_kernel(const u64 *tab, u64 cap, u64 *res) {
  __shared__ u64 bins[kLevelWords];
  if (threadIdx.x < kLevelWords) bins[threadIdx.x] = 0;
  __syncthreads();
  u64 ones = 0, mx = 0;   // (most sequences occur once: counted in a register)
  for (u64 i = (u64)blockIdx.x * kWG + threadIdx.x; i < cap; i += (u64)gridDim.x * kWG) {
    const ulonglong2 sl = reinterpret_cast<const ulonglong2 *>(tab)[i];
    if (!sl.x) continue;
    const u64 c = sl.y;
    mx = c > mx ? c : mx;
    if (c == 1) {
      ++ones;
    } else if (c) {
      const int lv = level_of(c);
      atomicAdd(&bins[lv], 1ull);
      atomicAdd(&bins[HPGQ_DUP_LEVELS + lv], c);
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    ones += shfl_down64(ones, d);
    const u64 o = shfl_down64(mx, d);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    if (ones) {
      atomicAdd(&bins[0], ones);
      atomicAdd(&bins[HPGQ_DUP_LEVELS], ones);
    }
    if (mx) atomicMax(&bins[kMax], mx);
  }
  __syncthreads();
  if (threadIdx.x < kLevelWords && bins[threadIdx.x]) {   // one atomic per nonzero bin
    if (threadIdx.x == kMax) atomicMax(&res[kMax], bins[kMax]);
    else atomicAdd(&res[threadIdx.x], bins[threadIdx.x]);
  }
}

// the occupied slots to keys[] / counts[], at most n of them, in the order the waves arrive
__global__ void __launch_bounds__(kWG) export_kernel(const u64 *tab, u64 cap, u64 *keys, u64 *counts, u64 n,
                                                     u64 *state) {
  const int lane = threadIdx.x & 63;
  for (u64 base = (u64)blockIdx.x * kWG; base < cap; base += (u64)gridDim.x * kWG) {   // (uniform trip count)
    const u64 i = base + threadIdx.x;
    ulonglong2 sl = {0, 0};
    if (i < cap) sl = reinterpret_cast<const ulonglong2 *>(tab)[i];
    const bool occ = sl.x != 0;
    const u64 b = __ballot(occ);
    if (!b) continue;
    u64 first = 0;
    if (lane == 0) first = atomicAdd(&state[kCursor], (u64)__popcll(b));
    const unsigned lo = __shfl((unsigned)first, 0), hi = __shfl((unsigned)(first >> 32), 0);
    const u64 at = (((u64)hi << 32) | lo) + (u64)__popcll(b & ((1ull << lane) - 1ull));
    if (occ && at < n) {
      keys[at] = sl.x;
      counts[at] = sl.y;
    }
  }
}

// hpgq_dup_top: export_kernel's compaction over the slots with count >= min_count.
// With n == 0 nothing is written and the cursor counts them (the first pass).
__global__ void __launch_bounds__(kWG) select_kernel(const u64 *tab, u64 cap, u64 min_count, u64 *keys, u64 *counts, u64 n,
                                                     u64 *state) {
  const int lane = threadIdx.x & 63;
  for (u64 base = (u64)blockIdx.x * kWG; base < cap; base += (u64)gridDim.x * kWG) {   // (uniform trip count)
    const u64 i = base + threadIdx.x;
    ulonglong2 sl = {0, 0};
    if (i < cap) sl = reinterpret_cast<const ulonglong2 *>(tab)[i];
    const bool hit = sl.x != 0 && sl.y >= min_count;
    const u64 b = __ballot(hit);
    if (!b) continue;
    u64 first = 0;
    if (lane == 0) first = atomicAdd(&state[kCursor], (u64)__popcll(b));
    const unsigned lo = __shfl((unsigned)first, 0), hi = __shfl((unsigned)(first >> 32), 0);
    const u64 at = (((u64)hi << 32) | lo) + (u64)__popcll(b & ((1ull << lane) - 1ull));
    if (hit && at < n) {
      keys[at] = sl.x;
      counts[at] = sl.y;
    }
  }
}

// the slot of a key that is in tab; false: it is not (a free slot or `cap` probes end the chain)
__device__ inline bool table_find(const u64 *tab, u64 capmask, u64 key, u64 &slot) {
  u64 s = key & capmask;
  for (u64 probe = 0; probe <= capmask; ++probe) {
    const u64 k = tab[2 * s];
    if (k == key) {
      slot = s;
      return true;
    }
    if (k == 0) return false;
    s = (s + 1) & capmask;
  }
  return false;
}

// The 16 bytes from byte p of the descriptor, bytes from `rem` on as 0: the five
// dwords that cover them (lane_dwords), cut with v_alignbyte.
__device__ inline v4u lane_bytes(const __amdgpu_buffer_rsrc_t rs, uint32_t limit, uint32_t p, int rem) {
  const uint32_t sh = p & 3u;
  uint32_t d0, d1, d2, d3, d4;
  lane_dwords(rs, limit, p & ~3u, d0, d1, d2, d3, d4);
  v4u w = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
           __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int left = rem - 4 * k;   // bytes of dword k that belong to the read
    if (left < 4) w[k] = left <= 0 ? 0u : w[k] & ((1u << (8 * left)) - 1u);
  }
  return w;
}

// Keeping mode, after the part's insert_kernel on the
// same stream: one fingerprint per lane (0: a read the mask left out), its slot
// found from the home slot, its count read.  A key at or above `min_count` whose
// representative word is kRepNone is claimed by one returning compare-and-swap
// to kRepBusy; nobody waits on that word (other lanes only see it nonzero, the
// host and the rehash read it after the kernel).  The wave's winners reserve
// kRepHeader + their length rounded up to 16 bytes each with ONE returning add
// on the arena cursor; a winner whose reservation passes `arena_bytes` sets
// kErrArena and puts kRepNone back.  The others are copied one after the other
// by the whole wave, 16 bytes per lane per pass, with 16-byte stores (the
// arena and every reservation are 16-byte aligned).  Winners are rare: a key
// is copied once in the table's life.
__global__ void __launch_bounds__(kWG) keep_kernel(const char *seq, const int32_t *idx, int64_t n, const u64 *fp,
                                                   const u64 *tab, u64 *rep, u64 capmask, u64 min_count,
                                                   unsigned char *arena, u64 arena_bytes, u64 *state) {
  const int lane = threadIdx.x & 63;
  // (the bytes alone: a lane reads its own read's two offsets with plain loads, and the keys are the mask)
  const reads::Batch rd = reads::open<false>(seq, idx, n, nullptr);
  const __amdgpu_buffer_rsrc_t rs = rd.bytes;
  const uint32_t shift = rd.shift, limit = rd.limit;
  u64 kept = 0, kept_bytes = 0;   // (wave-uniform)
  bool lost = false;
  for (int64_t base = (int64_t)blockIdx.x * kWG; base < n; base += (int64_t)gridDim.x * kWG) {   // (uniform trip count)
    const int64_t i = base + threadIdx.x;
    const u64 key = i < n ? fp[i] : 0ull;
    u64 slot = 0;
    bool win = false;
    if (key) {
      if (!table_find(tab, capmask, key, slot)) {
        lost = true;   // (the insert put it there: unreachable)
      } else if (tab[2 * slot + 1] >= min_count &&
                 __hip_atomic_load(&rep[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kRepNone) {
        win = atomicCAS(&rep[slot], kRepNone, kRepBusy) == kRepNone;
      }
    }
    u64 b = __ballot(win);
    if (!b) continue;
    const uint32_t a = win ? (uint32_t)idx[i] : 0u;
    const uint32_t len = win ? (uint32_t)idx[i + 1] - a : 0u;
    const u64 need = (u64)kRepHeader + (((u64)len + 15ull) & ~15ull);
    u64 total = 0, before = 0;
    for (u64 m = b; m; m &= m - 1ull) {
      const int w = __ffsll((long long)m) - 1;
      if (lane == w) before = total;
      total += (u64)kRepHeader + (((u64)__shfl(len, w) + 15ull) & ~15ull);
    }
    u64 first = 0;
    if (lane == 0) first = atomicAdd(&state[kArena], total);
    const unsigned flo = __shfl((unsigned)first, 0), fhi = __shfl((unsigned)(first >> 32), 0);
    const u64 off = (((u64)fhi << 32) | flo) + before;
    if (win && off + need > arena_bytes) {
      atomicOr(&state[kError], kErrArena);
      __hip_atomic_store(&rep[slot], kRepNone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      win = false;
    }
    b = __ballot(win);
    for (u64 m = b; m; m &= m - 1ull) {
      const int w = __ffsll((long long)m) - 1;
      const uint32_t aw = __shfl(a, w), lw = __shfl(len, w);
      const unsigned olo = __shfl((unsigned)off, w), ohi = __shfl((unsigned)(off >> 32), w);
      unsigned char *dst = arena + (((u64)ohi << 32) | olo);
      if (lane == w) *reinterpret_cast<ulonglong2 *>(dst) = ulonglong2{(u64)len, key};
      for (uint32_t o = (uint32_t)(kLane * lane); o < lw; o += 64u * kLane)
        *reinterpret_cast<v4u *>(dst + kRepHeader + o) = lane_bytes(rs, limit, aw + shift + o, (int)(lw - o));
      ++kept;
      kept_bytes += lw;
    }
    if (win) __hip_atomic_store(&rep[slot], kRepFirst + off / 16ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const bool any_lost = __any(lost);
  if (lane == 0) {
    if (kept) {
      atomicAdd(&state[kKeptSeqs], kept);
      atomicAdd(&state[kKeptBytes], kept_bytes);
    }
    if (any_lost) atomicOr(&state[kError], kErrFull);
  }
}

// the rehash in keeping mode, after its insert_kernel: every old slot's
// representative word to the key's new slot (the keys are distinct: a plain store)
__global__ void __launch_bounds__(kWG) carry_kernel(const u64 *old_tab, const u64 *old_rep, u64 old_cap, const u64 *tab,
                                                    u64 *rep, u64 capmask, u64 *state) {
  for (u64 i = (u64)blockIdx.x * kWG + threadIdx.x; i < old_cap; i += (u64)gridDim.x * kWG) {
    const u64 r = old_rep[i];
    if (r == kRepNone) continue;
    u64 slot = 0;
    if (table_find(tab, capmask, old_tab[2 * i], slot)) rep[slot] = r;
    else atomicOr(&state[kError], kErrFull);
  }
}

// hpgq_dup_sequence: the representative word of one key to state[kFound] (kRepNone: absent)
__global__ void find_kernel(const u64 *tab, const u64 *rep, u64 capmask, u64 key, u64 *state) {
  u64 slot = 0;
  state[kFound] = table_find(tab, capmask, key, slot) ? rep[slot] : kRepNone;
}

}  // namespace dup
}  // namespace hpgq

struct hpgq_dup {
  int device = 0;
  int log2 = 0, log2_max = 0;
  hpgq::accum::Stream stream;
  unsigned long long *d_tab = nullptr;     // [2^log2] {key, count}
  unsigned long long *d_state = nullptr;   // kStateWords words, see the enum
  unsigned long long *d_res = nullptr;     // levels_kernel's result
  unsigned long long *h_state = nullptr;   // pinned: the state words and the levels' words after them
  unsigned long long *d_fp = nullptr;      // one fingerprint per read of the batch in flight
  int64_t fp_cap = 0;
  uint64_t bound = 0;                      // occupied slots, an upper bound: the last count read + keys added since
  int cus = 0, max_wg = 0;
  int64_t rehashes = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // hpgq_dup_debug_set_timing: before, between and after the kernels
  bool timing = false, timed = false;
  hpgq::accum::Retired retired;            // buffers replaced or lent to a kernel
  // hpgq_dup_keep_sequences: keep_min == 0 is keeping off
  uint64_t keep_min = 0, arena_bytes = 0;
  unsigned long long *d_rep = nullptr;     // [2^log2] representative words, beside the slots
  unsigned char *d_arena = nullptr;        // [arena_bytes] {length, key} + bytes, every start 16-byte aligned
  bool touched = false;                    // counted or imported since open / reset
  bool keep_timed = false;
};

namespace {
using namespace hpgq::dup;

// wait for the stream, fetch the state words, free what was retired
int d_settle(hpgq_dup *d) {
  HPGQ_HIP_TRY(hipMemcpyAsync(d->h_state, d->d_state, kStateWords * 8, hipMemcpyDeviceToHost, d->stream));
  HPGQ_HIP_TRY(hipStreamSynchronize(d->stream));
  d->retired.free_all();
  d->bound = d->h_state[kOccupied];
  return d->h_state[kError] & kErrFull ? HPGQ_E_STATE : HPGQ_OK;
}

unsigned grid_for(const hpgq_dup *d, uint64_t items, int per_wg) {
  const uint64_t g = std::min<uint64_t>(8 * (uint64_t)std::max(1, d->cus), (items + per_wg - 1) / per_wg);
  return (unsigned)std::max<int64_t>(hpgq::accum::capped((int64_t)g, d->max_wg), 1);
}

// agg: the keys may repeat (fingerprints of reads), see insert_kernel
int d_insert(hpgq_dup *d, const u64 *keys, const u64 *counts, int64_t n, int stride, bool agg) {
  const dim3 grid(grid_for(d, (uint64_t)n, kWG));
  const u64 capmask = ((u64)1 << d->log2) - 1;
  if (agg)
    hipLaunchKernelGGL(insert_kernel<true>, grid, dim3(kWG), 0, d->stream, keys, counts, n, stride, d->d_tab, capmask,
                       d->d_state);
  else
    hipLaunchKernelGGL(insert_kernel<false>, grid, dim3(kWG), 0, d->stream, keys, counts, n, stride, d->d_tab, capmask,
                       d->d_state);
  HPGQ_HIP_TRY(hipGetLastError());
  return HPGQ_OK;
}

// Room for `incoming` more keys at a load of at most 1/2.  Synchronises only
// when the bound says the table may be too small; grows it only when the
// device's own count says so.  HPGQ_E_NOMEM: nothing changed.
int d_room(hpgq_dup *d, uint64_t incoming) {
  if (d->bound + incoming > ((uint64_t)1 << d->log2) / 2) {
    const int rc = d_settle(d);
    if (rc && rc != HPGQ_E_STATE) return rc;
  }
  if (d->bound + incoming > ((uint64_t)1 << d->log2) / 2) {
    int k = d->log2;
    while (k <= d->log2_max && d->bound + incoming > ((uint64_t)1 << k) / 2) ++k;
    if (k > d->log2_max) return HPGQ_E_NOMEM;
    unsigned long long *nt = nullptr;
    if (hipMalloc(&nt, (size_t)16 << k) != hipSuccess) {
      (void)hipGetLastError();
      return HPGQ_E_NOMEM;
    }
    unsigned long long *nr = nullptr;   // keeping mode: the representative words move with their keys
    if (d->keep_min && hipMalloc(&nr, (size_t)8 << k) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(nt);
      return HPGQ_E_NOMEM;
    }
    if (hipMemsetAsync(nt, 0, (size_t)16 << k, d->stream) != hipSuccess ||
        (nr && hipMemsetAsync(nr, 0, (size_t)8 << k, d->stream) != hipSuccess) ||
        hipMemsetAsync(d->d_state + kOccupied, 0, 8, d->stream) != hipSuccess) {
      (void)hipStreamSynchronize(d->stream);
      (void)hipFree(nt);
      (void)hipFree(nr);
      return HPGQ_E_HIP;
    }
    unsigned long long *old = d->d_tab, *old_rep = d->d_rep;
    const int64_t old_cap = (int64_t)1 << d->log2;
    d->d_tab = nt;
    d->d_rep = nr;
    d->log2 = k;
    d->retired.add(old);   // the rehash below reads it
    if (old_rep) d->retired.add(old_rep);
    ++d->rehashes;
    const int rc = d_insert(d, old, old + 1, old_cap, 2, false);   // (its claims count the occupied slots again)
    if (rc) return rc;
    if (nr) {
      hipLaunchKernelGGL(carry_kernel, dim3(grid_for(d, (uint64_t)old_cap, kWG)), dim3(kWG), 0, d->stream, old, old_rep,
                         (u64)old_cap, nt, nr, ((u64)1 << k) - 1, d->d_state);
      HPGQ_HIP_TRY(hipGetLastError());
    }
  }
  d->bound += incoming;
  return HPGQ_OK;
}

int d_fp_room(hpgq_dup *d, int64_t n) {
  if (n <= d->fp_cap) return HPGQ_OK;
  unsigned long long *p = nullptr;
  if (hipMalloc(&p, (size_t)n * 8) != hipSuccess) {
    (void)hipGetLastError();
    return HPGQ_E_NOMEM;
  }
  if (d->d_fp) d->retired.add(d->d_fp);   // (a kernel in flight may still read it)
  d->d_fp = p;
  d->fp_cap = n;
  return HPGQ_OK;
}

int d_fingerprints(hpgq_dup *d, const char *seq, const int32_t *ix, int64_t n, const uint8_t *mk) {
  const unsigned grid = grid_for(d, (uint64_t)n, kGroup);
  if (mk)
    hipLaunchKernelGGL(fp_kernel<true>, dim3(grid), dim3(kWG), 0, d->stream, seq, ix, n, mk, d->d_fp);
  else
    hipLaunchKernelGGL(fp_kernel<false>, dim3(grid), dim3(kWG), 0, d->stream, seq, ix, n, mk, d->d_fp);
  HPGQ_HIP_TRY(hipGetLastError());
  return HPGQ_OK;
}

// keeping mode: the part's reads whose key has reached keep_min and has no representative yet
int d_keep(hpgq_dup *d, const char *seq, const int32_t *ix, int64_t n) {
  hipLaunchKernelGGL(keep_kernel, dim3(grid_for(d, (uint64_t)n, kWG)), dim3(kWG), 0, d->stream, seq, ix, n, d->d_fp, d->d_tab,
                     d->d_rep, ((u64)1 << d->log2) - 1, (u64)d->keep_min, d->d_arena, (u64)d->arena_bytes, d->d_state);
  HPGQ_HIP_TRY(hipGetLastError());
  return HPGQ_OK;
}

// keeping off: the arena and the representative words freed (the stream is idle)
void d_keep_free(hpgq_dup *d) {
  (void)hipFree(d->d_rep);
  (void)hipFree(d->d_arena);
  d->d_rep = nullptr;
  d->d_arena = nullptr;
  d->keep_min = d->arena_bytes = 0;
  d->keep_timed = false;
}

constexpr int64_t kPart = (int64_t)1 << 26;   // reads per launch (32-bit offsets into idx; 512 MB of fingerprints)
}  // namespace

extern "C" {

int hpgq_dup_open(hpgq_dup_t **dp, int device, int log2_slots, int log2_max_slots, void *stream) {
  if (!dp || log2_slots < 4 || log2_max_slots < log2_slots || log2_max_slots > 34) return HPGQ_E_INVALID;
  *dp = nullptr;
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_dup *d = new hpgq_dup;
  d->device = device;
  d->log2 = log2_slots;
  d->log2_max = log2_max_slots;
  if ((rc = d->stream.open(stream)) != HPGQ_OK) {
    delete d;
    return rc;
  }
  const size_t hs = (size_t)(kStateWords + kLevelWords) * 8;
  if (hipMalloc(&d->d_tab, (size_t)16 << log2_slots) != hipSuccess || hipMalloc(&d->d_state, kStateWords * 8) != hipSuccess ||
      hipMalloc(&d->d_res, kLevelWords * 8) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void **>(&d->h_state), hs, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    hpgq_dup_close(d);
    return HPGQ_E_NOMEM;
  }
  for (int i = 0; i < kStateWords + kLevelWords; ++i) d->h_state[i] = 0;
  if (hipMemsetAsync(d->d_tab, 0, (size_t)16 << log2_slots, d->stream) != hipSuccess ||
      hipMemsetAsync(d->d_state, 0, kStateWords * 8, d->stream) != hipSuccess ||
      hipDeviceGetAttribute(&d->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
    hpgq_dup_close(d);
    return HPGQ_E_HIP;
  }
  *dp = d;
  return HPGQ_OK;
}

void hpgq_dup_close(hpgq_dup_t *d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  d->retired.free_all();
  (void)hipFree(d->d_tab);
  (void)hipFree(d->d_state);
  (void)hipFree(d->d_res);
  (void)hipFree(d->d_fp);
  (void)hipFree(d->d_rep);
  (void)hipFree(d->d_arena);
  if (d->h_state) (void)hipHostFree(d->h_state);
  for (hipEvent_t e : d->ev)
    if (e) (void)hipEventDestroy(e);
  d->stream.close();
  delete d;
}

int hpgq_dup_reset(hpgq_dup_t *d) {
  if (!d) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  HPGQ_HIP_TRY(hipMemsetAsync(d->d_tab, 0, (size_t)16 << d->log2, d->stream));
  HPGQ_HIP_TRY(hipMemsetAsync(d->d_state, 0, kStateWords * 8, d->stream));
  if (d->d_rep) HPGQ_HIP_TRY(hipMemsetAsync(d->d_rep, 0, (size_t)8 << d->log2, d->stream));   // (the arena's cursor is a state word)
  d->bound = 0;
  d->touched = false;
  return HPGQ_OK;
}

int hpgq_dup_count_device(hpgq_dup_t *d, const hpgq_batch_t *b, const uint8_t *mask) {
  if (!d || !b || b->num_reads < 0) return HPGQ_E_INVALID;
  if (b->num_reads == 0) return HPGQ_OK;
  if (!b->seq || !b->data_indices) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  d->touched = true;
  int rc = d_fp_room(d, std::min(kPart, b->num_reads));
  if (rc == 0) rc = d_room(d, (uint64_t)b->num_reads);   // (the whole batch or nothing)
  for (int64_t lo = 0; lo < b->num_reads && rc == 0; lo += kPart) {
    const int64_t n = std::min(kPart, b->num_reads - lo);
    if (d->timing) HPGQ_HIP_TRY(hipEventRecord(d->ev[0], d->stream));
    rc = d_fingerprints(d, b->seq, b->data_indices + lo, n, mask ? mask + lo : nullptr);
    if (d->timing) HPGQ_HIP_TRY(hipEventRecord(d->ev[1], d->stream));
    if (rc == 0) rc = d_insert(d, d->d_fp, nullptr, n, 1, true);
    if (d->timing) HPGQ_HIP_TRY(hipEventRecord(d->ev[2], d->stream));
    d->timed = d->timing && rc == 0;
    if (d->keep_min) {   // (d_fp is the next part's too: once per part)
      if (rc == 0) rc = d_keep(d, b->seq, b->data_indices + lo, n);
      if (d->timing) HPGQ_HIP_TRY(hipEventRecord(d->ev[3], d->stream));
      d->keep_timed = d->timed;
    }
  }
  return rc;
}

int hpgq_dup_sync(hpgq_dup_t *d) {
  if (!d) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  const int rc = d_settle(d);
  return rc == 0 && (d->h_state[kError] & kErrArena) ? HPGQ_E_NOMEM : rc;
}

int hpgq_dup_levels(hpgq_dup_t *d, hpgq_dup_levels_t *out) {
  if (!d || !out) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  const u64 cap = (u64)1 << d->log2;
  HPGQ_HIP_TRY(hipMemsetAsync(d->d_res, 0, kLevelWords * 8, d->stream));
  hipLaunchKernelGGL(levels_kernel, dim3(grid_for(d, cap, kWG)), dim3(kWG), 0, d->stream, d->d_tab, cap, d->d_res);
  HPGQ_HIP_TRY(hipGetLastError());
  unsigned long long *h = d->h_state + kStateWords;
  HPGQ_HIP_TRY(hipMemcpyAsync(h, d->d_res, kLevelWords * 8, hipMemcpyDeviceToHost, d->stream));
  const int rc = d_settle(d);
  if (rc) return rc;
  *out = hpgq_dup_levels_t{};
  for (int i = 0; i < HPGQ_DUP_LEVELS; ++i) {
    out->distinct_at[i] = h[i];
    out->reads_at[i] = h[HPGQ_DUP_LEVELS + i];
    out->distinct += h[i];
    out->reads += h[HPGQ_DUP_LEVELS + i];
  }
  out->max_count = h[kMax];
  return HPGQ_OK;
}

int hpgq_dup_export(hpgq_dup_t *d, uint64_t *keys, uint64_t *counts, size_t cap, size_t *n) {
  if (!d || !n) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  const int rc = d_settle(d);
  if (rc) return rc;
  const size_t occ = (size_t)d->h_state[kOccupied];
  *n = occ;
  if (!keys || !counts) return HPGQ_OK;
  if (cap < occ) return HPGQ_E_INVALID;
  if (!occ) return HPGQ_OK;
  unsigned long long *dk = nullptr;
  if (hipMalloc(&dk, occ * 16) != hipSuccess) {
    (void)hipGetLastError();
    return HPGQ_E_NOMEM;
  }
  const u64 slots = (u64)1 << d->log2;
  hipError_t e = hipMemsetAsync(d->d_state + kCursor, 0, 8, d->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(export_kernel, dim3(grid_for(d, slots, kWG)), dim3(kWG), 0, d->stream, d->d_tab, slots, dk, dk + occ,
                       (u64)occ, d->d_state);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
  if (e == hipSuccess) e = hipMemcpy(keys, dk, occ * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(counts, dk + occ, occ * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) (void)hipStreamSynchronize(d->stream);
  (void)hipFree(dk);
  HPGQ_HIP_TRY(e);
  return HPGQ_OK;
}

int hpgq_dup_import(hpgq_dup_t *d, const uint64_t *keys, const uint64_t *counts, size_t n) {
  if (!d || n > ((size_t)1 << 34)) return HPGQ_E_INVALID;
  if (n == 0) return HPGQ_OK;
  if (!keys || !counts) return HPGQ_E_INVALID;
  for (size_t i = 0; i < n; ++i)
    if (!keys[i] || !counts[i]) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  d->touched = true;
  int rc = d_room(d, (uint64_t)n);
  if (rc) return rc;
  unsigned long long *dk = nullptr;
  if (hipMalloc(&dk, n * 16) != hipSuccess) {
    (void)hipGetLastError();
    d->bound -= n;
    return HPGQ_E_NOMEM;
  }
  // (blocking copies: the pairs are on the device when they return, whatever the stream is doing)
  hipError_t e = hipMemcpy(dk, keys, n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dk + n, counts, n * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dk);
    d->bound -= n;
    HPGQ_HIP_TRY(e);
  }
  d->retired.add(dk);   // the kernel reads it
  return d_insert(d, dk, dk + n, (int64_t)n, 1, false);
}

int hpgq_dup_debug_set_max_workgroups(hpgq_dup_t *d, int max_wg) {
  if (!d || max_wg < 0) return HPGQ_E_INVALID;
  d->max_wg = max_wg;
  return HPGQ_OK;
}

int hpgq_dup_debug_set_timing(hpgq_dup_t *d, int on) {
  if (!d) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  for (hipEvent_t &e : d->ev)
    if (on && !e) HPGQ_HIP_TRY(hipEventCreate(&e));
  d->timing = on != 0;
  d->timed = d->keep_timed = false;
  return HPGQ_OK;
}

int hpgq_dup_debug_last_times(hpgq_dup_t *d, float *fp_us, float *insert_us) {
  if (!d || !fp_us || !insert_us) return HPGQ_E_INVALID;
  if (!d->timed) return HPGQ_E_STATE;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  HPGQ_HIP_TRY(hipEventSynchronize(d->ev[2]));
  float a = 0, b = 0;
  HPGQ_HIP_TRY(hipEventElapsedTime(&a, d->ev[0], d->ev[1]));
  HPGQ_HIP_TRY(hipEventElapsedTime(&b, d->ev[1], d->ev[2]));
  *fp_us = a * 1e3f;
  *insert_us = b * 1e3f;
  return HPGQ_OK;
}

int hpgq_dup_debug_info(hpgq_dup_t *d, int *log2_slots, int64_t *rehashes) {
  if (!d || !log2_slots || !rehashes) return HPGQ_E_INVALID;
  *log2_slots = d->log2;
  *rehashes = d->rehashes;
  return HPGQ_OK;
}

int hpgq_dup_debug_fingerprints(hpgq_dup_t *d, const hpgq_batch_t *b, uint64_t *out_host) {
  if (!d || !b || b->num_reads < 0 || b->num_reads > kPart) return HPGQ_E_INVALID;
  if (b->num_reads == 0) return HPGQ_OK;
  if (!b->seq || !b->data_indices || !out_host) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  int rc = d_fp_room(d, b->num_reads);
  if (rc == 0) rc = d_fingerprints(d, b->seq, b->data_indices, b->num_reads, nullptr);
  if (rc) return rc;
  HPGQ_HIP_TRY(hipStreamSynchronize(d->stream));
  HPGQ_HIP_TRY(hipMemcpy(out_host, d->d_fp, (size_t)b->num_reads * 8, hipMemcpyDeviceToHost));
  return HPGQ_OK;
}

int hpgq_dup_keep_sequences(hpgq_dup_t *d, uint64_t min_count, uint64_t arena_bytes) {
  if (!d || (min_count && (arena_bytes < 1 || arena_bytes > ((uint64_t)1 << 40)))) return HPGQ_E_INVALID;
  if (d->touched) return HPGQ_E_STATE;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  HPGQ_HIP_TRY(hipStreamSynchronize(d->stream));   // (open's or reset's memsets: nothing else is in flight)
  d_keep_free(d);
  if (!min_count) return HPGQ_OK;
  // (rounded up to 16 bytes for the last 16-byte store; the budget the kernel checks is arena_bytes)
  if (hipMalloc(&d->d_rep, (size_t)8 << d->log2) != hipSuccess ||
      hipMalloc(&d->d_arena, (size_t)((arena_bytes + 15) & ~(uint64_t)15)) != hipSuccess) {
    (void)hipGetLastError();
    d_keep_free(d);
    return HPGQ_E_NOMEM;
  }
  if (hipMemsetAsync(d->d_rep, 0, (size_t)8 << d->log2, d->stream) != hipSuccess ||
      hipMemsetAsync(d->d_state + kArena, 0, 3 * 8, d->stream) != hipSuccess) {   // kArena, kKeptSeqs, kKeptBytes
    (void)hipStreamSynchronize(d->stream);
    d_keep_free(d);
    return HPGQ_E_HIP;
  }
  d->keep_min = min_count;
  d->arena_bytes = arena_bytes;
  return HPGQ_OK;
}

int hpgq_dup_top(hpgq_dup_t *d, uint64_t min_count, uint64_t *keys, uint64_t *counts, size_t cap, size_t *total) {
  if (!d || !total || min_count < 1 || (keys && !counts)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  const u64 slots = (u64)1 << d->log2;
  const dim3 grid(grid_for(d, slots, kWG));
  // first pass: how many qualify
  HPGQ_HIP_TRY(hipMemsetAsync(d->d_state + kCursor, 0, 8, d->stream));
  hipLaunchKernelGGL(select_kernel, grid, dim3(kWG), 0, d->stream, d->d_tab, slots, (u64)min_count, (u64 *)nullptr,
                     (u64 *)nullptr, (u64)0, d->d_state);
  HPGQ_HIP_TRY(hipGetLastError());
  const int rc = d_settle(d);
  if (rc) return rc;
  const size_t hits = (size_t)d->h_state[kCursor];
  *total = hits;
  if (!keys || !hits || !cap) return HPGQ_OK;
  // second pass: the candidates alone to the host, sorted there
  unsigned long long *dk = nullptr;
  if (hipMalloc(&dk, hits * 16) != hipSuccess) {
    (void)hipGetLastError();
    return HPGQ_E_NOMEM;
  }
  std::vector<uint64_t> hk, hc;
  try {
    hk.resize(hits);
    hc.resize(hits);
  } catch (...) {
    (void)hipFree(dk);
    return HPGQ_E_NOMEM;
  }
  hipError_t e = hipMemsetAsync(d->d_state + kCursor, 0, 8, d->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(select_kernel, grid, dim3(kWG), 0, d->stream, d->d_tab, slots, (u64)min_count, dk, dk + hits,
                       (u64)hits, d->d_state);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
  if (e == hipSuccess) e = hipMemcpy(hk.data(), dk, hits * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(hc.data(), dk + hits, hits * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) (void)hipStreamSynchronize(d->stream);
  (void)hipFree(dk);
  HPGQ_HIP_TRY(e);
  size_t again = 0;
  return hpgq_dup_top_of(hk.data(), hc.data(), hits, min_count, keys, counts, cap, &again);
}

int hpgq_dup_sequence(hpgq_dup_t *d, uint64_t key, void *buf, size_t cap, int64_t *len) {
  if (!d || !len) return HPGQ_E_INVALID;
  if (!d->keep_min) return HPGQ_E_STATE;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  *len = -1;
  hipLaunchKernelGGL(find_kernel, dim3(1), dim3(1), 0, d->stream, d->d_tab, d->d_rep, ((u64)1 << d->log2) - 1, (u64)key,
                     d->d_state);
  HPGQ_HIP_TRY(hipGetLastError());
  const int rc = d_settle(d);
  if (rc) return rc;
  if (d->h_state[kError] & kErrArena) return HPGQ_E_NOMEM;
  const uint64_t r = d->h_state[kFound];
  if (r < kRepFirst) return HPGQ_OK;
  const unsigned char *at = d->d_arena + (r - kRepFirst) * 16;
  uint64_t head[2] = {0, 0};
  HPGQ_HIP_TRY(hipMemcpy(head, at, sizeof(head), hipMemcpyDeviceToHost));
  *len = (int64_t)head[0];
  if (!buf) return HPGQ_OK;
  if (cap < head[0]) return HPGQ_E_INVALID;
  if (head[0]) HPGQ_HIP_TRY(hipMemcpy(buf, at + kRepHeader, (size_t)head[0], hipMemcpyDeviceToHost));
  return HPGQ_OK;
}

int hpgq_dup_debug_kept(hpgq_dup_t *d, uint64_t *sequences, uint64_t *bytes) {
  if (!d || !sequences || !bytes) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  const int rc = d_settle(d);
  if (rc) return rc;
  *sequences = d->h_state[kKeptSeqs];
  *bytes = d->h_state[kKeptBytes];
  return HPGQ_OK;
}

int hpgq_dup_debug_last_keep_time(hpgq_dup_t *d, float *keep_us) {
  if (!d || !keep_us) return HPGQ_E_INVALID;
  if (!d->keep_timed) return HPGQ_E_STATE;
  HPGQ_HIP_TRY(hipSetDevice(d->device));
  HPGQ_HIP_TRY(hipEventSynchronize(d->ev[3]));
  float a = 0;
  HPGQ_HIP_TRY(hipEventElapsedTime(&a, d->ev[2], d->ev[3]));
  *keep_us = a * 1e3f;
  return HPGQ_OK;
}

}  // extern "C"
