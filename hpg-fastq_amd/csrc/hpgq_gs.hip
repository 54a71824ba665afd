// hpgq_gs.hip — genomic signature of FASTA text on the device.
//
// The rule is build-defined (the reference's generator is absent; what is left
// of it is lut_table_init, old/chaos_game.c:51-72): headers ('>' .. '\n') are
// dropped and break the word, N/n breaks the word, A/C/G/T in either case are
// bases, every other byte is skipped without breaking the word.  Each window
// of k consecutive kept bases adds 1 to table[co_x][co_y], bit i of co_x / co_y
// being dx / dy of the window's i-th oldest base (the (int)f cell of
// old/chaos_game.c:201-251 while the double state does not saturate).
//
//   gs_pack_kernel    reads the text once, 4 x 16 B per lane, and classifies four
//                     bytes at a time (SWAR); one chained scan over 16 KB tiles
//                     (per-tile {header state, kept count} functions, decoupled
//                     look-back) gives every kept byte its place in a compacted
//                     code stream: 0..3 = dx | dy << 1, 4 = break (one per N,
//                     one per header).  Also bases / Ns / sequences.
//   gs_count_kernel   16 codes per lane + the 16 before them: every window of
//                     k base codes is a word.  k <= 7: LDS table of u32 cells,
//                     flushed once per workgroup; k >= 8: global u32 adds.
//   gs_carry_kernel   the stream's last 16 codes become the next call's prefix
//                     and the header flag is stored, so a text may be cut at
//                     any byte and no call waits for the GPU.
#include "hpgq_accum.h"

#include <cstring>

namespace hpgq {
namespace gs {

constexpr int kTB = 256;            // threads of a pack workgroup
constexpr int kPer = 4;             // 16-byte loads per lane and tile
constexpr int kTile = kTB * 16 * kPer;   // text bytes per tile
constexpr int kPrefix = 16;         // carried codes in front of the packed stream (>= k - 1)
constexpr int kCountTB = 1024;      // threads of a count workgroup
constexpr uint32_t kBreak = 4;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// everything a call carries to the next one, and the counts
struct State {
  unsigned long long words, bases, ns, sequences;
  uint32_t in_header;
  uint32_t pad;
};

// A piece of text is a function of the header flag at its start:
// s -> (flag at its end, bytes it keeps).  Packed: bit 0 / 1 = end flag for
// s = 0 / 1, bits 2..16 / 17..31 = kept count for s = 0 / 1 (<= kTile).
constexpr uint32_t kFnId = 2u;
static_assert(kTile <= 0x7FFF, "a tile's kept count must fit 15 bits");
__device__ __forceinline__ uint32_t fn_make(uint32_t e0, uint32_t e1, uint32_t c0, uint32_t c1) {
  return e0 | (e1 << 1) | (c0 << 2) | (c1 << 17);
}
__device__ __forceinline__ uint32_t fn_end(uint32_t f, uint32_t s) { return (f >> s) & 1u; }
__device__ __forceinline__ uint32_t fn_cnt(uint32_t f, uint32_t s) { return (f >> (2u + 15u * s)) & 0x7FFFu; }
// f first, then g
__device__ __forceinline__ uint32_t fn_then(uint32_t f, uint32_t g) {
  const uint32_t e0 = fn_end(f, 0), e1 = fn_end(f, 1);
  return fn_make(fn_end(g, e0), fn_end(g, e1), fn_cnt(f, 0) + fn_cnt(g, e0), fn_cnt(f, 1) + fn_cnt(g, e1));
}

// the same over many tiles: counts too large for the packed form
struct Fn {
  uint32_t e, c0, c1;   // e: bit s = end flag for start flag s
};
__device__ __forceinline__ Fn fn_then_wide(Fn f, Fn g) {
  const uint32_t x0 = f.e & 1u, x1 = (f.e >> 1) & 1u;
  return Fn{((g.e >> x0) & 1u) | (((g.e >> x1) & 1u) << 1), f.c0 + (x0 ? g.c1 : g.c0), f.c1 + (x1 ? g.c1 : g.c0)};
}

// tile descriptor, one naturally aligned 8-byte word written by one store:
// bits 0..1 status, then  AGG: the tile's function << 2
//                         INC: end flag << 2 | kept bytes up to and including the tile << 32
constexpr uint64_t kAgg = 1, kInc = 2;
__device__ __forceinline__ void desc_store(uint64_t *d, uint64_t v) {
  __hip_atomic_store(d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t desc_load(const uint64_t *d) {
  return __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 0x80 in every byte of x that equals the byte of k4 (exact: no carry leaves a byte)
__device__ __forceinline__ uint32_t eq80(uint32_t x, uint32_t k4) {
  const uint32_t v = x ^ k4;
  return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}
// the 0x80 flags of four bytes -> bits 0..3
__device__ __forceinline__ uint32_t gather4(uint32_t f) {
  uint32_t x = f >> 7;
  x |= x >> 7;
  x |= x >> 14;
  return x & 0xFu;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// text: the 16-byte aligned address at or below the first byte; the bytes of
// the call are [lead, nv) of it.  ticket: the next tile to hand out; desc: one
// word per tile, both zeroed before the launch.  Tiles are handed out in
// order, so every tile a workgroup waits for is held by a running workgroup.
__global__ void __launch_bounds__(kTB) gs_pack_kernel(const uint8_t *text, uint32_t lead, int64_t nv,
                                                      uint32_t ntiles, uint32_t *ticket, uint64_t *desc,
                                                      uint8_t *packed, State *st) {
  __shared__ uint32_t s_tile, s_s0, s_c0, s_agg;
  __shared__ uint32_t s_wave[kTB / 64];
  __shared__ uint32_t s_stage[kTile / 4 + 2];
  uint8_t *stage = reinterpret_cast<uint8_t *>(s_stage);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n_bases = 0, n_ns = 0, n_seqs = 0;

  for (;;) {
    if (tid == 0) s_tile = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t tile = s_tile;
    if (tile >= ntiles) break;

    // 1. this lane's kPer x 16 bytes -> per 16: masks (bit i = byte i)
    //    and the 16 codes
    const int64_t v0 = (int64_t)tile * kTile + (int64_t)tid * (16 * kPer);
    uint32_t gt[kPer], bm[kPer], nm[kPer], h0[kPer], h1[kPer], fc[kPer];
    uint64_t cdl[kPer], cdh[kPer];   // the 16 codes, one byte each
    uint32_t mine = kFnId;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int64_t v = v0 + 16 * q;
      uint32_t g_ = 0, nl = 0, b_ = 0, n_ = 0;
      uint32_t cd[4] = {0u, 0u, 0u, 0u};
      if (v < nv) {
        const u32x4 w4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(text + v));
        const uint32_t ww[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // four bytes at a time
          const uint32_t w = ww[j], u = w | 0x20202020u;
          const uint32_t fb = eq80(u, 0x61616161u) | eq80(u, 0x63636363u) | eq80(u, 0x67676767u) |
                              eq80(u, 0x74747474u);
          const uint32_t fn = eq80(u, 0x6E6E6E6Eu), fg = eq80(w, 0x3E3E3E3Eu), fl = eq80(w, 0x0A0A0A0Au);
          b_ |= gather4(fb) << (4 * j);
          n_ |= gather4(fn) << (4 * j);
          g_ |= gather4(fg) << (4 * j);
          nl |= gather4(fl) << (4 * j);
          // bits 1..2 of A / C / G / T are 0 1 3 2 in either case: ^ 1 gives dx | dy << 1
          const uint32_t brk = (fn | fg) >> 7;   // 0x01 per byte that ends the word
          cd[j] = ((((w >> 1) & 0x03030303u) ^ 0x01010101u) & ~((brk << 8) - brk)) | (brk << 2);
        }
        // bytes of the aligned 16 that lie outside the call's text are skipped
        const int64_t lo = (int64_t)lead - v, hi = nv - v;
        const uint32_t valid = (hi >= 16 ? 0xFFFFu : ((1u << (uint32_t)hi) - 1u)) &
                               ~(lo > 0 ? ((1u << (uint32_t)(lo > 16 ? 16 : lo)) - 1u) : 0u);
        g_ &= valid;
        nl &= valid;
        b_ &= valid;
        n_ &= valid;
      }
      const uint32_t kc = b_ | n_ | g_;   // kept when outside a header
      const uint32_t anym = g_ | nl;
      // header mask for a start outside a header (m0) and inside one (m1).  m0: from the
      // byte after each '>' through the next marker; the add carries through the bytes between
      const uint32_t fr = ~anym & 0xFFFFu, af = (g_ << 1) & 0xFFFFu;
      const uint32_t m0 = ((((af & fr) + fr) ^ fr) | af) & 0xFFFFu;
      const uint32_t m1 = m0 | (anym ? ((2u << __builtin_ctz(anym)) - 1u) : 0xFFFFu);
      const uint32_t last = anym ? ((g_ >> (31 - __builtin_clz(anym))) & 1u) : 0u;
      gt[q] = g_;
      bm[q] = b_;
      nm[q] = n_;
      cdl[q] = (uint64_t)cd[0] | ((uint64_t)cd[1] << 32);
      cdh[q] = (uint64_t)cd[2] | ((uint64_t)cd[3] << 32);
      h0[q] = m0;
      h1[q] = m1;
      fc[q] = fn_make(anym ? last : 0u, anym ? last : 1u, __builtin_popcount(kc & ~m0),
                      __builtin_popcount(kc & ~m1));
      mine = fn_then(mine, fc[q]);
    }

    // 2. scan of the functions over the workgroup
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= (uint32_t)d) incl = fn_then(up, incl);
    }
    uint32_t excl = __shfl_up(incl, 1);
    if (lane == 0) excl = kFnId;
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();

    // 3. the tile's start: header flag and kept bytes before it.  Wave 0 looks
    //    back 64 descriptors at a time: aggregates up to the nearest inclusive one.
    if (wave == 0) {
      uint32_t agg = s_wave[0];
#pragma unroll
      for (int i = 1; i < kTB / 64; ++i) agg = fn_then(agg, s_wave[i]);
      uint32_t s0 = 0, c0 = 0;
      if (tile == 0) {
        s0 = st->in_header & 1u;
      } else {
        if (lane == 0) desc_store(desc + tile, ((uint64_t)agg << 2) | kAgg);
        Fn f = {2u, 0u, 0u};   // the tiles between the window and this one
        for (int64_t base = (int64_t)tile - 1;; base -= 64) {
          const int64_t j = base - (int64_t)lane;   // this lane's tile
          uint64_t d, inc;
          for (;;) {
            d = j >= 0 ? desc_load(desc + j) : 3u;   // status 3: before the first tile
            const uint32_t status = (uint32_t)d & 3u;
            inc = __ballot(status == (uint32_t)kInc);
            const uint64_t wait = __ballot(status == 0u), past = __ballot(status == 3u);
            // ready: every lane nearer than the nearest inclusive one is published,
            // or all 64 are aggregates (tile 0 only ever publishes an inclusive one)
            if (inc ? (wait & ((inc & (0 - inc)) - 1u)) == 0 : (wait | past) == 0) break;
            __builtin_amdgcn_s_sleep(1);
          }
          const uint32_t m = inc ? (uint32_t)__builtin_ctzll(inc) : 64u;   // aggregates: lanes [0, m)
          Fn r = {2u, 0u, 0u};
          if (lane < m) {
            const uint32_t a = (uint32_t)(d >> 2);
            r = Fn{a & 3u, fn_cnt(a, 0), fn_cnt(a, 1)};
          }
          // lane 0 <- (lane 63) then ... then (lane 1) then (lane 0): tile order
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const Fn t = {(uint32_t)__shfl_down(r.e, o), (uint32_t)__shfl_down(r.c0, o),
                          (uint32_t)__shfl_down(r.c1, o)};
            if (lane + (uint32_t)o < 64u) r = fn_then_wide(t, r);
          }
          r = Fn{(uint32_t)__shfl(r.e, 0), (uint32_t)__shfl(r.c0, 0), (uint32_t)__shfl(r.c1, 0)};
          f = fn_then_wide(r, f);
          if (inc) {
            const uint32_t dlo = __shfl((uint32_t)d, (int)m), dhi = __shfl((uint32_t)(d >> 32), (int)m);
            const uint32_t sj = (dlo >> 2) & 1u;
            s0 = (f.e >> sj) & 1u;
            c0 = dhi + (sj ? f.c1 : f.c0);
            break;
          }
        }
      }
      if (lane == 0) {
        desc_store(desc + tile,
                   ((uint64_t)(c0 + fn_cnt(agg, s0)) << 32) | ((uint64_t)fn_end(agg, s0) << 2) | kInc);
        s_s0 = s0;
        s_c0 = c0;
        s_agg = agg;
      }
    }
    uint32_t before = kFnId;   // the waves before this thread's own
    for (uint32_t i = 0; i < wave; ++i) before = fn_then(before, s_wave[i]);
    __syncthreads();
    const uint32_t s0 = s_s0, c0 = s_c0, agg = s_agg;

    // 4. kept bytes -> LDS, at their place in the tile's part of the stream
    const uint32_t sh = c0 & 3u;   // the stream is stored in aligned dwords
    uint32_t pre = fn_then(before, excl);
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const uint32_t hm = fn_end(pre, s0) ? h1[q] : h0[q];
      uint32_t kept = (bm[q] | nm[q] | gt[q]) & ~hm;
      n_bases += __builtin_popcount(bm[q] & ~hm);
      n_ns += __builtin_popcount(nm[q] & ~hm);
      n_seqs += __builtin_popcount(gt[q] & ~hm);
      uint32_t o = sh + fn_cnt(pre, s0);
      while (kept) {
        const int i = __builtin_ctz(kept);
        kept &= kept - 1u;
        stage[o++] = (uint8_t)((((i & 8) ? cdh[q] : cdl[q]) >> ((i & 7) * 8)) & 7u);
      }
      pre = fn_then(pre, fc[q]);
    }
    __syncthreads();

    // 5. LDS -> stream: whole dwords, single bytes at the two ends (the
    //    neighbouring tiles own the rest of those dwords)
    const uint32_t span = sh + fn_cnt(agg, s0);
    uint8_t *out = packed + kPrefix + (size_t)(c0 - sh);
    for (uint32_t w = tid; w * 4u < span; w += kTB) {
      const uint32_t lo = w * 4u, hi = lo + 4u;
      if (lo >= sh && hi <= span) {
        reinterpret_cast<uint32_t *>(out)[w] = s_stage[w];
      } else {
        for (uint32_t b = lo; b < hi; ++b)
          if (b >= sh && b < span) out[b] = stage[b];
      }
    }
    __syncthreads();
  }

  const unsigned long long b = wave_sum(n_bases), n = wave_sum(n_ns), s = wave_sum(n_seqs);
  if (lane == 0) {
    if (b) atomicAdd(&st->bases, b);
    if (n) atomicAdd(&st->ns, n);
    if (s) atomicAdd(&st->sequences, s);
  }
}

// packed: [kPrefix carried codes | M codes]; M is in the last tile's descriptor.
// Lane chunk c owns codes [16 c, 16 c + 16) and reads the 16 before them.
template <bool kLds>
__global__ void __launch_bounds__(kCountTB) gs_count_kernel(const uint8_t *packed, const uint64_t *desc_last,
                                                            int k, uint32_t *table, State *st) {
  extern __shared__ uint32_t s_tab[];
  const uint32_t cells = 1u << (2 * k);
  if (kLds) {
    for (uint32_t i = threadIdx.x; i < cells; i += kCountTB) s_tab[i] = 0;
    __syncthreads();
  }
  const int64_t M = (int64_t)(*desc_last >> 32);
  const int64_t nchunks = (M + 15) / 16;
  const int hstart = 16 - (k - 1);
  const uint32_t top = (uint32_t)(k - 1);
  uint32_t words = 0;
  for (int64_t c = (int64_t)blockIdx.x * kCountTB + threadIdx.x; c < nchunks; c += (int64_t)gridDim.x * kCountTB) {
    const u32x4 pv = *reinterpret_cast<const u32x4 *>(packed + 16 * c);
    const u32x4 cv = *reinterpret_cast<const u32x4 *>(packed + 16 * c + kPrefix);
    const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w}, cw[4] = {cv.x, cv.y, cv.z, cv.w};
    uint32_t run = 0, cx = 0, cy = 0;
#pragma unroll
    for (int i = 1; i < 16; ++i) {   // the k - 1 codes before the chunk
      const uint32_t code = (pw[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
      if (i >= hstart) {
        if (code < kBreak) {
          run += 1;
          cx = (cx >> 1) | ((code & 1u) << top);
          cy = (cy >> 1) | ((code >> 1) << top);
        } else {
          run = 0;
        }
      }
    }
    const int64_t left = M - 16 * c;   // codes of the chunk that exist
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t code = (cw[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
      if (i < left) {
        if (code < kBreak) {
          run = run < (uint32_t)k ? run + 1 : run;
          cx = (cx >> 1) | ((code & 1u) << top);
          cy = (cy >> 1) | ((code >> 1) << top);
          if (run == (uint32_t)k) {
            const uint32_t cell = (cx << k) | cy;
            if (kLds)
              atomicAdd(&s_tab[cell], 1u);
            else
              atomicAdd(&table[cell], 1u);
            ++words;
          }
        } else {
          run = 0;
        }
      }
    }
  }
  const unsigned long long w = wave_sum(words);
  if ((threadIdx.x & 63u) == 0 && w) atomicAdd(&st->words, w);
  if (kLds) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cells; i += kCountTB) {
      const uint32_t v = s_tab[i];
      if (v) atomicAdd(&table[i], v);
    }
  }
}

// one wave: the last kPrefix codes of [prefix | M codes] become the prefix
__global__ void __launch_bounds__(64) gs_carry_kernel(uint8_t *packed, const uint64_t *desc_last, State *st) {
  const uint64_t d = *desc_last;
  const size_t M = (size_t)(d >> 32);
  uint8_t v = 0;
  if (threadIdx.x < kPrefix) v = packed[M + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < kPrefix) packed[threadIdx.x] = v;
  if (threadIdx.x == 0) st->in_header = (uint32_t)(d >> 2) & 1u;
}

}  // namespace gs
}  // namespace hpgq

struct hpgq_gs {
  int device = 0;
  int k = 0;
  int num_cus = 0;
  int max_wg = 0;              // hpgq_gs_debug_set_max_workgroups (0: no limit)
  hpgq::accum::Stream stream;
  uint32_t *d_table = nullptr;
  hpgq::gs::State *d_state = nullptr;
  uint8_t *d_packed = nullptr; // [kPrefix | codes]
  size_t packed_cap = 0;
  uint64_t *d_desc = nullptr;  // [ticket | one descriptor per tile]
  size_t desc_cap = 0;
  // hpgq_gs_add_host: two page-locked slots, one device copy of the piece
  static constexpr size_t kStage = (size_t)8 << 20;
  uint8_t *h_stage[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool ev_used[2] = {false, false};
  int slot = 0;
  uint8_t *d_text = nullptr;
};

static int gs_clear(hpgq_gs *g) {
  using namespace hpgq::gs;
  HPGQ_HIP_TRY(hipMemsetAsync(g->d_table, 0, ((size_t)4 << (2 * g->k)), g->stream));
  HPGQ_HIP_TRY(hipMemsetAsync(g->d_state, 0, sizeof(State), g->stream));
  HPGQ_HIP_TRY(hipMemsetAsync(g->d_packed, (int)kBreak, kPrefix, g->stream));
  return HPGQ_OK;
}

extern "C" {

int hpgq_gs_open(hpgq_gs_t **gs, int device, int k, void *stream) {
  using namespace hpgq::gs;
  if (!gs) return HPGQ_E_INVALID;
  *gs = nullptr;
  if (k < 1 || k > 12) return HPGQ_E_INVALID;
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_gs *g = new hpgq_gs();
  g->device = device;
  g->k = k;
  auto fail = [&](int code) {
    hpgq_gs_close(g);
    return code;
  };
  if (hipDeviceGetAttribute(&g->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      g->num_cus <= 0)
    return fail(HPGQ_E_HIP);
  if ((rc = g->stream.open(stream)) != HPGQ_OK) return fail(rc);
  g->packed_cap = kPrefix + 4096;
  if (hipMalloc(&g->d_table, (size_t)4 << (2 * k)) != hipSuccess ||
      hipMalloc(&g->d_state, sizeof(State)) != hipSuccess ||
      hipMalloc(&g->d_packed, g->packed_cap) != hipSuccess)
    return fail(HPGQ_E_NOMEM);
  if ((rc = gs_clear(g)) != HPGQ_OK) return fail(rc);
  *gs = g;
  return HPGQ_OK;
}

void hpgq_gs_close(hpgq_gs_t *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  (void)hipFree(g->d_table);
  (void)hipFree(g->d_state);
  (void)hipFree(g->d_packed);
  (void)hipFree(g->d_desc);
  (void)hipFree(g->d_text);
  for (int i = 0; i < 2; ++i) {
    if (g->h_stage[i]) (void)hipHostFree(g->h_stage[i]);
    if (g->ev[i]) (void)hipEventDestroy(g->ev[i]);
  }
  g->stream.close();
  delete g;
}

int hpgq_gs_add_device(hpgq_gs_t *g, const char *text_dev, int64_t n) {
  using namespace hpgq::gs;
  if (!g || n < 0 || n >= ((int64_t)1 << 31) || (!text_dev && n > 0)) return HPGQ_E_INVALID;
  if (n == 0) return HPGQ_OK;
  HPGQ_HIP_TRY(hipSetDevice(g->device));
  const uintptr_t addr = reinterpret_cast<uintptr_t>(text_dev);
  const uint32_t lead = (uint32_t)(addr & 15u);
  const int64_t nv = (int64_t)lead + n;
  const uint32_t ntiles = (uint32_t)((nv + kTile - 1) / kTile);
  // the stream holds at most n codes; the count kernel reads whole 16-byte chunks
  const size_t need = (size_t)kPrefix + (size_t)n + 64;
  if (need > g->packed_cap) {   // (the carried prefix moves to the larger buffer)
    const size_t cap = need + need / 4;
    uint8_t *p = nullptr;
    if (hipMalloc(&p, cap) != hipSuccess) return HPGQ_E_NOMEM;
    HPGQ_HIP_TRY(hipMemcpyAsync(p, g->d_packed, kPrefix, hipMemcpyDeviceToDevice, g->stream));
    HPGQ_HIP_TRY(hipStreamSynchronize(g->stream));
    (void)hipFree(g->d_packed);
    g->d_packed = p;
    g->packed_cap = cap;
  }
  const size_t dneed = ((size_t)ntiles + 1) * 8;
  if (dneed > g->desc_cap) {
    HPGQ_HIP_TRY(hipStreamSynchronize(g->stream));
    (void)hipFree(g->d_desc);
    g->d_desc = nullptr;
    g->desc_cap = 0;
    const size_t cap = dneed + dneed / 4 + 1024;
    if (hipMalloc(&g->d_desc, cap) != hipSuccess) return HPGQ_E_NOMEM;
    g->desc_cap = cap;
  }
  HPGQ_HIP_TRY(hipMemsetAsync(g->d_desc, 0, dneed, g->stream));
  uint32_t *ticket = reinterpret_cast<uint32_t *>(g->d_desc);
  uint64_t *desc = g->d_desc + 1;
  const uint64_t *last = desc + (ntiles - 1);

  int64_t pg = (int64_t)g->num_cus * 8;
  if (pg > (int64_t)ntiles) pg = ntiles;
  if (g->max_wg > 0 && pg > g->max_wg) pg = g->max_wg;
  gs_pack_kernel<<<(unsigned)pg, kTB, 0, g->stream>>>(reinterpret_cast<const uint8_t *>(addr - lead), lead, nv,
                                                      ntiles, ticket, desc, g->d_packed, g->d_state);
  HPGQ_HIP_TRY(hipGetLastError());

  const int64_t groups = ((n + 15) / 16 + kCountTB - 1) / kCountTB;   // chunks are at most ceil(n / 16)
  int64_t cg = (int64_t)g->num_cus * 2;
  if (cg > groups) cg = groups;
  if (g->max_wg > 0 && cg > g->max_wg) cg = g->max_wg;
  if (g->k <= 7)
    gs_count_kernel<true><<<(unsigned)cg, kCountTB, (size_t)4 << (2 * g->k), g->stream>>>(
        g->d_packed, last, g->k, g->d_table, g->d_state);
  else
    gs_count_kernel<false><<<(unsigned)cg, kCountTB, 0, g->stream>>>(g->d_packed, last, g->k, g->d_table,
                                                                      g->d_state);
  HPGQ_HIP_TRY(hipGetLastError());
  gs_carry_kernel<<<1, 64, 0, g->stream>>>(g->d_packed, last, g->d_state);
  HPGQ_HIP_TRY(hipGetLastError());
  return HPGQ_OK;
}

int hpgq_gs_add_host(hpgq_gs_t *g, const char *text, int64_t n) {
  if (!g || n < 0 || (!text && n > 0)) return HPGQ_E_INVALID;
  if (n == 0) return HPGQ_OK;
  HPGQ_HIP_TRY(hipSetDevice(g->device));
  if (!g->d_text) {
    for (int i = 0; i < 2; ++i) {
      if (!g->h_stage[i] && hipHostMalloc((void **)&g->h_stage[i], hpgq_gs::kStage, hipHostMallocDefault) != hipSuccess)
        return HPGQ_E_NOMEM;
      if (!g->ev[i]) HPGQ_HIP_TRY(hipEventCreateWithFlags(&g->ev[i], hipEventDisableTiming));
    }
    if (hipMalloc(&g->d_text, hpgq_gs::kStage + 16) != hipSuccess) return HPGQ_E_NOMEM;
  }
  // the state is carried on the device, so the text is cut wherever a slot ends
  for (int64_t off = 0; off < n;) {
    const size_t len = (size_t)((n - off) < (int64_t)hpgq_gs::kStage ? (n - off) : (int64_t)hpgq_gs::kStage);
    const int s = g->slot;
    g->slot ^= 1;
    if (g->ev_used[s]) HPGQ_HIP_TRY(hipEventSynchronize(g->ev[s]));   // the slot's last copy has left it
    std::memcpy(g->h_stage[s], text + off, len);
    HPGQ_HIP_TRY(hipMemcpyAsync(g->d_text, g->h_stage[s], len, hipMemcpyHostToDevice, g->stream));
    HPGQ_HIP_TRY(hipEventRecord(g->ev[s], g->stream));
    g->ev_used[s] = true;
    const int rc = hpgq_gs_add_device(g, reinterpret_cast<const char *>(g->d_text), (int64_t)len);
    if (rc) return rc;
    off += (int64_t)len;
  }
  return HPGQ_OK;
}

int hpgq_gs_sync(hpgq_gs_t *g) {
  if (!g) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(g->device));
  HPGQ_HIP_TRY(hipStreamSynchronize(g->stream));
  return HPGQ_OK;
}

int hpgq_gs_reset(hpgq_gs_t *g) {
  if (!g) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(g->device));
  return gs_clear(g);
}

int hpgq_gs_read(hpgq_gs_t *g, uint32_t *table, hpgq_gs_info_t *info) {
  if (!g || (!table && !info)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(g->device));
  hpgq::gs::State st;
  if (table)
    HPGQ_HIP_TRY(hipMemcpyAsync(table, g->d_table, (size_t)4 << (2 * g->k), hipMemcpyDeviceToHost, g->stream));
  HPGQ_HIP_TRY(hipMemcpyAsync(&st, g->d_state, sizeof(st), hipMemcpyDeviceToHost, g->stream));
  HPGQ_HIP_TRY(hipStreamSynchronize(g->stream));
  if (info) {
    info->words = st.words;
    info->bases = st.bases;
    info->ns = st.ns;
    info->sequences = st.sequences;
  }
  return HPGQ_OK;
}

int hpgq_gs_debug_set_max_workgroups(hpgq_gs_t *g, int max_wg) {
  if (!g || max_wg < 0) return HPGQ_E_INVALID;
  g->max_wg = max_wg;
  return HPGQ_OK;
}

}  // extern "C"
