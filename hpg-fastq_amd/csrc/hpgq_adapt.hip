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
// A step: lane l takes the read's bytes p0 + 4l .. p0 + 4l + 3 (one 8-byte
// dword-aligned load, hpgq_reads.h, and v_alignbyte), zeroes those past
// the read's end, and packs them, four bytes at once, into four 2-bit base
// codes ((b >> 1) & 3: A 0, C 1, T 2, G 3) and four validity bits: the byte is
// exactly the one base with its code.  2-bit codes alias (a, N and 250 other
// values share them), so a window matches only if the codes are equal AND its
// first K bases are all valid.  Bytes past the read's end -- the next read's
// bases, the slack -- are invalid, so no window reaches over it.
//
// Windows cross lanes.  Each lane builds the codes and validity bits of the
// bases of lanes l .. l + H by doubling with ds_bpermute (codes and validity
// packed into one word while they fit): H = 3 and two permutes give 16 bases in
// a 32-bit window for probes of up to 13 bases (NARROW: the default set); H = 8
// and five permutes give 36 bases in a 64 + 8 bit window for probes of up to 32
// (WIDE).  The last H lanes of a step only supply bases: a step covers the
// starts p0 .. p0 + S - 1, S = 4 (64 - H) = 244 or 224, and the next step
// starts at p0 + S, so no window needs the following step's bytes.  150 and
// 250 bp reads with the default set take one step.
//
// Prefilter: every probe has at least 8 bases, so the workgroup keeps a 65,536
// bit map of the set's 8-base prefixes (16 code bits) in LDS; a start is a
// candidate iff its next 8 bases are valid and their bit is set: one ds_read
// and a few VALU per start, and one ballot per step.  Almost every step of
// real data ends there (DESIGN.md 4.13 has both variants' times: without the
// bitmap the default set took 1.6 - 2 x as long on reads without adapters, 32
// probes 2.7 - 5 x).
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
#include "hpgq_reads.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace hpgq {
namespace adapt {

constexpr int kP = 256;     // positions whose counts stay on chip
constexpr int kMaxProbes = HPGQ_ADAPT_MAX_PROBES;
constexpr int kWG = 512;
constexpr int kWaves = kWG / 64;
constexpr int kR = 16;      // reads per wave step
constexpr int kPre = 4;     // of them with their first load in flight
constexpr int kGroup = kWaves * kR;   // reads per workgroup step
constexpr int kNarrowMax = 13;        // longest probe of the 32-bit window: 16 bases less the 3 a start may skip
using reads::v2u;
constexpr int kBitmapWords = 65536 / 32;   // one bit per 8-base prefix (16 code bits)
static_assert(kR % kPre == 0, "the reads of a wave step go in blocks of kPre");
static_assert(kMaxProbes == 32, "the found-mask is one 32-bit word");

// the probe set as the kernel takes it (by value: scalar loads)
struct Probes {
  uint64_t code[kMaxProbes];   // base j at bits 2j .. 2j + 1
  uint32_t len[kMaxProbes];
  int32_t n, kmin;
};

// the 2-bit code of an A C G T byte
__host__ __device__ inline uint32_t code_of(uint32_t b) { return (b >> 1) & 3u; }

__device__ __forceinline__ uint32_t pull(uint32_t v, int lane, int d) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(((lane + d) & 63) * 4, (int)v);
}

// One counted read of len <= rows bytes at st0 (from the descriptor's base);
// w0: its first step's load.  Everything but the lane's bytes is wave-uniform.
template <bool WIDE>
__device__ __forceinline__ uint32_t scan_read(const __amdgpu_buffer_rsrc_t rq, const Probes &pr, int lane, uint32_t st0,
                                              int len, v2u w0, uint32_t pc_lo, uint32_t pc_hi, uint32_t pk,
                                              uint32_t *t, const uint32_t *bm, unsigned long long *first) {
  constexpr int H = WIDE ? 8 : 3;          // lanes after its own a lane's windows reach into
  constexpr int S = 4 * (64 - H);          // starts per step
  const uint32_t all = pr.n == kMaxProbes ? 0xFFFFFFFFu : (1u << pr.n) - 1u;
  uint32_t found = 0;
  for (int p0 = 0; p0 + pr.kmin <= len; p0 += S) {
    const int rem = len - p0;
    const uint32_t st = st0 + (uint32_t)p0;
    const v2u w = p0 == 0 ? w0 : reads::lane_load8(rq, st, rem, lane);
    // positions p0 + 4 lane + [0, 4); the bytes past the read's end become 0, which is no base
    const int nb = rem - 4 * lane;
    const uint32_t raw = __builtin_amdgcn_alignbyte(w[1], w[0], st & 3u);
    const uint32_t v = nb >= 4 ? raw : nb <= 0 ? 0u : raw & ((1u << (8 * nb)) - 1u);
    // the four bytes at once: x the code of each byte, `want` the one byte with
    // that code that is a base (0x41 + 2 code, and T = 0x54 for code 2), z bit 7
    // of every byte that equals it (the zero-byte test of v ^ want)
    const uint32_t x = v >> 1 & 0x03030303u;
    const uint32_t isT = x >> 1 & ~x & 0x01010101u;
    const uint32_t d = v ^ (0x41414141u + 2u * x + 15u * isT);
    const uint32_t z = ~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
    const uint32_t c = (x | x >> 6 | x >> 12 | x >> 18) & 0xFFu;          // base j at bits 2j .. 2j + 1
    const uint32_t ok = (z >> 7 | z >> 14 | z >> 21 | z >> 28) & 0xFu;    // base j at bit j
    // 16 bases from lanes l .. l + 3: codes 32 bits, validity 16
    const uint32_t x1 = c | ok << 8;
    const uint32_t y1 = pull(x1, lane, 1);
    const uint32_t c2 = c | (y1 & 0xFFu) << 8, ok2 = ok | (y1 >> 8 & 0xFu) << 4;
    const uint32_t y2 = pull(c2 | ok2 << 16, lane, 2);
    const uint32_t c4 = c2 | y2 << 16, ok4 = ok2 | (y2 >> 16 & 0xFFu) << 8;
    uint64_t win[4];    // the bases from start k on (WIDE: 32 of them, else 16 - k)
    uint32_t val[4];    // their validity bits (WIDE: 32, else 16 - k)
    if (WIDE) {
      const uint64_t c8 = (uint64_t)c4 | (uint64_t)pull(c4, lane, 4) << 32;
      const uint32_t ok8 = ok4 | pull(ok4, lane, 4) << 16;
      const uint32_t y9 = pull(x1, lane, 8);
      const uint64_t c9 = y9 & 0xFFu;
      const uint32_t ok9 = y9 >> 8 & 0xFu;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        win[k] = k ? c8 >> (2 * k) | c9 << (64 - 2 * k) : c8;
        val[k] = k ? ok8 >> k | ok9 << (32 - k) : ok8;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        win[k] = c4 >> (2 * k);
        val[k] = ok4 >> k;
      }
    }
    // Prefilter: every probe has at least 8 bases, so a probe can start only
    // where the next 8 bases are valid (r8: ok4 folded three times) and their 16
    // code bits are the first 8 bases of some probe (one bit of bm).  Most
    // steps of real data end here.
    const bool starts = lane < 64 - H;   // the last H lanes only supply bases
    const uint32_t r2 = ok4 & ok4 >> 1, r4 = r2 & r2 >> 2, r8 = r4 & r4 >> 4;
    uint32_t cand = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t ix8 = (uint32_t)win[k] & 0xFFFFu;
      cand |= (bm[ix8 >> 5] >> (ix8 & 31u) & r8 >> k & 1u) << k;
    }
    if (!__ballot(starts && cand != 0)) continue;   // no probe starts in this step
    uint32_t run[4];    // valid bases from start k on, as far as the window goes
#pragma unroll
    for (int k = 0; k < 4; ++k) run[k] = (uint32_t)__builtin_ctzll(~(uint64_t)val[k]);   // (WIDE: 32 when all are valid)
    for (int a = 0; a < pr.n; ++a) {
      if (found >> a & 1u) continue;
      // probe a's length and code from lane a of pk / pc_lo / pc_hi (no scalar load in the loop)
      const uint32_t K = (uint32_t)__builtin_amdgcn_readlane((int)pk, a);
      const uint32_t code_lo = (uint32_t)__builtin_amdgcn_readlane((int)pc_lo, a);
      uint32_t m = 0;
      if (WIDE) {
        const uint64_t code = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)pc_hi, a) << 32 | code_lo;
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
  for (int i = threadIdx.x; i < kBitmapWords; i += kWG) bm[i] = 0;
  __syncthreads();
  if ((int)threadIdx.x < pr.n) {
    const uint32_t ix8 = (uint32_t)pr.code[threadIdx.x] & 0xFFFFu;
    atomicOr(&bm[ix8 >> 5], 1u << (ix8 & 31u));
  }
  __syncthreads();
  const reads::Batch rd = reads::open<MASK>(seq, idx, n, mask);
  const int64_t ngroups = (n + kGroup - 1) / kGroup;
  // lane a holds probe a: its code's halves and its length
  const int pa = lane < pr.n ? lane : 0;
  const uint32_t pc_lo = (uint32_t)pr.code[pa], pc_hi = (uint32_t)(pr.code[pa] >> 32), pk = pr.len[pa];
  // over this wave's counted reads (wave-uniform)
  int longest = 0;
  uint32_t clipped = 0, nreads = 0, nany = 0;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t rb = g * kGroup + wave * kR;
    if (rb >= n) continue;
    int32_t ix;
    uint32_t mk;
    reads::step_reads<kR, MASK>(rd, rb, n, lane, ix, mk);
    // read i of the step: its first byte from the descriptor's base, its
    // length, and whether it is scanned (counted, inside the rows, long enough)
    auto first_load = [&](int i) {
      const int32_t a = __builtin_amdgcn_readlane(ix, i);
      const int32_t len = __builtin_amdgcn_readlane(ix, i + 1) - a;
      const bool cnt = (uint32_t)__builtin_amdgcn_readlane((int)mk, i) == 1u;
      const bool scan = cnt && len <= rows && len >= pr.kmin;
      return reads::lane_load8(rd.bytes, (uint32_t)a + rd.shift, scan ? len : 0, lane);
    };
    v2u wq[kPre];
#pragma unroll
    for (int j = 0; j < kPre; ++j) wq[j] = first_load(j);
    for (int i0 = 0; i0 < kR; i0 += kPre) {
#pragma unroll
      for (int j = 0; j < kPre; ++j) {
        const int i = i0 + j;
        const int32_t a = __builtin_amdgcn_readlane(ix, i);
        const int32_t len = __builtin_amdgcn_readlane(ix, i + 1) - a;
        const bool cnt = (uint32_t)__builtin_amdgcn_readlane((int)mk, i) == 1u;
        const v2u w = wq[j];
        if (i0 + kPre < kR) wq[j] = first_load(i + kPre);
        if (!cnt) continue;   // (wave-uniform)
        ++nreads;
        longest = max(longest, len);
        if (len > rows) {
          ++clipped;
          continue;
        }
        if (scan_read<WIDE>(rd.bytes, pr, lane, (uint32_t)a + rd.shift, len, w, pc_lo, pc_hi, pk, t, bm, first)) ++nany;
      }
    }
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
  hpgq::adapt::Probes pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.n = nprobes;
  pr.kmin = HPGQ_ADAPT_MAX_LEN;
  int kmax = 0;
  for (int a = 0; a < nprobes; ++a) {
    if (hpgq_adapt_find(nullptr, 0, probes[a]) == -2) return HPGQ_E_INVALID;   // the probe rules
    const int k = (int)std::strlen(probes[a]);
    for (int j = 0; j < k; ++j) pr.code[a] |= (uint64_t)hpgq::adapt::code_of((unsigned char)probes[a][j]) << (2 * j);
    pr.len[a] = (uint32_t)k;
    pr.kmin = std::min(pr.kmin, k);
    kmax = std::max(kmax, k);
  }
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_adapt *q = new hpgq_adapt;
  q->pr = pr;
  q->wide = kmax > hpgq::adapt::kNarrowMax;
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

