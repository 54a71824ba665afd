// hpgq_parse.hip — FASTQ text -> SoA batch on the device.
//
// Replaces the parsing half of the reference's producer (fastq_fread_se,
// src/stats_fastq.c:183; the reader lives in the absent bioinfo-libs) for the
// GPU path: the host streams raw file bytes to HBM and the batch the engine
// reads (hpgq_batch_t: concatenated seq / quality + data_indices) is built on
// the device.  Records are 4 lines — "@header", sequence, "+[header]",
// quality of the sequence's length — with "\n" or "\r\n" line ends.
//
//   nl_count_kernel    newlines per 16 KB tile (SWAR byte compare)
//   (hipCUB scan)      tile offsets
//   nl_write_kernel    newline positions, in order (block scan per tile)
//   record_kernel      one thread per record: line bounds, validation, length
//   (hipCUB scan)      lengths -> data_indices
//   copy_kernel        one wave per record: seq / quality bytes into the batch
// Per-record offsets (record start, sequence, '+' line, quality) stay on the
// device for writers (hpgq_parse_records).
//
// Mate pairs:
//   interleaved text   the same passes up to record_kernel, then split_len_kernel
//                      and two scans of the lengths (even records, odd
//                      records), and split_copy_kernel, which routes record
//                      r to mate r & 1
//   pair_check_kernel  one lane per pair compares the two header names in
//                      16-byte windows; the lowest bad pair by wave reduction
//                      and one atomicMin per wave
#include "hpgq_accum.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>

namespace hpgq {
namespace parse {

constexpr int kTB = 256;               // threads per tile block
constexpr int kPerThread = 64;         // bytes per thread
constexpr int kTile = kTB * kPerThread;
constexpr int32_t kNoBad = 0x7FFFFFFF;   // d_bad[0]: no malformed record

__device__ __forceinline__ uint32_t nl_bytes(uint32_t w) {   // 0x80 per '\n' byte
  const uint32_t v = w ^ 0x0A0A0A0Au;
  return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

// newlines in this thread's 64 bytes; optionally their positions
__device__ __forceinline__ uint32_t thread_count(const uint8_t *t, int64_t n, int64_t base) {
  if (base + kPerThread <= n) {
    const uint4 *p = reinterpret_cast<const uint4 *>(t + base);
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kPerThread / 16; ++i) {
      const uint4 v = p[i];
      c += __builtin_popcount(nl_bytes(v.x)) + __builtin_popcount(nl_bytes(v.y)) +
           __builtin_popcount(nl_bytes(v.z)) + __builtin_popcount(nl_bytes(v.w));
    }
    return c;
  }
  uint32_t c = 0;
  for (int64_t i = base; i < n && i < base + kPerThread; ++i) c += t[i] == '\n';
  return c;
}

__global__ void __launch_bounds__(kTB) nl_count_kernel(const uint8_t *t, int64_t n, uint32_t *tiles) {
  typedef hipcub::BlockReduce<uint32_t, kTB> R;
  __shared__ typename R::TempStorage tmp;
  const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
  const uint32_t c = base < n ? thread_count(t, n, base) : 0u;
  const uint32_t s = R(tmp).Sum(c);
  if (threadIdx.x == 0) tiles[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kTB) nl_write_kernel(const uint8_t *t, int64_t n,
                                                       const uint32_t *tile_off, uint32_t *nl) {
  typedef hipcub::BlockScan<uint32_t, kTB> S;
  __shared__ typename S::TempStorage tmp;
  const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerThread;
  const uint32_t c = base < n ? thread_count(t, n, base) : 0u;
  uint32_t off;
  S(tmp).ExclusiveSum(c, off);
  off += tile_off[blockIdx.x];
  if (!c) return;
  const int64_t end = std::min<int64_t>(base + kPerThread, n);
  for (int64_t i = base; i < end; ++i)
    if (t[i] == '\n') nl[off++] = (uint32_t)i;
}

struct Rec {
  uint32_t *start, *seq, *plus, *qual;   // per-record offsets into the text
  int32_t *len;
};

// line [b, e) without a trailing '\r'
__device__ __forceinline__ uint32_t line_end(const uint8_t *t, uint32_t b, uint32_t e) {
  return (e > b && t[e - 1] == '\r') ? e - 1 : e;
}

// record i: its line bounds, the checks, its length (0 when malformed)
__device__ __forceinline__ int32_t record_one(const uint8_t *t, const uint32_t *nl, int64_t i, Rec R, int32_t *bad) {
  const uint32_t start = i ? nl[4 * i - 1] + 1 : 0u;
  const uint32_t n0 = nl[4 * i], n1 = nl[4 * i + 1], n2 = nl[4 * i + 2], n3 = nl[4 * i + 3];
  const uint32_t sb = n0 + 1, se = line_end(t, sb, n1);
  const uint32_t pb = n1 + 1, qb = n2 + 1, qe = line_end(t, qb, n3);
  const bool ok = n0 > start && t[start] == '@' && pb < n2 && t[pb] == '+' && (se - sb) == (qe - qb);
  R.start[i] = start;
  R.seq[i] = sb;
  R.plus[i] = pb;
  R.qual[i] = qb;
  R.len[i] = ok ? (int32_t)(se - sb) : 0;
  if (!ok) atomicMin(bad, (int32_t)min<int64_t>(i, 0x7FFFFFFF));
  return ok ? (int32_t)(se - sb) : 0;
}

// bad[0]: the first malformed record (atomicMin); bad[1]: the longest record
// (the long-read tail's reservation, hpgq_parser_max_length)
__global__ void __launch_bounds__(256) record_kernel(const uint8_t *t, const uint32_t *nl, int64_t nrec,
                                                     Rec R, int32_t *bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t len = 0;
  if (i < nrec) len = record_one(t, nl, i, R, bad);
  for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o));
  if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(bad + 1, len);
}

// one wave per record
__global__ void __launch_bounds__(256) copy_kernel(const uint8_t *t, Rec R, const int32_t *idx,
                                                   int64_t nrec, uint8_t *seq, uint8_t *qual) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nrec) return;
  const int lane = threadIdx.x & 63;
  const int32_t o = idx[i], L = idx[i + 1] - o;
  const uint8_t *s = t + R.seq[i], *q = t + R.qual[i];
  for (int j = lane; j < L; j += 64) {
    seq[o + j] = s[j];
    qual[o + j] = q[j];
  }
}

// ---- mate pairs -------------------------------------------------------------

constexpr int kMaxGrid = 2048;   // the grid-strided kernels' cap (256 CUs x 8)

// the lengths of an interleaved text's records, each mate's apart: out[m * np + i] = len[2 i + m]
// (two plain arrays, so the two scans are the single-text parse's own hipCUB instantiation)
__global__ void __launch_bounds__(256) split_len_kernel(const int32_t *len, int64_t nrec, int64_t np, int32_t *out) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nrec; r += (int64_t)gridDim.x * 256)
    out[(r & 1) * np + (r >> 1)] = len[r];
}

// L bytes s -> d by one wave: d's unaligned head and tail bytewise, the aligned
// words between as one dword store each (s is at any alignment: four byte loads)
__device__ __forceinline__ void wave_copy(uint8_t *d, const uint8_t *s, int L, int lane) {
  const int head = min(L, (int)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 3u)) & 3u));
  const int nw = (L - head) >> 2;
  const int tail = head + 4 * nw;
  if (lane < head) d[lane] = s[lane];
  for (int w = lane; w < nw; w += 64) {
    const uint8_t *p = s + head + 4 * w;
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    *reinterpret_cast<uint32_t *>(d + head + 4 * w) = v;
  }
  if (lane < L - tail) d[tail + lane] = s[tail + lane];
}

// one wave per record, grid-strided: record r of the text is read r >> 1 of mate r & 1
__global__ void __launch_bounds__(256) split_copy_kernel(const uint8_t *t, Rec R, const int32_t *idx1,
                                                         const int32_t *idx2, int64_t nrec, uint8_t *seq1,
                                                         uint8_t *qual1, uint8_t *seq2, uint8_t *qual2) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrec; r += (int64_t)gridDim.x * 4) {
    const int64_t i = r >> 1;
    const int32_t *idx = (r & 1) ? idx2 : idx1;
    const int32_t o = idx[i], L = idx[i + 1] - o;
    wave_copy(((r & 1) ? seq2 : seq1) + o, t + R.seq[r], L, lane);
    wave_copy(((r & 1) ? qual2 : qual1) + o, t + R.qual[r], L, lane);
  }
}

// One side of the name check: record i of the side is record i * stride + first
// of the parse (stride 2 for an interleaved text); n: bytes of the text.
struct NameSide {
  const uint8_t *t;
  const uint32_t *start, *seq;
  int64_t n;
  int stride, first;
};

// 16 bytes of the header at text offset pos; bytes at or past `end` (the header
// line's '\n', which the parse has placed inside the text) read as '\n'.  The
// vector load is taken only when all 16 bytes lie inside the text.
__device__ __forceinline__ void name_window(const uint8_t *t, int64_t n, int64_t pos, int64_t end, uint8_t w[16]) {
  if (pos + 16 <= n) {
    uint4 v;
    __builtin_memcpy(&v, t + pos, 16);
    __builtin_memcpy(w, &v, 16);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = pos + j < n ? t[pos + j] : (uint8_t)'\n';
  }
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (pos + j >= end) w[j] = '\n';
}

__device__ __forceinline__ bool name_ends(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

// The mate-name rule (hpgq.h) for one pair: the names run to the first
// space / tab / CR / LF; they must end at the same byte; they may differ in
// no byte, or in the last one alone as '1' against '2' after a '/'.  Names
// longer than a window go round the loop; a length difference ends it.
__device__ __forceinline__ bool names_in_step(const NameSide &A, const NameSide &B, int64_t i) {
  const int64_t ra = i * A.stride + A.first, rb = i * B.stride + B.first;
  const int64_t pa = (int64_t)A.start[ra] + 1, ea = (int64_t)A.seq[ra] - 1;   // after '@' .. the '\n'
  const int64_t pb = (int64_t)B.start[rb] + 1, eb = (int64_t)B.seq[rb] - 1;
  int ndiff = 0;            // differing bytes so far
  int64_t dpos = -1;        // where the first one is
  uint8_t da = 0, db = 0, dprev = 0, prev = 0;
  for (int64_t k = 0;; k += 16) {
    uint8_t wa[16], wb[16];
    name_window(A.t, A.n, pa + k, ea, wa);
    name_window(B.t, B.n, pb + k, eb, wb);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const bool enda = name_ends(wa[j]), endb = name_ends(wb[j]);
      if (enda || endb) {
        if (!(enda && endb)) return false;   // one name is longer
        if (ndiff == 0) return true;
        return dpos == k + j - 1 && da == '1' && db == '2' && dprev == '/';
      }
      if (wa[j] != wb[j]) {
        if (++ndiff > 1) return false;
        dpos = k + j;
        da = wa[j];
        db = wb[j];
        dprev = prev;
      }
      prev = wa[j];
    }
  }
}

// first_bad: the lowest pair out of step (atomicMin, one per wave)
__global__ void __launch_bounds__(256) pair_check_kernel(NameSide A, NameSide B, int64_t npairs, int32_t *first_bad) {
  int32_t bad = 0x7FFFFFFF;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * 256)
    if (!names_in_step(A, B, i)) bad = min(bad, (int32_t)i);
  for (int o = 32; o > 0; o >>= 1) bad = min(bad, __shfl_xor(bad, o));
  if ((threadIdx.x & 63) == 0 && bad != 0x7FFFFFFF) atomicMin(first_bad, bad);
}

}  // namespace parse
}  // namespace hpgq

struct hpgq_parser {
  int device = 0;
  hpgq::accum::Stream stream;
  uint8_t *d_text = nullptr;
  size_t text_cap = 0;
  uint32_t *d_tiles = nullptr;   // counts, then offsets (+ total)
  size_t tiles_cap = 0;
  uint32_t *d_nl = nullptr;
  size_t nl_cap = 0;
  uint32_t *d_rec = nullptr;     // 4 arrays of rec_cap
  int32_t *d_len = nullptr;      // rec_cap + 1 (data_indices)
  int32_t *d_idx = nullptr;
  size_t rec_cap = 0;
  uint8_t *d_seq = nullptr, *d_qual = nullptr;
  size_t data_cap = 0;
  int32_t *d_bad = nullptr;
  void *d_tmp = nullptr;
  size_t tmp_cap = 0;
  int64_t last_n = 0;            // records of the last parse
  int64_t max_len = 0;           // its longest record
  // mate 2 of an interleaved parse
  int32_t *d_idx2 = nullptr;
  size_t idx2_cap = 0;
  int32_t *d_len2 = nullptr;     // the lengths, each mate's apart (split_len_kernel)
  size_t len2_cap = 0;
  uint8_t *d_seq2 = nullptr, *d_qual2 = nullptr;
  size_t data2_cap = 0;
  // the last parse, for hpgq_parse_pair_check
  const uint8_t *last_text = nullptr;
  int64_t last_text_n = 0;
  bool last_interleaved = false;
  int max_wg = 0;                // hpgq_parser_debug_set_max_workgroups (0: no limit)
};

static int grow(void **p, size_t *cap, size_t need) {
  if (need <= *cap) return HPGQ_OK;
  (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t c = need + need / 4 + 4096;
  if (hipMalloc(p, c) != hipSuccess) return HPGQ_E_NOMEM;
  *cap = c;
  return HPGQ_OK;
}

static int scan_tmp(hpgq_parser *p, size_t need) {
  return grow(&p->d_tmp, &p->tmp_cap, need);
}

extern "C" {

int hpgq_parser_open(hpgq_parser_t **ps, int device, void *stream) {
  if (!ps) return HPGQ_E_INVALID;
  *ps = nullptr;
  int rc = hpgq::accum::use_device(device);
  if (rc) return rc;
  hpgq_parser *p = new hpgq_parser();
  p->device = device;
  if ((rc = p->stream.open(stream)) != HPGQ_OK) {
    delete p;
    return rc;
  }
  if (hipMalloc(&p->d_bad, 8) != hipSuccess) {
    hpgq_parser_close(p);
    return HPGQ_E_HIP;
  }
  *ps = p;
  return HPGQ_OK;
}

void hpgq_parser_close(hpgq_parser_t *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  (void)hipStreamSynchronize(p->stream);
  (void)hipFree(p->d_text);
  (void)hipFree(p->d_tiles);
  (void)hipFree(p->d_nl);
  (void)hipFree(p->d_rec);
  (void)hipFree(p->d_len);
  (void)hipFree(p->d_idx);
  (void)hipFree(p->d_seq);
  (void)hipFree(p->d_qual);
  (void)hipFree(p->d_bad);
  (void)hipFree(p->d_tmp);
  (void)hipFree(p->d_idx2);
  (void)hipFree(p->d_len2);
  (void)hipFree(p->d_seq2);
  (void)hipFree(p->d_qual2);
  p->stream.close();
  delete p;
}

// length of the text without trailing blank lines ("...\n\n", "\r\n\r\n" at the
// end of a file hold no record); tail: its last `nt` bytes
static int64_t trim_blank_tail(const char *tail, int64_t nt, int64_t n, bool &more) {
  more = false;
  const int64_t base = n - nt;   // text offset of tail[0]
  for (;;) {
    if (n < 1 || tail[n - 1 - base] != '\n') break;
    int64_t b = n - 1;   // content end of the last line
    if (b > base && tail[b - 1 - base] == '\r') --b;
    if (b == 0) {   // the text is blank lines only
      n = 0;
      break;
    }
    if (b - 1 < base) {   // the byte before lies past the fetched tail: fetch again, ending at n
      more = true;
      break;
    }
    if (tail[b - 1 - base] != '\n') break;   // the last line is not blank
    n = b;
  }
  return n;
}

}  // extern "C"

// steps 1-3 of a parse, shared by the single and the interleaved form: newline
// tiles, newline positions, record_kernel (queued, not waited for).  *nrec 0: an
// empty text.  pairs: an odd record count is HPGQ_E_PAIRING.
static int parse_lines(hpgq_parser *p, const char *text, int64_t n, bool pairs, int64_t *nrec_out,
                       hpgq::parse::Rec *R_out) {
  using namespace hpgq::parse;
  *nrec_out = 0;
  p->last_n = 0;
  p->max_len = 0;
  p->last_text = nullptr;
  p->last_text_n = 0;
  p->last_interleaved = pairs;
  HPGQ_HIP_TRY(hipSetDevice(p->device));
  for (bool more = n > 0; more;) {   // drop trailing blank lines
    char tail[64];
    const int64_t nt = n < 64 ? n : 64;
    HPGQ_HIP_TRY(hipMemcpyAsync(tail, text + n - nt, (size_t)nt, hipMemcpyDeviceToHost, p->stream));
    HPGQ_HIP_TRY(hipStreamSynchronize(p->stream));
    n = trim_blank_tail(tail, nt, n, more);
  }
  const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
  // 1. newline count per tile, tile offsets, total
  const int64_t ntiles = (n + kTile - 1) / kTile;
  // counts [0, ntiles + 1) then offsets [ntiles + 1, 2 (ntiles + 1))
  if (grow((void **)&p->d_tiles, &p->tiles_cap, (size_t)(ntiles + 1) * 8)) return HPGQ_E_NOMEM;
  uint32_t *d_off = p->d_tiles + ntiles + 1;
  HPGQ_HIP_TRY(hipMemsetAsync(p->d_tiles, 0, (size_t)(ntiles + 1) * 4, p->stream));
  if (ntiles) {
    nl_count_kernel<<<(unsigned)ntiles, kTB, 0, p->stream>>>(t, n, p->d_tiles);
    HPGQ_HIP_TRY(hipGetLastError());
  }
  size_t tb = 0;
  HPGQ_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, p->d_tiles, d_off, (int)ntiles + 1, p->stream));
  if (scan_tmp(p, tb)) return HPGQ_E_NOMEM;
  HPGQ_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(p->d_tmp, tb, p->d_tiles, d_off, (int)ntiles + 1, p->stream));
  uint32_t total = 0;
  HPGQ_HIP_TRY(hipMemcpyAsync(&total, d_off + ntiles, 4, hipMemcpyDeviceToHost, p->stream));
  HPGQ_HIP_TRY(hipStreamSynchronize(p->stream));
  if (total % 4 != 0) return HPGQ_E_FORMAT;   // not whole 4-line records
  const int64_t nrec = total / 4;
  if (nrec == 0) return HPGQ_OK;
  if (pairs && (nrec & 1)) return HPGQ_E_PAIRING;   // a mate without its partner
  // 2. newline positions
  if (grow((void **)&p->d_nl, &p->nl_cap, (size_t)total * 4)) return HPGQ_E_NOMEM;
  nl_write_kernel<<<(unsigned)ntiles, kTB, 0, p->stream>>>(t, n, d_off, p->d_nl);
  HPGQ_HIP_TRY(hipGetLastError());
  // 3. records
  if ((size_t)nrec + 1 > p->rec_cap) {
    (void)hipFree(p->d_rec);
    (void)hipFree(p->d_len);
    (void)hipFree(p->d_idx);
    p->d_rec = nullptr;
    p->d_len = p->d_idx = nullptr;
    p->rec_cap = 0;
    const size_t c = (size_t)nrec + nrec / 4 + 1024;
    if (hipMalloc(&p->d_rec, c * 16) != hipSuccess || hipMalloc(&p->d_len, c * 4) != hipSuccess ||
        hipMalloc(&p->d_idx, (c + 1) * 4) != hipSuccess)
      return HPGQ_E_NOMEM;
    p->rec_cap = c;
  }
  Rec R{p->d_rec, p->d_rec + p->rec_cap, p->d_rec + 2 * p->rec_cap, p->d_rec + 3 * p->rec_cap, p->d_len};
  const int32_t init[2] = {kNoBad, 0};   // first malformed record, longest record
  HPGQ_HIP_TRY(hipMemcpyAsync(p->d_bad, init, 8, hipMemcpyHostToDevice, p->stream));
  record_kernel<<<(unsigned)((nrec + 255) / 256), 256, 0, p->stream>>>(t, p->d_nl, nrec, R, p->d_bad);
  HPGQ_HIP_TRY(hipGetLastError());
  *nrec_out = nrec;
  *R_out = R;
  p->last_text = t;
  p->last_text_n = n;
  return HPGQ_OK;
}

// seq / quality buffers for `data_end` bytes (+ the engine's readable slack)
static int grow_data(uint8_t **seq, uint8_t **qual, size_t *cap, size_t data_end) {
  const size_t need = data_end + HPGQ_DEVICE_SLACK + 64;
  if (need <= *cap) return HPGQ_OK;
  (void)hipFree(*seq);
  (void)hipFree(*qual);
  *seq = *qual = nullptr;
  *cap = 0;
  const size_t c = need + need / 4 + 4096;
  if (hipMalloc(seq, c) != hipSuccess || hipMalloc(qual, c) != hipSuccess) return HPGQ_E_NOMEM;
  *cap = c;
  return HPGQ_OK;
}

// workgroups of a grid-strided kernel: capped, and by the tests' limit
static unsigned capped_grid(const hpgq_parser *p, int64_t blocks) {
  int64_t g = std::min<int64_t>(blocks, hpgq::parse::kMaxGrid);
  if (p->max_wg > 0 && g > p->max_wg) g = p->max_wg;
  return (unsigned)std::max<int64_t>(g, 1);
}

extern "C" {

int hpgq_parse_device(hpgq_parser_t *p, const char *text, int64_t n, hpgq_batch_t *out) {
  using namespace hpgq::parse;
  if (!p || !out || n < 0 || n >= ((int64_t)1 << 31)) return HPGQ_E_INVALID;
  *out = hpgq_batch_t{0, nullptr, nullptr, nullptr};
  int64_t nrec = 0;
  Rec R{};
  const int rc = parse_lines(p, text, n, false, &nrec, &R);
  if (rc || nrec == 0) return rc;
  const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
  size_t tb = 0;
  // 4. data_indices = [0, inclusive scan of the lengths]
  HPGQ_HIP_TRY(hipMemsetAsync(p->d_idx, 0, 4, p->stream));
  HPGQ_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb, p->d_len, p->d_idx + 1, (int)nrec, p->stream));
  if (scan_tmp(p, tb)) return HPGQ_E_NOMEM;
  HPGQ_HIP_TRY(hipcub::DeviceScan::InclusiveSum(p->d_tmp, tb, p->d_len, p->d_idx + 1, (int)nrec, p->stream));
  int32_t bad[2] = {0, 0}, data_end = 0;
  HPGQ_HIP_TRY(hipMemcpyAsync(bad, p->d_bad, 8, hipMemcpyDeviceToHost, p->stream));
  HPGQ_HIP_TRY(hipMemcpyAsync(&data_end, p->d_idx + nrec, 4, hipMemcpyDeviceToHost, p->stream));
  HPGQ_HIP_TRY(hipStreamSynchronize(p->stream));
  if (bad[0] != kNoBad) return HPGQ_E_FORMAT;
  // 5. the batch bytes (+ the engine's readable slack)
  if (grow_data(&p->d_seq, &p->d_qual, &p->data_cap, (size_t)data_end)) return HPGQ_E_NOMEM;
  copy_kernel<<<(unsigned)((nrec + 3) / 4), 256, 0, p->stream>>>(t, R, p->d_idx, nrec, p->d_seq, p->d_qual);
  HPGQ_HIP_TRY(hipGetLastError());
  out->num_reads = nrec;
  out->seq = reinterpret_cast<const char *>(p->d_seq);
  out->quality = reinterpret_cast<const char *>(p->d_qual);
  out->data_indices = p->d_idx;
  p->last_n = nrec;
  p->max_len = bad[1];
  return HPGQ_OK;
}

int hpgq_parse_host(hpgq_parser_t *p, const char *text, int64_t n, hpgq_batch_t *out) {
  if (!p || (!text && n > 0) || n < 0 || n >= ((int64_t)1 << 31)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(p->device));
  if (grow((void **)&p->d_text, &p->text_cap, (size_t)n + 16)) return HPGQ_E_NOMEM;
  if (n) HPGQ_HIP_TRY(hipMemcpyAsync(p->d_text, text, (size_t)n, hipMemcpyHostToDevice, p->stream));
  return hpgq_parse_device(p, reinterpret_cast<const char *>(p->d_text), n, out);
}

int hpgq_parse_device_interleaved(hpgq_parser_t *p, const char *text, int64_t n, hpgq_batch_t *out1,
                                  hpgq_batch_t *out2) {
  using namespace hpgq::parse;
  if (!p || !out1 || !out2 || n < 0 || n >= ((int64_t)1 << 31)) return HPGQ_E_INVALID;
  *out1 = *out2 = hpgq_batch_t{0, nullptr, nullptr, nullptr};
  int64_t nrec = 0;
  Rec R{};
  const int rc = parse_lines(p, text, n, true, &nrec, &R);
  if (rc || nrec == 0) return rc;
  const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
  const int np = (int)(nrec / 2);
  // 4. each mate's data_indices: the lengths of the even and of the odd records, scanned apart
  if (grow((void **)&p->d_idx2, &p->idx2_cap, ((size_t)np + 1) * 4) ||
      grow((void **)&p->d_len2, &p->len2_cap, (size_t)nrec * 4))
    return HPGQ_E_NOMEM;
  int32_t *idx[2] = {p->d_idx, p->d_idx2};
  split_len_kernel<<<capped_grid(p, (nrec + 255) / 256), 256, 0, p->stream>>>(p->d_len, nrec, np, p->d_len2);
  HPGQ_HIP_TRY(hipGetLastError());
  for (int m = 0; m < 2; ++m) {
    int32_t *in = p->d_len2 + (size_t)m * np;   // (int32_t *, as the single-text scan: one instantiation)
    size_t tb = 0;
    HPGQ_HIP_TRY(hipMemsetAsync(idx[m], 0, 4, p->stream));
    HPGQ_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb, in, idx[m] + 1, np, p->stream));
    if (scan_tmp(p, tb)) return HPGQ_E_NOMEM;
    HPGQ_HIP_TRY(hipcub::DeviceScan::InclusiveSum(p->d_tmp, tb, in, idx[m] + 1, np, p->stream));
  }
  int32_t bad[2] = {0, 0}, data_end[2] = {0, 0};
  HPGQ_HIP_TRY(hipMemcpyAsync(bad, p->d_bad, 8, hipMemcpyDeviceToHost, p->stream));
  for (int m = 0; m < 2; ++m)
    HPGQ_HIP_TRY(hipMemcpyAsync(&data_end[m], idx[m] + np, 4, hipMemcpyDeviceToHost, p->stream));
  HPGQ_HIP_TRY(hipStreamSynchronize(p->stream));
  if (bad[0] != kNoBad) return HPGQ_E_FORMAT;
  // 5. one copy pass: record r to mate r & 1
  if (grow_data(&p->d_seq, &p->d_qual, &p->data_cap, (size_t)data_end[0]) ||
      grow_data(&p->d_seq2, &p->d_qual2, &p->data2_cap, (size_t)data_end[1]))
    return HPGQ_E_NOMEM;
  split_copy_kernel<<<capped_grid(p, (nrec + 3) / 4), 256, 0, p->stream>>>(t, R, p->d_idx, p->d_idx2, nrec, p->d_seq,
                                                                         p->d_qual, p->d_seq2, p->d_qual2);
  HPGQ_HIP_TRY(hipGetLastError());
  out1->num_reads = out2->num_reads = np;
  out1->seq = reinterpret_cast<const char *>(p->d_seq);
  out1->quality = reinterpret_cast<const char *>(p->d_qual);
  out1->data_indices = p->d_idx;
  out2->seq = reinterpret_cast<const char *>(p->d_seq2);
  out2->quality = reinterpret_cast<const char *>(p->d_qual2);
  out2->data_indices = p->d_idx2;
  p->last_n = nrec;
  p->max_len = bad[1];
  return HPGQ_OK;
}

int hpgq_parse_host_interleaved(hpgq_parser_t *p, const char *text, int64_t n, hpgq_batch_t *out1,
                                hpgq_batch_t *out2) {
  if (!p || (!text && n > 0) || n < 0 || n >= ((int64_t)1 << 31)) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(p->device));
  if (grow((void **)&p->d_text, &p->text_cap, (size_t)n + 16)) return HPGQ_E_NOMEM;
  if (n) HPGQ_HIP_TRY(hipMemcpyAsync(p->d_text, text, (size_t)n, hipMemcpyHostToDevice, p->stream));
  return hpgq_parse_device_interleaved(p, reinterpret_cast<const char *>(p->d_text), n, out1, out2);
}

int hpgq_parse_pair_check(hpgq_parser_t *p1, hpgq_parser_t *p2, int64_t *first_bad) {
  using namespace hpgq::parse;
  if (!p1 || !first_bad || p1 == p2) return HPGQ_E_INVALID;
  *first_bad = -1;
  if (p2 ? (p2->device != p1->device || p1->last_interleaved || p2->last_interleaved) : !p1->last_interleaved)
    return p2 && p2->device != p1->device ? HPGQ_E_INVALID : HPGQ_E_STATE;
  HPGQ_HIP_TRY(hipSetDevice(p1->device));
  const int64_t n1 = p2 ? p1->last_n : p1->last_n / 2, n2 = p2 ? p2->last_n : n1;
  const int64_t np = std::min(n1, n2);
  int32_t bad = kNoBad;
  if (np > 0) {
    // (the parses synchronise their streams, so ps2's records are complete)
    NameSide A{p1->last_text, p1->d_rec, p1->d_rec + p1->rec_cap, p1->last_text_n, p2 ? 1 : 2, 0};
    NameSide B = p2 ? NameSide{p2->last_text, p2->d_rec, p2->d_rec + p2->rec_cap, p2->last_text_n, 1, 0}
                    : NameSide{A.t, A.start, A.seq, A.n, 2, 1};
    HPGQ_HIP_TRY(hipMemcpyAsync(p1->d_bad, &bad, 4, hipMemcpyHostToDevice, p1->stream));
    pair_check_kernel<<<capped_grid(p1, (np + 255) / 256), 256, 0, p1->stream>>>(A, B, np, p1->d_bad);
    HPGQ_HIP_TRY(hipGetLastError());
    HPGQ_HIP_TRY(hipMemcpyAsync(&bad, p1->d_bad, 4, hipMemcpyDeviceToHost, p1->stream));
  }
  HPGQ_HIP_TRY(hipStreamSynchronize(p1->stream));
  if (bad != kNoBad) *first_bad = bad;
  else if (n1 != n2) *first_bad = np;
  return *first_bad < 0 ? HPGQ_OK : HPGQ_E_PAIRING;
}

int hpgq_parser_debug_set_max_workgroups(hpgq_parser_t *p, int max_wg) {
  if (!p || max_wg < 0) return HPGQ_E_INVALID;
  p->max_wg = max_wg;
  return HPGQ_OK;
}

int hpgq_parse_records(hpgq_parser_t *p, uint32_t *rec_start, uint32_t *seq_start,
                       uint32_t *plus_start, uint32_t *qual_start) {
  if (!p) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(p->device));
  const size_t b = (size_t)p->last_n * 4;
  uint32_t *dst[4] = {rec_start, seq_start, plus_start, qual_start};
  for (int k = 0; k < 4; ++k)
    if (dst[k] && b)
      HPGQ_HIP_TRY(hipMemcpyAsync(dst[k], p->d_rec + (size_t)k * p->rec_cap, b, hipMemcpyDeviceToHost,
                                  p->stream));
  HPGQ_HIP_TRY(hipStreamSynchronize(p->stream));
  return HPGQ_OK;
}

void *hpgq_parser_stream(hpgq_parser_t *p) { return p ? (void *)p->stream : nullptr; }

int64_t hpgq_parser_max_length(hpgq_parser_t *p) { return p ? p->max_len : 0; }

}  // extern "C"
