// hpgq_engine_lds.h — the dynamic LDS of the engine kernels, laid out ONCE.
//
// The kernels (tri_body in hpgq_engine_tri.h, engine_kernel in
// hpgq_engine_kernel.h) take every LDS pointer from the structs below, and the
// host (hpgq_engine.hip, through each instance's descriptor) takes the byte
// count of the launch from the same struct's bytes(), so a region added here
// is allocated and addressed at once.  Every region is one accessor, in 32-bit
// words: given the kernel's `uint32_t *` to the start of the dynamic LDS it
// returns the region's pointer, given the integer 0 its word offset (host,
// tests).  Plain C++17, no HIP: tests/lds_layout/ compiles it with a host
// compiler and checks every region of every instance.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/hpgq.h"

#if defined(__HIPCC__)
#define HPGQ_HD __host__ __device__
#else
#define HPGQ_HD
#endif

namespace hpgq {

constexpr int kWG = 256;
constexpr int kWaves = kWG / 64;

constexpr int GEO_TRI = 0, GEO_HEX = 1, GEO_WIDE = 2;
constexpr int X_NOOR = 1, X_LR = 2;   // extra filter scans (engine_tri_x_kernel)
constexpr int X_ST = 4;               // single-end edit, trims applied at the step (tri_body ST)

// kBlock reads (<= 64: lane j <-> read j in the epilogue) in steps of kSegs
// reads, kU steps per pipeline group, an even number of groups per block.
template <int G>
struct Geo;
template <>
struct Geo<GEO_TRI> {
  static constexpr int kNW = 2, kSegs = 3, kSegW = 21, kOwn = 20, kBlock = 54, kU = 3, kPos = 160;
};
template <>
struct Geo<GEO_HEX> {
  static constexpr int kNW = 4, kSegs = 6, kSegW = 10, kOwn = 10, kBlock = 48, kU = 2, kPos = 156;
};
template <>
struct Geo<GEO_WIDE> {   // 60-read blocks: read-table entry 63 stays empty (the padding steps' source)
  static constexpr int kNW = 4, kSegs = 4, kSegW = 16, kOwn = 16, kBlock = 60, kU = 2, kPos = 252;
};

// The exact mean-quality sum (u64 per lane and mate) accumulates in per-lane
// LDS slots (one no-return ds_add_u64 per unit) instead of a VGPR pair held
// across the loop: the paired-end edit kernel spilled exactly those pairs, a
// scratch load + store per unit and mate (~200 MB of scratch writes per 10 M
// pairs).  (32 slots, lane & 31, since round 6: two lanes add into each, which
// frees the LDS the reciprocal table takes without costing the paired-end edit
// kernel its third workgroup per CU)
constexpr int kFxSlots = 32;
constexpr int kFxWords = 2 * kFxSlots;   // per wave and mate: kFxSlots u64
// ST: per wave, the step's raw seq and quality dwords of every lane (64 x 16 B
// each, + 32 B read past the last lane), read back from a per-lane byte offset
constexpr int kStWords = 2 * (64 * 4 + 8);
constexpr int kColdWords = 34;   // sizeof(ColdParams) / 4 (asserted in hpgq_engine_kernel.h)

// The segmented kernels (tri_body<MINW, NM, EDIT, G, XM, FOLLOW>), lmax given:
//   per mate    pos_acc [6][lp] u32 (row 5: "other" until the epilogue turns it
//               into N) | hist [hlen] u32 | sc [8] u64
//   per wave    (ST: two shift buffers, first so that their reads' offsets fit
//               the ds_read2 offset fields) | per mate two read tables [64] x
//               16 B alternating between blocks and the segment ends [64] (+
//               [64] NX, + [64] LR) | a compaction scratch [64] | the deferral
//               word (u64, disjoint from the scratch: no type-punned aliasing)
//               | per mate the mean-quality slots | (TDMA: per mate three DMA
//               rows of kBlock x 16 B: left, right 0, right 1)
//   then        the byte-mask table [4 NW + 1][NW] | the reciprocal table
//               [kPos + 1] of the epilogue's divisions
// The on-chip partials cover lp = min(lmax, kPos) positions: every read these
// kernels merge is at most that long (longer ones are deferred), so the
// counter set on chip does not grow with lmax.
template <int NM, int G, int XM, bool EDIT, bool FOLLOW>
struct SegLds {
  using GG = Geo<G>;
  static constexpr bool NX = (XM & X_NOOR) != 0, LR = (XM & X_LR) != 0, ST = (XM & X_ST) != 0;
  // TDMA: paired-end edit, first stage, no extra scans (tri_body)
  static constexpr bool TDMA = EDIT && !FOLLOW && NM == 2 && XM == 0;

  // ---- a wave's region (w: its start, from wave()) -----------------------
  static constexpr int kStBufWords = ST ? kStWords : 0;
  static constexpr int kMateWaveWords = 2 * 256 + 64 * (1 + (NX ? 1 : 0) + (LR ? 1 : 0));
  static constexpr int kRowWords = GG::kBlock * 4;   // one DMA row
  static constexpr int kDmaWords = TDMA ? NM * 3 * kRowWords : 0;
  static constexpr int kWaveWords = kStBufWords + NM * kMateWaveWords + 64 + 4 + NM * kFxWords + kDmaWords;
  template <class P> static constexpr HPGQ_HD P stbuf(P w, int b) { return w + b * (kStWords / 2); }   // ST: seq, quality
  template <class P> static constexpr HPGQ_HD P tab(P w, int m, int tb) {
    return w + kStBufWords + m * kMateWaveWords + tb * 256;
  }
  template <class P> static constexpr HPGQ_HD P ends(P w, int m) { return tab(w, m, 2); }
  template <class P> static constexpr HPGQ_HD P ends2(P w, int m) { return ends(w, m) + 64; }   // NX only
  template <class P> static constexpr HPGQ_HD P ends3(P w, int m) { return ends(w, m) + (NX ? 128 : 64); }   // LR only
  template <class P> static constexpr HPGQ_HD P scratch(P w) { return w + kStBufWords + NM * kMateWaveWords; }
  template <class P> static constexpr HPGQ_HD P dword(P w) { return scratch(w) + 64; }   // u64
  template <class P> static constexpr HPGQ_HD P fxs(P w, int m) { return scratch(w) + 64 + 4 + m * kFxWords; }   // u64
  template <class P> static constexpr HPGQ_HD P dma_row(P w, int m, int r) {   // TDMA
    return scratch(w) + 64 + 4 + NM * kFxWords + (m * 3 + r) * kRowWords;
  }

  // ---- after the waves ------------------------------------------------------
  static constexpr int kMaskWords = (4 * GG::kNW + 1) * GG::kNW;   // written and read
  // (reserved: a fixed 17 x 16 B, also for tri, which uses 18 words of it)
  static constexpr int kMaskSlotWords = 17 * 4;
  static constexpr int kRecipWords = GG::kPos + 1;
  // tab_words rounds the mates' partials up to 16 B, by at most 12 bytes; the
  // allocation carries a whole 16 B for it.  Both this and the mask slot's
  // unused words are slack the byte count has always had: it decides the
  // workgroups per CU and with them every grid, so it stays.
  static constexpr int kAlignPadWords = 4;

  static_assert(kStBufWords % 8 == 0 && kMateWaveWords % 4 == 0 && kFxWords % 4 == 0 && kRowWords % 4 == 0, "16 B regions");
  static_assert(kMaskWords <= kMaskSlotWords, "mask table slot");
  static_assert(kWaves <= kMaskSlotWords, "pos_fix's wave totals reuse the mask table");

  int lp, hist_words, mate_words, tab_words;
  HPGQ_HD static int positions(int lmax) { return lmax < GG::kPos ? lmax : GG::kPos; }   // on chip
  HPGQ_HD explicit SegLds(int lmax) {
    lp = positions(lmax);
    const int hlen = lp + 1 + HPGQ_MEANQ_BINS + HPGQ_GC_BINS;
    hist_words = (hlen + 1) & ~1;
    mate_words = 6 * lp + hist_words + 2 * HPGQ_NUM_SCALARS;   // even: sc 8-B aligned
    tab_words = (NM * mate_words + 3) & ~3;                    // 16 B aligned
  }
  template <class P> HPGQ_HD P pos_acc(P base, int m) const { return base + m * mate_words; }
  template <class P> HPGQ_HD P other(P base, int m) const { return base + m * mate_words + 5 * lp; }
  template <class P> HPGQ_HD P hist(P base, int m) const { return base + m * mate_words + 6 * lp; }
  template <class P> HPGQ_HD P sc(P base, int m) const { return hist(base, m) + hist_words; }   // [8] u64
  HPGQ_HD int partial_words() const { return NM * mate_words; }   // from base on: zeroed at the start
  template <class P> HPGQ_HD P wave(P base, int w) const { return base + tab_words + w * kWaveWords; }
  template <class P> HPGQ_HD P mtab(P base) const { return base + tab_words + kWaves * kWaveWords; }
  template <class P> HPGQ_HD P rtab(P base) const { return mtab(base) + kMaskSlotWords; }
  // reuse: after the unit loop the mask table is free and holds pos_fix's kWaves wave totals
  template <class P> HPGQ_HD P pos_fix_wtot(P base) const { return mtab(base); }
  HPGQ_HD size_t bytes() const {
    return ((size_t)NM * mate_words + kAlignPadWords + (size_t)kWaves * kWaveWords + kMaskSlotWords + kRecipWords) * 4;
  }
  static size_t bytes_for(int lmax) { return SegLds(lmax).bytes(); }   // (the host's descriptor holds this)
};

// The catch-all (engine_kernel<NM, NCH, GEN, FOLLOW>): pos_acc [NM][6][lmax]
// u32 | hist [NM][hlen] u32 | sc [NM][8] u64 | the cold parameters | per wave
// a compaction scratch [64] u32.
template <int NM>
struct CatchAllLds {
  int lmax, hlen;
  HPGQ_HD explicit CatchAllLds(int lmax_) : lmax(lmax_), hlen(lmax_ + 1 + HPGQ_MEANQ_BINS + HPGQ_GC_BINS) {}
  HPGQ_HD int hist_words() const { return (NM * hlen + 1) & ~1; }   // even: sc 8-B aligned
  template <class P> HPGQ_HD P pos_acc(P base, int m) const { return base + m * 6 * lmax; }
  template <class P> HPGQ_HD P hist(P base, int m) const { return base + NM * 6 * lmax + m * hlen; }
  HPGQ_HD int partial_words() const { return NM * 6 * lmax + hist_words(); }   // from base on: zeroed at the start
  template <class P> HPGQ_HD P sc(P base, int m) const {
    return base + NM * 6 * lmax + hist_words() + m * 2 * HPGQ_NUM_SCALARS;   // [8] u64
  }
  template <class P> HPGQ_HD P cold(P base) const { return sc(base, NM); }
  template <class P> HPGQ_HD P scratch(P base, int w) const { return cold(base) + kColdWords + w * 64; }
  // reuse: after the unit loop the compaction scratch is free and holds pos_fix's kWaves wave totals
  template <class P> HPGQ_HD P pos_fix_wtot(P base) const { return scratch(base, 0); }
  HPGQ_HD size_t bytes() const { return (size_t)scratch(0, kWaves) * 4; }
  static size_t bytes_for(int lmax) { return CatchAllLds(lmax).bytes(); }
};

}  // namespace hpgq
