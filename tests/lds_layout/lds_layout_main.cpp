// Prints the LDS layout of every engine kernel instance (hpgq_engine_lds.h) for
// tests/test_lds_layout_cpu.py: per instance and lmax one "I" line with
// bytes(), then one "R" line per region: name, [begin, end) in bytes, the
// alignment it needs, and the region it reuses after the unit loop ("-": none).
// Host only; includes nothing but the layout header and the ABI header.
#include <cstdio>

#include "hpgq.h"
#include "hpgq_engine_lds.h"

using namespace hpgq;

static const int kLmax[] = {1, 2, 155, 156, 157, 160, 161, 251, 252, 253, 1023, 1024};

static void region(const char *name, int m, int w, int k, long begin_words, long words, int align, const char *reuses) {
  char full[64];
  std::snprintf(full, sizeof(full), "%s[m%d,w%d,%d]", name, m, w, k);
  std::printf("R %s %ld %ld %d %s\n", full, begin_words * 4, (begin_words + words) * 4, align, reuses);
}

template <int NM, int G, int XM, bool EDIT, bool FOLLOW>
static void seg() {
  using L = SegLds<NM, G, XM, EDIT, FOLLOW>;
  for (int lmax : kLmax) {
    const L lay(lmax);
    std::printf("I seg geo=%d nm=%d xm=%d edit=%d follow=%d lmax=%d bytes=%zu block=%d pos=%d\n", G, NM, XM, (int)EDIT,
                (int)FOLLOW, lmax, lay.bytes(), Geo<G>::kBlock, Geo<G>::kPos);
    for (int m = 0; m < NM; ++m) {
      region("pos_acc", m, 0, 0, lay.pos_acc(0L, m), 5L * lay.lp, 4, "-");
      region("other", m, 0, 0, lay.other(0L, m), lay.lp, 4, "-");   // pos_acc's sixth row
      region("hist", m, 0, 0, lay.hist(0L, m), lay.lp + 1 + HPGQ_MEANQ_BINS + HPGQ_GC_BINS, 4, "-");
      region("sc", m, 0, 0, lay.sc(0L, m), 2 * HPGQ_NUM_SCALARS, 8, "-");
    }
    for (int w = 0; w < kWaves; ++w) {
      const long wr = lay.wave(0L, w);
      if (L::ST)
        for (int b = 0; b < 2; ++b) region("stbuf", 0, w, b, L::stbuf(wr, b), kStWords / 2, 16, "-");
      for (int m = 0; m < NM; ++m) {
        for (int tb = 0; tb < 2; ++tb) region("tab", m, w, tb, L::tab(wr, m, tb), 256, 16, "-");
        region("ends", m, w, 0, L::ends(wr, m), 64, 4, "-");
        if (L::NX) region("ends2", m, w, 0, L::ends2(wr, m), 64, 4, "-");
        if (L::LR) region("ends3", m, w, 0, L::ends3(wr, m), 64, 4, "-");
        region("fxs", m, w, 0, L::fxs(wr, m), kFxWords, 8, "-");
        if (L::TDMA)
          for (int r = 0; r < 3; ++r) region("dma_row", m, w, r, L::dma_row(wr, m, r), L::kRowWords, 16, "-");
      }
      region("scratch", 0, w, 0, L::scratch(wr), 64, 4, "-");
      region("dword", 0, w, 0, L::dword(wr), 2, 8, "-");
    }
    region("mtab", 0, 0, 0, lay.mtab(0L), L::kMaskWords, 16, "-");
    region("rtab", 0, 0, 0, lay.rtab(0L), L::kRecipWords, 4, "-");
    region("pos_fix_wtot", 0, 0, 0, lay.pos_fix_wtot(0L), kWaves, 4, "mtab[m0,w0,0]");
  }
}

template <int NM, bool EDIT, int G, bool FOLLOW>
static void scans() {
  seg<NM, G, 0, EDIT, FOLLOW>();
  seg<NM, G, X_NOOR, EDIT, FOLLOW>();
  seg<NM, G, X_LR, EDIT, FOLLOW>();
  seg<NM, G, X_NOOR | X_LR, EDIT, FOLLOW>();
}

template <int G, bool FOLLOW>
static void geometry() {
  scans<1, false, G, FOLLOW>();
  scans<1, true, G, FOLLOW>();
  scans<2, false, G, FOLLOW>();
  scans<2, true, G, FOLLOW>();
}

template <int NM>
static void catch_all() {
  for (int lmax : kLmax) {
    const CatchAllLds<NM> lay(lmax);
    std::printf("I catch_all nm=%d lmax=%d bytes=%zu\n", NM, lmax, lay.bytes());
    for (int m = 0; m < NM; ++m) {
      region("pos_acc", m, 0, 0, lay.pos_acc(0L, m), 6L * lmax, 4, "-");
      region("hist", m, 0, 0, lay.hist(0L, m), lay.hlen, 4, "-");
      region("sc", m, 0, 0, lay.sc(0L, m), 2 * HPGQ_NUM_SCALARS, 8, "-");
    }
    region("cold", 0, 0, 0, lay.cold(0L), kColdWords, 4, "-");
    for (int w = 0; w < kWaves; ++w) region("scratch", 0, w, 0, lay.scratch(0L, w), 64, 4, "-");
    region("pos_fix_wtot", 0, 0, 0, lay.pos_fix_wtot(0L), kWaves, 4, "scratch[m0,w0,0]");
  }
}

int main() {
  geometry<GEO_TRI, false>();
  geometry<GEO_HEX, false>();
  geometry<GEO_WIDE, false>();
  seg<1, GEO_HEX, X_ST, true, false>();   // single-end edit, trims at the step
  geometry<GEO_WIDE, true>();             // the wide follow-up
  catch_all<1>();
  catch_all<2>();
  return 0;
}
