// hpgq_engine_geo.hip — instances of the segmented kernel for ONE geometry
// (built once per geometry with -DHPGQ_GEO=0|1|2, so the three compile in
// parallel).  Occupancy per variant (MINW, waves per SIMD) is the highest at
// which the variant's registers fit without spills: single-end 4 (tri 5),
// paired-end 3 (two mates' accumulators), single-end edit 3 (its next trim
// windows held in VGPRs, tri_body EG; 4 with the extra scans or as a
// follow-up; 4 with the trims at the step, tri_body ST), see DESIGN.md §4.1.  Every
// combination of paired-end, edit and the extra filter scans has an instance.
#include <cstdio>

#include "hpgq_engine_tri.h"

#ifndef HPGQ_GEO
#error "build with -DHPGQ_GEO=0 (tri), 1 (hex) or 2 (wide)"
#endif

namespace hpgq {

namespace {

constexpr int G = HPGQ_GEO;
#ifndef HPGQ_SE_WAVES
#define HPGQ_SE_WAVES (G == GEO_TRI ? 5 : 4)
#endif
constexpr int kSeW = HPGQ_SE_WAVES;          // single-end
#ifndef HPGQ_PE_WAVES
#define HPGQ_PE_WAVES 3
#endif
constexpr int kPeW = HPGQ_PE_WAVES;          // paired-end
#ifndef HPGQ_EDIT_WAVES
#define HPGQ_EDIT_WAVES 3
#endif
constexpr int kEdW = HPGQ_EDIT_WAVES;        // single-end edit (its trim windows in VGPRs a group early: tri_body EG)
constexpr int kEdXW = kSeW;                  // single-end edit with extra filter scans
#ifndef HPGQ_ST_WAVES
#define HPGQ_ST_WAVES 4
#endif
constexpr int kStW = HPGQ_ST_WAVES;          // single-end edit, trims at the step (tri_body ST; its 7
                                             // spilled VGPRs sit outside the group loop)
constexpr const char *kGeoName = G == GEO_TRI ? "tri" : (G == GEO_HEX ? "hex" : "wide");

// the descriptor of ONE instance: everything the host needs comes from the
// same template arguments as the kernel (its LDS bytes from its own layout)
template <int MINW, int NM, bool EDIT, int XM, bool F>
KernelDesc desc() {
  KernelDesc d;
  if constexpr (XM == 0) {
    d.fn = (const void *)engine_tri_kernel<MINW, NM, EDIT, G, F>;
    std::snprintf(d.name, sizeof(d.name), "hpgq::engine_tri_kernel<%d, %d, %s, %s%s>", MINW, NM,
                  EDIT ? "edit" : "filter", kGeoName, F ? ", follow" : "");
  } else {
    d.fn = (const void *)engine_tri_x_kernel<MINW, NM, G, F, XM, EDIT>;
    if constexpr (XM == X_ST)
      std::snprintf(d.name, sizeof(d.name), "hpgq::engine_tri_kernel<%d, 1, edit, %s, st>", MINW, kGeoName);
    else
      std::snprintf(d.name, sizeof(d.name), "hpgq::engine_tri_x_kernel<%d, %d, %s%s%s%s%s>", MINW, NM, kGeoName,
                    EDIT ? ", edit" : "", F ? ", follow" : "", (XM & X_NOOR) ? ", noor" : "",
                    (XM & X_LR) ? ", window" : "");
  }
  d.block = Geo<G>::kBlock;
  d.pos = Geo<G>::kPos;
  d.lds_bytes = SegLds<NM, G, XM, EDIT, F>::bytes_for;
  return d;
}

template <bool F, bool EDIT, int XM>
KernelDesc inst(int nm) {
  constexpr int kW1 = EDIT ? (XM || F ? kEdXW : kEdW) : kSeW;   // single-end waves per SIMD
  return nm == 2 ? desc<kPeW, 2, EDIT, XM, F>() : desc<kW1, 1, EDIT, XM, F>();
}

// the instance for (nm, edit, xm) as a first (F false) or follow-up stage; fn
// stays null when there is none
template <bool F, bool EDIT>
KernelDesc pick_xm(int nm, int xm) {
  switch (xm) {
    case 0: return inst<F, EDIT, 0>(nm);
    case X_NOOR: return inst<F, EDIT, X_NOOR>(nm);
    case X_LR: return inst<F, EDIT, X_LR>(nm);
    case X_NOOR | X_LR: return inst<F, EDIT, X_NOOR | X_LR>(nm);
    case X_ST:   // single-end edit with the trims applied at the step (hex, first stage: tri_body ST)
      if constexpr (G == GEO_HEX && !F && EDIT) {
        if (nm == 1) return desc<kStW, 1, true, X_ST, false>();
      }
      break;
    default: break;
  }
  return KernelDesc{};
}

template <bool F>
KernelDesc pick(int nm, bool edit, int xm) {
  return edit ? pick_xm<F, true>(nm, xm) : pick_xm<F, false>(nm, xm);
}

}  // namespace

#if HPGQ_GEO == 0
KernelDesc seg_kernel_tri(int nm, bool edit, int xm, bool follow) {
  return follow ? KernelDesc{} : pick<false>(nm, edit, xm);
}
#elif HPGQ_GEO == 1
KernelDesc seg_kernel_hex(int nm, bool edit, int xm, bool follow) {
  return follow ? KernelDesc{} : pick<false>(nm, edit, xm);
}
#else
KernelDesc seg_kernel_wide(int nm, bool edit, int xm, bool follow) {
  return follow ? pick<true>(nm, edit, xm) : pick<false>(nm, edit, xm);
}
#endif

}  // namespace hpgq
