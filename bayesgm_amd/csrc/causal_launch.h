// causal_launch.h -- host-side dispatch of the LDS-resident CausalBGM kernels, shared by the translation units that instantiate them
// (causal_api.hip, causal_event_api.hip, causal_prior_api.hip, causal_rowadapt_api.hip, causal_bx3_api.hip, fit_api.hip): the launch
// geometry, the table of compiled shapes and the dispatch from a handle's shape to a template instantiation.  The launch itself is
// bgm_launch (bgm_host.h), shared with the BGM kernels (bgm_launch.h).  Host only: no kernel lives here, and which kernels a unit instantiates is decided by the lambdas it passes to bgm_causal_dispatch.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>

#include "bgm_host.h"

// ---- launch geometry: MH_WAVES waves per workgroup, MH_R 16-row tiles per wave (build options: build.py -D BGM_MH_WAVES=n).
// bgm_causal_mh_run sizes the grid, the slot count it reports, the slot-private counters, the ADRF partial sums and the event regions
// from these two, so every kernel of the family is instantiated with them.
#ifndef BGM_MH_R
#define BGM_MH_R 1
#endif
#ifndef BGM_MH_WAVES
#define BGM_MH_WAVES 8
#endif
static constexpr int MH_R = BGM_MH_R, MH_WAVES = BGM_MH_WAVES;
static_assert(MH_R == 1, "BGM_MH_R != 1: the conditional-prior, per-chain-scale, event-form and split-precision MH kernels exist for one row "
                         "tile per wave only, and they share the grid and the per-slot buffers of the default path");

// workgroups over n rows at `row_tiles` 16-row tiles per wave, at most one per CU; a wave slot (grid * MH_WAVES of them) loops over the rest
static inline int bgm_causal_grid(const bgm_handle *h, int64_t n, int row_tiles) {
  return bgm_tile_grid(h, (n + 16 * row_tiles - 1) / (16 * row_tiles), MH_WAVES);
}

// ---- compiled shapes.  (KT1, KSL1, NTL): first-layer K tiling and number of 16-wide output tiles of g's last layer.
//   (1,3,13): z_dims [1,1,1,7], p = 200   (configs/Sim_Hirano_Imbens.yaml)
//   (2,1, 7): z_dims [3,3,6,6], p = 100   (cli/cli.py defaults)
//   (1,3, 2): z_dims [1,1,1,7], p <= 31   (small panels / tests)
//   (2,1, 2): z_dims [3,3,6,6], p <= 31
template <int KT1_, int KSL1_, int NTL_>
struct CausalShape { static constexpr int KT1 = KT1_, KSL1 = KSL1_, NTL = NTL_; };
template <class... S>
struct CausalShapeList {};
using CausalShapes = CausalShapeList<CausalShape<1, 3, 13>, CausalShape<1, 3, 7>, CausalShape<1, 3, 2>,
                                     CausalShape<2, 1, 10>, CausalShape<2, 1, 7>, CausalShape<2, 1, 2>>;

template <class... S>
constexpr bool bgm_causal_shape_listed(CausalShapeList<S...>, int KT1, int KSL1, int NTL) {
  return (... || (S::KT1 == KT1 && S::KSL1 == KSL1 && S::NTL == NTL));
}
// every shape bgm_causal_shape (bgm_host.h) can ask for is compiled: q + 1 = 1..20 and p + 1 = 1..209 span all of its branches
constexpr bool bgm_causal_shapes_cover() {
  for (int q1 = 1; q1 <= 20; ++q1)
    for (int p1 = 1; p1 <= 209; ++p1) {
      int KT1 = 0, KSL1 = 0, NTL = 0;
      if (bgm_causal_shape(q1, p1, KT1, KSL1, NTL) && !bgm_causal_shape_listed(CausalShapes{}, KT1, KSL1, NTL)) return false;
    }
  return true;
}
static_assert(bgm_causal_shapes_cover(), "bgm_causal_shape() returns a (KT1, KSL1, NTL) that is not in CausalShapes");

// Calls f(S{}) with the listed shape S that equals (KT1, KSL1, NTL), so that S::KT1, S::KSL1, S::NTL are constants inside the generic
// lambda f, and returns f's code.  `what` names the kernel (and the path that refuses) in the error when no shape matches.
// A LEFT fold on purpose: clang instantiates the operands of a right fold last to first, which would emit a unit's kernels in the
// reverse of the table's order -- and the order of the kernels in a module changes the register allocation of some of them
// (scripts/compare_code_objects.py shows it).
template <class F, class... S>
static int bgm_causal_dispatch(CausalShapeList<S...>, int KT1, int KSL1, int NTL, const char *what, F &&f) {
  int rc = BGM_E_UNSUPPORTED;
  if (!(... || (S::KT1 == KT1 && S::KSL1 == KSL1 && S::NTL == NTL && ((rc = f(S{})), true))))
    bgm_set_error(std::string("no compiled ") + what + " variant for (KT1,KSL1,NTL)=(" + std::to_string(KT1) + "," + std::to_string(KSL1) + "," +
                  std::to_string(NTL) + ")");
  return rc;
}
template <class F>
static int bgm_causal_dispatch(const bgm_handle *h, const char *what, F &&f) {
  return bgm_causal_dispatch(CausalShapes{}, h->KT1, h->KSL1, h->NTL, what, f);
}

// The run-time effect code of a launch as the kernels' EFFECT template argument: f(std::integral_constant<int, EFFECT>) with
// 0 = transitions / draws only, 1 = ADRF, 2 = ITE, 3 = event form of the retained phase (causal_event_api.hip)
template <class F>
static int bgm_causal_with_effect(int effect, F &&f) {
  if (effect == 3) return f(std::integral_constant<int, 3>{});
  if (effect == BGM_EFFECT_ADRF) return f(std::integral_constant<int, 1>{});
  if (effect == BGM_EFFECT_ITE) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 0>{});
}

// Where f's 32 -> 8 -> 2 tail runs in the dose passes of the fused keep kernel, as the kernels' VTAILS template argument:
// f(std::true_type) = vector ALU (the default), f(std::false_type) = matrix pipe (BGM_MH_MFMA_TAILS at bgm_create)
template <class F>
static int bgm_causal_with_tails(bool valu, F &&f) {
  return valu ? f(std::true_type{}) : f(std::false_type{});
}
