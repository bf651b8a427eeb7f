// bgm_launch.h -- host-side dispatch of the dual-access-blob BGM kernels (bgm_kernels.h, bgm_fit_kernels.h), shared by the translation
// units that instantiate them (bgm_api.hip, fit_api.hip): the table of compiled variants, the proof that bgm_layout (bgm_state.h) can ask
// for no other, and the dispatch from a state's variant to a template instantiation.  The launch itself is bgm_launch (bgm_host.h).
// Host only: no kernel lives here, and which kernels a unit instantiates is decided by the lambdas it passes to bgm_bgm_dispatch.
#pragma once
#include <string>
#include <utility>

#include "bgm_state.h"

// ---- waves per workgroup of the posterior kernels, shared by the units that instantiate them (bgm_api.hip, bgm_rowstep_api.hip)
static constexpr int BGM_WAVES = 8;
#ifndef BGM_WAVES_WIDE_HMC
#define BGM_WAVES_WIDE_HMC 12   // 148 VGPRs -> 3 waves/SIMD; measured 89 vs 86 (8) vs 86 (16) TF at p=500
#endif
#ifndef BGM_SX3_WAVES_DEFAULT
#define BGM_SX3_WAVES_DEFAULT 12      // ms per transition at N = 2e5, p = 500: 3.43 (8 waves, no spill) / 3.19 (12 waves, 168 registers); two 6-wave workgroups per CU: 4.0; two / three / four units per stream step: 3.12 / 3.24 / 3.34
#endif
// the posterior blob of the handle's current weights and precision, packed and uploaded when it is not current (bgm_api.hip)
int bgm_bgm_build_blob(bgm_handle *h, hipStream_t stream);

// ---- compiled variants.  (KTQ, NTX, NH): z_dim <= 16; x_dim in (16, 32] / (96, 112] LDS-resident, NTX = 0 = wide (any x_dim, head weights
// streamed through an LDS stage); 5 hidden layers (configs/*.yaml) or 3.  Split precision is always the streamed variant.
template <int KTQ_, int NTX_, int NH_>
struct BgmVariant { static constexpr int KTQ = KTQ_, NTX = NTX_, NH = NH_; };
template <class... V>
struct BgmVariantList {};
using BgmVariants = BgmVariantList<BgmVariant<1, 2, 5>, BgmVariant<1, 7, 5>, BgmVariant<1, 0, 5>,
                                   BgmVariant<1, 2, 3>, BgmVariant<1, 7, 3>, BgmVariant<1, 0, 3>>;
using BgmSx3Variants = BgmVariantList<BgmVariant<1, 0, 5>, BgmVariant<1, 0, 3>>;

template <class... V>
constexpr bool bgm_bgm_variant_listed(BgmVariantList<V...>, int KTQ, int NTX, int NH) {
  return (... || (V::KTQ == KTQ && V::NTX == NTX && V::NH == NH));
}
// every variant bgm_layout can choose for a shape that gxb_wanted() (gx_bgm_api.hip) leaves on this path is compiled: z_dim q = 1..16,
// 3 or 5 hidden layers, the streamed variant forced (BGM_FORCE_WIDE, split precision) or not, x_dim p from 1 to the first width that no
// layout holds -- every width to 512 (the heads of 19 tiles, p > 288, already exceed the LDS, so no resident variant can lie beyond),
// then the last width of every 16-feature block, since the layout reads p only as ceil(p / 16).  (Every width to the end, some 13 800 at
// NH = 3, is 720 000 evaluations: a minute of compile time per pass.)  One constant per (q, NH, forced): each is a constant evaluation of its own,
// inside the compiler's step limit.
constexpr bool bgm_bgm_variants_cover(int q, int NH, bool force_wide) {
  for (int p = 1;; p += p < 512 ? 1 : 16) {
    BgmMeta m{};
    int ntx = 0;
    if (bgm_layout_at(q, p, NH, force_wide, m, ntx) < 0) return true;
    if (!bgm_bgm_variant_listed(BgmVariants{}, (q + 15) / 16, ntx, NH)) return false;
  }
}
template <int Q, int NH, bool FORCE_WIDE>
constexpr bool bgm_bgm_covered = bgm_bgm_variants_cover(Q, NH, FORCE_WIDE);
template <int... Q0>
constexpr bool bgm_bgm_all_covered(std::integer_sequence<int, Q0...>) {
  return (... && (bgm_bgm_covered<Q0 + 1, 3, false> && bgm_bgm_covered<Q0 + 1, 3, true> && bgm_bgm_covered<Q0 + 1, 5, false> && bgm_bgm_covered<Q0 + 1, 5, true>));
}
#ifndef __HIP_DEVICE_COMPILE__      // (once per unit: the host pass)
static_assert(bgm_bgm_all_covered(std::make_integer_sequence<int, 16>{}), "bgm_layout() returns a (KTQ, NTX, NH) that is not in BgmVariants");
#endif

// Calls f(V{}) with the listed variant V that equals (KTQ, NTX, NH), so that V::KTQ, V::NTX, V::NH are constants inside the generic
// lambda f, and returns f's code.  `what` names the kernel in the error when no variant matches.  A left fold, as in causal_launch.h:
// a right fold would emit a unit's kernels in the reverse of the table's order, and that order changes their register allocation.
template <class F, class... V>
static int bgm_bgm_dispatch(BgmVariantList<V...>, int KTQ, int NTX, int NH, const char *what, F &&f) {
  int rc = BGM_E_UNSUPPORTED;
  if (!(... || (V::KTQ == KTQ && V::NTX == NTX && V::NH == NH && ((rc = f(V{})), true))))
    bgm_set_error(std::string("no compiled ") + what + " variant for (KTQ,NTX,NH)=(" + std::to_string(KTQ) + "," + std::to_string(NTX) + "," +
                  std::to_string(NH) + ")");
  return rc;
}
template <class F>
static int bgm_bgm_dispatch(const BgmState *s, const char *what, F &&f) {
  return bgm_bgm_dispatch(BgmVariants{}, s->KTQ, s->NTX, s->NH, what, f);
}
