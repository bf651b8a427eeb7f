// causal_rowadapt_api.hip -- the CausalBGM MH kernels with a proposal scale per chain, adapted by that chain alone during burn-in
// (bgm_causal_set_row_scale, include/bgm_hip.h): the ROWADAPT = true instantiations of causal_mh_kernel (causal_kernels.h) for the
// fp32 LDS-resident shapes with the standard-normal prior -- burn-in / draws, ADRF, ITE and the event form's transitions, direct and
// Gram likelihood -- kept in their own translation unit.  The default path (causal_api.hip) is untouched.
// replaces: the block-wide q_sd *= 0.9 / 1.1 of metropolis_hastings_sampler (causalbgm/base.py:880-893), opt-in.
#include <cmath>
#include <string>

#include "bgm_host.h"

// the launch geometry of bgm_causal_mh_run (causal_api.hip sizes the grid, the slot-private counters, the ADRF partial sums and the event
// regions with BGM_MH_WAVES waves per workgroup and BGM_MH_R row tiles per wave): the same build options, one row tile per wave
#ifndef BGM_MH_R
#define BGM_MH_R 1
#endif
#ifndef BGM_MH_WAVES
#define BGM_MH_WAVES 8
#endif
static constexpr int RA_WAVES = BGM_MH_WAVES;
// (the kernels are instantiated with one row tile per wave; a build with BGM_MH_R != 1 is refused by bgm_causal_mh_run before it gets here)
#define BGM_ROWADAPT_VARIANTS(X) X(1, 3, 13) X(1, 3, 7) X(1, 3, 2) X(2, 1, 10) X(2, 1, 7) X(2, 1, 2)

extern "C" int bgm_causal_set_row_scale(bgm_handle *h, float *scale_dev, const float *up_dev, const float *dn_dev, int32_t n_table,
                                        float s_min, float s_max) {
  if (!h) { bgm_set_error("bgm_causal_set_row_scale: NULL handle"); return BGM_E_INVALID; }
  if (!scale_dev) {
    h->ra_scale = nullptr; h->ra_up = h->ra_dn = nullptr; h->ra_n = 0; h->ra_min = h->ra_max = 0.0f;
    return BGM_OK;
  }
  if (n_table < 0 || (n_table > 0 && (!up_dev || !dn_dev))) { bgm_set_error("bgm_causal_set_row_scale: up_dev / dn_dev must hold n_table >= 0 factors"); return BGM_E_INVALID; }
  if (!(s_min > 0.0f) || !(s_max >= s_min) || !std::isfinite(s_max)) { bgm_set_error("bgm_causal_set_row_scale: the clamp needs 0 < s_min <= s_max < inf"); return BGM_E_INVALID; }
  h->ra_scale = scale_dev; h->ra_up = up_dev; h->ra_dn = dn_dev; h->ra_n = n_table; h->ra_min = s_min; h->ra_max = s_max;
  return BGM_OK;
}

template <class K>
static int ra_set_lds(K kernel, int bytes) {
  BGM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return BGM_OK;
}

template <int EFFECT>
static int ra_launch_mh(bgm_handle *h, const CausalMhKArgs &ka, int grid, int lds, hipStream_t stream) {
  int rc;
#define X(KT1_, KSL1_, NTL_)                                                                          \
  if (h->KT1 == KT1_ && h->KSL1 == KSL1_ && h->NTL == NTL_) {                                         \
    auto k = ka.uc ? causal_mh_kernel<KT1_, KSL1_, NTL_, 1, RA_WAVES, EFFECT, 0, (NTL_ > 2), true>    \
                   : causal_mh_kernel<KT1_, KSL1_, NTL_, 1, RA_WAVES, EFFECT, 0, false, true>;        \
    rc = ra_set_lds(k, lds);                                                                          \
    if (rc) return rc;                                                                                \
    hipLaunchKernelGGL(k, dim3(grid), dim3(64 * RA_WAVES), lds, stream, ka);                          \
    BGM_HIP_CHECK(hipGetLastError());                                                                 \
    return BGM_OK;                                                                                    \
  }
  BGM_ROWADAPT_VARIANTS(X)
#undef X
  bgm_set_error("per-chain proposal scale: no compiled MH kernel variant for this shape");
  return BGM_E_UNSUPPORTED;
}

int bgm_causal_rowadapt_mh_launch(bgm_handle *h, const CausalMhKArgs &ka, int effect, int grid, int lds, hipStream_t stream) {
  if (!ka.row_scale || ka.seg) { bgm_set_error("per-chain proposal scale: launched without a scale buffer / with a conditional prior"); return BGM_E_STATE; }
  if (effect == 3) return ra_launch_mh<3>(h, ka, grid, lds, stream);         // event form of the retained phase (causal_event_api.hip)
  if (effect == BGM_EFFECT_ADRF) return ra_launch_mh<1>(h, ka, grid, lds, stream);
  if (effect == BGM_EFFECT_ITE) return ra_launch_mh<2>(h, ka, grid, lds, stream);
  return ra_launch_mh<0>(h, ka, grid, lds, stream);
}
