// causal_rowadapt_api.hip -- the CausalBGM MH kernels with a proposal scale per chain, adapted by that chain alone during burn-in
// (bgm_causal_set_row_scale, include/bgm_hip.h): the ROWADAPT = true instantiations of causal_mh_kernel (causal_kernels.h) for the
// fp32 LDS-resident shapes with the standard-normal prior -- burn-in / draws, ADRF, ITE and the event form's transitions, direct and
// Gram likelihood -- kept in their own translation unit.  The default path (causal_api.hip) is untouched.
// replaces: the block-wide q_sd *= 0.9 / 1.1 of metropolis_hastings_sampler (causalbgm/base.py:880-893), opt-in.
#include <cmath>
#include <string>

#include "causal_launch.h"

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

int bgm_causal_rowadapt_mh_launch(bgm_handle *h, const CausalMhKArgs &ka, int effect, int grid, int lds, hipStream_t stream) {
  if (!ka.row_scale || ka.seg) { bgm_set_error("per-chain proposal scale: launched without a scale buffer / with a conditional prior"); return BGM_E_STATE; }
  return bgm_causal_with_effect(effect, [&](auto e) {
    return bgm_causal_dispatch(h, "per-chain proposal scale: MH kernel", [&](auto s) {
      using S = decltype(s);
      constexpr int EFFECT = decltype(e)::value;
      return bgm_causal_with_tails(EFFECT == 1 && !h->mh_mfma_tails, [&](auto vt) {      // (as in causal_api.hip, launch_mh)
        constexpr bool VT = EFFECT == 1 && decltype(vt)::value;
        constexpr bool VT_G = VT && causal_valu_tails(S::KT1, S::NTL, S::NTL > 2, true), VT_D = VT && causal_valu_tails(S::KT1, S::NTL, false, true);
        return bgm_launch(ka.uc ? causal_mh_kernel<S::KT1, S::KSL1, S::NTL, MH_R, MH_WAVES, EFFECT, 0, (S::NTL > 2), true, VT_G>
                                : causal_mh_kernel<S::KT1, S::KSL1, S::NTL, MH_R, MH_WAVES, EFFECT, 0, false, true, VT_D>,
                          grid, MH_WAVES, lds, stream, ka);
      });
    });
  });
}
