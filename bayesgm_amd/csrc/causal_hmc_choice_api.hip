// causal_hmc_choice_api.hip -- bgm_causal_hmc_run_row_choice (include/bgm_hip.h): bgm_causal_hmc_run_row_effects with the choice among
// the doses kept beside the curve -- per row, how often every dose was the best of a retained draw, the best value's shifted sum and,
// optionally, how often every dose exceeded a threshold (causal_hmc_choice_kernels.h: the CHOICE instantiations of chmc_run, with and
// without the metric and the observation pattern; ONE of the eight combinations per shape is not built and is refused, see launch), in
// a translation unit of its own, compiled beside those of the other HMC entry points.
// Prologue, preparation and the launch of a kernel with its metric twin are those of every entry point with an effect pass
// (causal_hmc_fx_host.h, causal_hmc_host.h); what is this unit's own is its argument checks and the kernels it names.
// replaces: nothing in causalbgm/base.py; the reference has no per-row quantity for a continuous treatment.
#include <cmath>
#include <string>

#include "causal_launch.h"
#include "causal_hmc_fx_host.h"
#include "causal_hmc_choice_kernels.h"

namespace {
const char *WHO = "bgm_causal_hmc_run_row_choice";

template <bool OBS>
int launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, const CausalHmcChoiceArgs &rc) {
  const std::string what = bgm_causal_hmc_obs_named(OBS, "HMC kernel with per-row dose choice");
  return bgm_causal_hmc_launch_pair(
      h, l, what, [](auto s) { using S = decltype(s); return causal_hmc_choice_kernel<S::KT1, S::KSL1, MH_WAVES, OBS>; },
      [&](auto s) {
        using S = decltype(s);
        // Not shipped: the metric with the observation pattern at KT1 = 2.  hipcc gives that instantiation 256 VGPRs and 12 bytes of
        // scratch, whatever the choice block looks like; the other seven have none.
        if constexpr (OBS && S::KT1 == 2) {
          bgm_set_error(std::string(WHO) + ": no " + what + ", with a diagonal metric, at more than 11 latent features (KT1 = 2): it cannot be "
                        "had without scratch memory at two waves per SIMD; run it without the metric, or use "
                        "bgm_causal_hmc_run_row_effects with row_draws_dev");
          return (int)BGM_E_UNSUPPORTED;
        } else {
          return causal_hmc_mass_choice_kernel<S::KT1, S::KSL1, MH_WAVES, OBS>;
        }
      }, fx, rc);
}
}  // namespace

extern "C" int bgm_causal_hmc_run_row_choice(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base,
                                             float *state, float *logp, float *grad, float *step, const float *up, const float *dn,
                                             int32_t n_table, float s_min, float s_max, int32_t init, int32_t it_begin, int32_t n_iters,
                                             int32_t burn_in, int32_t n_leapfrog, uint64_t seed, uint32_t *acc_count, float *draws,
                                             int32_t n_keep, int32_t sample_y, const float *x_values, int32_t n_doses, float *row_moments,
                                             float *row_draws, uint32_t *best_count, float *best_moments, uint32_t *above_count,
                                             float threshold, int32_t maximize, void *stream_) {
  bool go;
  if (int rc = bgm_causal_hmc_rows_begin(h, WHO, n, n_iters, "the dose-choice kernels", x_values, n_doses, row_moments, go); rc || !go) return rc;
  const std::string who(WHO);
  if (!best_count) { bgm_set_error(who + ": best_count_dev required"); return BGM_E_INVALID; }
  if (!best_moments) { bgm_set_error(who + ": best_moments_dev required"); return BGM_E_INVALID; }
  if (above_count && !std::isfinite(threshold)) {
    bgm_set_error(who + ": threshold must be finite when above_count_dev is given");
    return BGM_E_INVALID;
  }
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, BGM_CAUSAL_HMC_CALL, sample_y, n_doses, x_values, l, fx)) return rc;
  const CausalHmcChoiceArgs rc{row_moments, row_draws, CausalChoiceArgs{best_count, best_moments, above_count, maximize ? 1.0f : -1.0f,
                                                                         above_count ? threshold : 0.0f}};
  return bgm_causal_hmc_with_pattern(h, [&](auto obs) { return launch<decltype(obs)::value>(h, l, fx, rc); });
}
