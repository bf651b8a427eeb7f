// causal_hmc_tails_api.hip -- bgm_causal_hmc_run_row_tails (include/bgm_hip.h): bgm_causal_hmc_run_row_effects with the two tails of
// every (row, dose) series kept beside its moments (causal_hmc_tails_kernels.h: the TAILS instantiations of chmc_run, with and without
// the metric and the observation pattern), in a translation unit of its own, compiled beside those of the other HMC entry points.
// Prologue, preparation and the launch of a kernel with its metric twin are those of every entry point with an effect pass
// (causal_hmc_fx_host.h, causal_hmc_host.h); what is this unit's own is its argument checks and the kernels it names.
// replaces: nothing in causalbgm/base.py; its intervals are np.quantile over stored draws (:640-642, :664-666).
#include <string>

#include "causal_launch.h"
#include "causal_hmc_fx_host.h"
#include "causal_hmc_tails_kernels.h"

namespace {
const char *WHO = "bgm_causal_hmc_run_row_tails";
}  // namespace

extern "C" int bgm_causal_hmc_run_row_tails(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base,
                                            float *state, float *logp, float *grad, float *step, const float *up, const float *dn,
                                            int32_t n_table, float s_min, float s_max, int32_t init, int32_t it_begin, int32_t n_iters,
                                            int32_t burn_in, int32_t n_leapfrog, uint64_t seed, uint32_t *acc_count, float *draws,
                                            int32_t n_keep, int32_t sample_y, const float *x_values, int32_t n_doses, float *row_moments,
                                            float *row_draws, float *row_tails, int32_t k_tail, void *stream_) {
  bool go;
  if (int rc = bgm_causal_hmc_rows_begin(h, WHO, n, n_iters, "the tail-buffer kernels", x_values, n_doses, row_moments, go); rc || !go) return rc;
  const std::string who(WHO);
  if (!row_tails) { bgm_set_error(who + ": row_tails_dev required"); return BGM_E_INVALID; }
  if (k_tail < 1 || k_tail > n_keep) {
    bgm_set_error(who + ": k_tail must be in [1, n_keep] = [1, " + std::to_string(n_keep) + "]; got " + std::to_string(k_tail));
    return BGM_E_INVALID;
  }
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, BGM_CAUSAL_HMC_CALL, sample_y, n_doses, x_values, l, fx)) return rc;
  const CausalHmcTailsArgs rt{row_moments, row_draws, row_tails, k_tail};
  return bgm_causal_hmc_launch_pair(
      h, l, bgm_causal_hmc_obs_named(h->hmc_partial, "HMC kernel with per-row tails"),
      [](auto s, auto obs) {
        using S = decltype(s);
        if constexpr (decltype(obs)::value) return causal_hmc_obs_tails_kernel<S::KT1, S::KSL1, MH_WAVES>;
        else return causal_hmc_tails_kernel<S::KT1, S::KSL1, MH_WAVES>;
      },
      [](auto s, auto obs) {
        using S = decltype(s);
        if constexpr (decltype(obs)::value) return causal_hmc_obs_mass_tails_kernel<S::KT1, S::KSL1, MH_WAVES>;
        else return causal_hmc_mass_tails_kernel<S::KT1, S::KSL1, MH_WAVES>;
      }, fx, rt);
}
