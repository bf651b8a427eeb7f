// causal_hmc_contrast_api.hip -- bgm_causal_hmc_run_row_contrasts (include/bgm_hip.h): bgm_causal_hmc_run_row_effects with the
// difference of every dose to the baseline dose (dose 0) kept beside the curve, and, optionally, its draws and its two tails
// (causal_hmc_contrast_kernels.h: the CONTRAST instantiations of chmc_run, with and without the metric, the observation pattern and
// the tails), in a translation unit of its own, compiled beside those of the other HMC entry points.
// replaces: nothing in causalbgm/base.py; the reference has no per-row quantity for a continuous treatment.
#include <string>

#include "causal_launch.h"
#include "causal_hmc_fx_host.h"
#include "causal_hmc_contrast_kernels.h"

namespace {
const char *WHO = "bgm_causal_hmc_run_row_contrasts";

template <bool OBS, bool TAILS>
int launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, const CausalHmcContrastArgs &rc) {
  std::string what = TAILS ? "HMC kernel with per-row dose contrasts and their tails" : "HMC kernel with per-row dose contrasts";
  if (OBS) what += " for partially observed rows";
  return bgm_causal_hmc_dispatch(h, l.st, what, [&](auto s, auto metric) {
    using S = decltype(s);
    if constexpr (decltype(metric)::value)
      return bgm_launch(causal_hmc_mass_contrast_kernel<S::KT1, S::KSL1, MH_WAVES, OBS, TAILS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka,
                        l.st->mass, fx, rc);
    else
      return bgm_launch(causal_hmc_contrast_kernel<S::KT1, S::KSL1, MH_WAVES, OBS, TAILS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, fx, rc);
  });
}
}  // namespace

extern "C" int bgm_causal_hmc_run_row_contrasts(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base,
                                                float *state, float *logp, float *grad, float *step, const float *up, const float *dn,
                                                int32_t n_table, float s_min, float s_max, int32_t init, int32_t it_begin, int32_t n_iters,
                                                int32_t burn_in, int32_t n_leapfrog, uint64_t seed, uint32_t *acc_count, float *draws,
                                                int32_t n_keep, int32_t sample_y, const float *x_values, int32_t n_doses, float *row_moments,
                                                float *row_cmoments, float *contrast_draws, float *contrast_tails, int32_t k_tail,
                                                void *stream_) {
  if (int rc = bgm_causal_hmc_check(h, WHO)) return rc;
  if (n <= 0 || n_iters <= 0) return BGM_OK;
  if (int rc = bgm_causal_hmc_traj_refuse(h, WHO, "the dose-contrast kernels")) return rc;
  const std::string who(WHO);
  if (h->cfg.binary_treatment != 0) {
    bgm_set_error(who + ": a binary treatment has its per-row effect already: bgm_causal_hmc_run_effects (BGM_EFFECT_ITE)");
    return BGM_E_INVALID;
  }
  if (!x_values || n_doses <= 0 || !row_moments) { bgm_set_error(who + ": x_values / row_moments required"); return BGM_E_INVALID; }
  if (!row_cmoments) { bgm_set_error(who + ": row_cmoments_dev required"); return BGM_E_INVALID; }
  if (contrast_tails && (k_tail < 1 || k_tail > n_keep)) {
    bgm_set_error(who + ": k_tail must be in [1, n_keep] = [1, " + std::to_string(n_keep) + "]; got " + std::to_string(k_tail));
    return BGM_E_INVALID;
  }
  const CausalHmcCall call{x, y, v, n, row_base, state, logp, grad, step, up, dn, n_table, s_min, s_max, init, it_begin, n_iters, burn_in,
                           n_leapfrog, seed, acc_count, draws, n_keep, (hipStream_t)stream_};
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, call, l, fx)) return rc;
  fx.sample_y = sample_y; fx.n_doses = n_doses; fx.x_values = x_values;
  const CausalHmcContrastArgs rc{row_moments, row_cmoments, contrast_draws, contrast_tails, contrast_tails ? k_tail : 0};
  const bool partial = h->hmc_partial;                                           // bgm_causal_hmc_set_partial
  if (contrast_tails) return partial ? launch<true, true>(h, l, fx, rc) : launch<false, true>(h, l, fx, rc);
  return partial ? launch<true, false>(h, l, fx, rc) : launch<false, false>(h, l, fx, rc);
}
