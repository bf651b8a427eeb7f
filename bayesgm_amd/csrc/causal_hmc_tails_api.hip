// causal_hmc_tails_api.hip -- bgm_causal_hmc_run_row_tails (include/bgm_hip.h): bgm_causal_hmc_run_row_effects with the two tails of
// every (row, dose) series kept beside its moments (causal_hmc_tails_kernels.h: the TAILS instantiations of chmc_run, with and without
// the metric and the observation pattern), in a translation unit of its own, compiled beside those of the other HMC entry points.
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
  if (int rc = bgm_causal_hmc_check(h, WHO)) return rc;
  if (n <= 0 || n_iters <= 0) return BGM_OK;
  if (int rc = bgm_causal_hmc_traj_refuse(h, WHO, "the tail-buffer kernels")) return rc;
  const std::string who(WHO);
  if (h->cfg.binary_treatment != 0) {
    bgm_set_error(who + ": a binary treatment has its per-row effect already: bgm_causal_hmc_run_effects (BGM_EFFECT_ITE)");
    return BGM_E_INVALID;
  }
  if (!x_values || n_doses <= 0 || !row_moments) { bgm_set_error(who + ": x_values / row_moments required"); return BGM_E_INVALID; }
  if (!row_tails) { bgm_set_error(who + ": row_tails_dev required"); return BGM_E_INVALID; }
  if (k_tail < 1 || k_tail > n_keep) {
    bgm_set_error(who + ": k_tail must be in [1, n_keep] = [1, " + std::to_string(n_keep) + "]; got " + std::to_string(k_tail));
    return BGM_E_INVALID;
  }
  const CausalHmcCall call{x, y, v, n, row_base, state, logp, grad, step, up, dn, n_table, s_min, s_max, init, it_begin, n_iters, burn_in,
                           n_leapfrog, seed, acc_count, draws, n_keep, (hipStream_t)stream_};
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, call, l, fx)) return rc;
  fx.sample_y = sample_y; fx.n_doses = n_doses; fx.x_values = x_values;
  const CausalHmcTailsArgs rt{row_moments, row_draws, row_tails, k_tail};
  const bool partial = h->hmc_partial;                                           // bgm_causal_hmc_set_partial
  return bgm_causal_hmc_dispatch(h, l.st, partial ? "HMC kernel with per-row tails for partially observed rows" : "HMC kernel with per-row tails",
                                 [&](auto s, auto metric) {
    using S = decltype(s);
    if constexpr (decltype(metric)::value) {
      if (partial)
        return bgm_launch(causal_hmc_obs_mass_tails_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, l.st->mass, fx, rt);
      return bgm_launch(causal_hmc_mass_tails_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, l.st->mass, fx, rt);
    } else {
      if (partial) return bgm_launch(causal_hmc_obs_tails_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, fx, rt);
      return bgm_launch(causal_hmc_tails_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, fx, rt);
    }
  });
}
