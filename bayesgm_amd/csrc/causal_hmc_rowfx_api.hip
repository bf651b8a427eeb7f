// causal_hmc_rowfx_api.hip -- bgm_causal_hmc_run_row_effects (include/bgm_hip.h): the CausalBGM HMC latent sampler with the
// dose-response of every row kept inside the retained iterations (causal_hmc_rowfx_kernels.h: the ROWS instantiations of chmc_run),
// in a translation unit of its own, compiled beside those of the other HMC entry points.
// replaces: nothing in causalbgm/base.py; infer_from_latent_posterior (:671-763) averages y_i(x_k) over the rows of the panel.
#include <string>

#include "causal_launch.h"
#include "causal_hmc_fx_host.h"
#include "causal_hmc_rowfx_kernels.h"
#include "causal_hmc_obs_host.h"

namespace {
const char *WHO = "bgm_causal_hmc_run_row_effects";
}  // namespace

extern "C" int bgm_causal_hmc_run_row_effects(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base,
                                              float *state, float *logp, float *grad, float *step, const float *up, const float *dn,
                                              int32_t n_table, float s_min, float s_max, int32_t init, int32_t it_begin, int32_t n_iters,
                                              int32_t burn_in, int32_t n_leapfrog, uint64_t seed, uint32_t *acc_count, float *draws,
                                              int32_t n_keep, int32_t sample_y, const float *x_values, int32_t n_doses, float *row_moments,
                                              float *row_draws, void *stream_) {
  if (int rc = bgm_causal_hmc_check(h, WHO)) return rc;
  if (n <= 0 || n_iters <= 0) return BGM_OK;
  const std::string who(WHO);
  if (h->cfg.binary_treatment != 0) {
    bgm_set_error(who + ": a binary treatment has its per-row effect already: bgm_causal_hmc_run_effects (BGM_EFFECT_ITE)");
    return BGM_E_INVALID;
  }
  if (!x_values || n_doses <= 0 || !row_moments) { bgm_set_error(who + ": x_values / row_moments required"); return BGM_E_INVALID; }
  const CausalHmcCall call{x, y, v, n, row_base, state, logp, grad, step, up, dn, n_table, s_min, s_max, init, it_begin, n_iters, burn_in,
                           n_leapfrog, seed, acc_count, draws, n_keep, (hipStream_t)stream_};
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, call, l, fx)) return rc;
  fx.sample_y = sample_y; fx.n_doses = n_doses; fx.x_values = x_values;
  const CausalHmcRowFxArgs rf{row_moments, row_draws};
  if (l.st->traj_set()) return bgm_causal_hmc_traj_rowfx_launch(h, l, fx, rf);      // bgm_causal_hmc_set_trajectory
  if (h->hmc_partial) return bgm_causal_hmc_obs_rowfx_launch(h, l, fx, rf);      // bgm_causal_hmc_set_partial
  return bgm_causal_hmc_dispatch(h, l.st, "HMC kernel with per-row effects", [&](auto s, auto metric) {
    using S = decltype(s);
    if constexpr (decltype(metric)::value)
      return bgm_launch(causal_hmc_mass_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, l.st->mass, fx, rf);
    else
      return bgm_launch(causal_hmc_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, fx, rf);
  });
}
