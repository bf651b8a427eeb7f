// causal_hmc_rowfx_api.hip -- bgm_causal_hmc_run_row_effects (include/bgm_hip.h): the CausalBGM HMC latent sampler with the
// dose-response of every row kept inside the retained iterations (causal_hmc_rowfx_kernels.h: the ROWS instantiations of chmc_run),
// in a translation unit of its own, compiled beside those of the other HMC entry points.  Prologue and preparation are those of
// every per-row entry point (causal_hmc_fx_host.h); this one has TRAJ and OBS twins, launched from their own units.
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
  bool go;
  if (int rc = bgm_causal_hmc_rows_begin(h, WHO, n, n_iters, nullptr, x_values, n_doses, row_moments, go); rc || !go) return rc;
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, BGM_CAUSAL_HMC_CALL, sample_y, n_doses, x_values, l, fx)) return rc;
  const CausalHmcRowFxArgs rf{row_moments, row_draws};
  if (l.st->traj_set()) return bgm_causal_hmc_traj_rowfx_launch(h, l, fx, rf);      // bgm_causal_hmc_set_trajectory
  if (h->hmc_partial) return bgm_causal_hmc_obs_rowfx_launch(h, l, fx, rf);      // bgm_causal_hmc_set_partial
  return bgm_causal_hmc_launch_pair(
      h, l, "HMC kernel with per-row effects",
      [](auto s) { using S = decltype(s); return causal_hmc_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES>; },
      [](auto s) { using S = decltype(s); return causal_hmc_mass_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES>; }, fx, rf);
}
