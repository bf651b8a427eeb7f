// causal_hmc_fx_api.hip -- bgm_causal_hmc_run_effects (include/bgm_hip.h): the CausalBGM HMC latent sampler with the effect pass
// fused into the retained iterations (the EFFECT 1 / 2 instantiations of chmc_run, causal_hmc_fx_kernels.h), in a translation unit
// of its own, compiled beside the others: bgm_causal_hmc_run (causal_hmc_api.hip, causal_hmc_mass_api.hip) never comes here.
// Prologue, preparation and the launch of a kernel with its metric twin are those of every entry point with an effect pass
// (causal_hmc_fx_host.h, causal_hmc_host.h); what is this unit's own is its argument checks and the kernels it names.
// replaces: nothing in causalbgm/base.py; infer_from_latent_posterior (:671-763) runs there on stored MH draws.
#include <string>

#include "causal_launch.h"
#include "causal_hmc_fx_host.h"
#include "causal_hmc_obs_host.h"

namespace {

const char *WHO = "bgm_causal_hmc_run_effects";

template <int EFFECT>
int launch_fx(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx) {
  return bgm_causal_hmc_launch_pair(
      h, l, "HMC kernel with fused effects", [](auto s) { using S = decltype(s); return causal_hmc_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT>; },
      [](auto s) { using S = decltype(s); return causal_hmc_mass_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT>; }, fx);
}

}  // namespace

extern "C" int bgm_causal_hmc_run_effects(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base,
                                          float *state, float *logp, float *grad, float *step, const float *up, const float *dn,
                                          int32_t n_table, float s_min, float s_max, int32_t init, int32_t it_begin, int32_t n_iters,
                                          int32_t burn_in, int32_t n_leapfrog, uint64_t seed, uint32_t *acc_count, float *draws,
                                          int32_t n_keep, int32_t sample_y, const float *x_values, int32_t n_doses, float *adrf_partial,
                                          float *ite, void *stream_) {
  bool go;
  if (int rc = bgm_causal_hmc_begin(h, WHO, n, n_iters, nullptr, go); rc || !go) return rc;
  const std::string who(WHO);
  const bool binary = h->cfg.binary_treatment != 0;
  if (h->hmc_partial && !binary) {
    bgm_set_error(who + ": the panel's dose-response has no kernel for partially observed rows (bgm_causal_hmc_set_partial); the "
                        "per-row dose-response has: bgm_causal_hmc_run_row_effects");
    return BGM_E_UNSUPPORTED;
  }
  if (binary && !ite) { bgm_set_error(who + ": ite_dev required for binary treatment"); return BGM_E_INVALID; }
  if (!binary && (!x_values || n_doses <= 0 || !adrf_partial)) { bgm_set_error(who + ": x_values / adrf_partial required"); return BGM_E_INVALID; }
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, BGM_CAUSAL_HMC_CALL, sample_y, binary ? 2 : n_doses, x_values, l, fx)) return rc;
  fx.adrf_partial = adrf_partial; fx.ite = ite;
  if (l.st->traj_set()) return bgm_causal_hmc_traj_fx_launch(h, l, fx, binary);      // bgm_causal_hmc_set_trajectory
  if (h->hmc_partial) return bgm_causal_hmc_obs_ite_launch(h, l, fx);      // (binary: checked above)
  return binary ? launch_fx<2>(h, l, fx) : launch_fx<1>(h, l, fx);
}
