// causal_hmc_traj_api.hip -- bgm_causal_hmc_set_trajectory (include/bgm_hip.h) and the launches of the CausalBGM HMC kernels with a
// number of leapfrog steps per chain and iteration (causal_hmc_traj_kernels.h: the TRAJ instantiations of chmc_run), in a translation
// unit of their own, compiled beside those of the other HMC entry points: bgm_causal_hmc_run, bgm_causal_hmc_run_effects and
// bgm_causal_hmc_run_row_effects come here only while an option is set, after their own argument checks.
// replaces: nothing in causalbgm/base.py; the options are max_trajectory / jitter_leapfrog of the BGM imputation sampler here.
#include <cmath>
#include <string>

#include "causal_launch.h"
#include "causal_hmc_host.h"
#include "causal_hmc_traj_kernels.h"

extern "C" int bgm_causal_hmc_set_trajectory(bgm_handle *h, float max_trajectory, int32_t jitter, int32_t *n_steps_dev) {
  const std::string who("bgm_causal_hmc_set_trajectory");
  if (!h) { bgm_set_error(who + ": NULL handle"); return BGM_E_INVALID; }
  if (!(max_trajectory >= 0.0f) || !std::isfinite(max_trajectory)) {
    bgm_set_error(who + ": max_trajectory must be finite and >= 0 (0: no cap); got " + std::to_string(max_trajectory));
    return BGM_E_INVALID;
  }
  if (jitter != 0 && jitter != 1) { bgm_set_error(who + ": jitter must be 0 or 1; got " + std::to_string(jitter)); return BGM_E_INVALID; }
  if (max_trajectory == 0.0f && !jitter && !n_steps_dev) {      // back to the kernels without TRAJ
    if (h->hmc_state) static_cast<HmcState *>(h->hmc_state)->traj = CausalHmcTrajArgs{};
    return BGM_OK;
  }
  if (int rc = bgm_causal_hmc_check(h, who.c_str())) return rc;
  CausalHmcTrajArgs &tj = bgm_causal_hmc_state(h)->traj;
  tj.max_traj = max_trajectory; tj.jitter = jitter; tj.n_steps = n_steps_dev;
  return BGM_OK;
}

int bgm_causal_hmc_traj_refuse(const bgm_handle *h, const char *who, const char *kernels) {
  const CausalHmcTrajArgs *tj = bgm_causal_hmc_traj(h);
  if (!tj) return BGM_OK;
  bgm_set_error(std::string(who) + ": " + kernels + " have no variant with a trajectory length per chain (bgm_causal_hmc_set_trajectory: " +
                (tj->max_traj > 0.0f ? "max_trajectory" : tj->jitter ? "jitter" : "n_steps_dev") +
                " is set); clear it with (0, 0, NULL) or use bgm_causal_hmc_run, bgm_causal_hmc_run_effects or bgm_causal_hmc_run_row_effects");
  return BGM_E_UNSUPPORTED;
}

namespace {

std::string named(const bgm_handle *h, const char *what) {
  return std::string(what) + " with a trajectory length per chain" + (h->hmc_partial ? " for partially observed rows" : "");
}

// f(std::bool_constant<OBS>) by the handle's observation pattern (bgm_causal_hmc_set_partial)
template <class F>
int with_pattern(const bgm_handle *h, F &&f) {
  return h->hmc_partial ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace

int bgm_causal_hmc_traj_launch(bgm_handle *h, const CausalHmcLaunch &l) {
  const CausalHmcTrajArgs &tj = l.st->traj;
  return bgm_causal_hmc_dispatch(h, l.st, named(h, "HMC kernel"), [&](auto s, auto metric) {
    using S = decltype(s);
    return with_pattern(h, [&](auto obs) {
      constexpr bool OBS = decltype(obs)::value;
      if constexpr (decltype(metric)::value)
        return bgm_launch(causal_hmc_traj_mass_kernel<S::KT1, MH_WAVES, OBS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, l.st->mass, tj);
      else
        return bgm_launch(causal_hmc_traj_kernel<S::KT1, MH_WAVES, OBS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, tj);
    });
  });
}

namespace {

template <int EFFECT, bool OBS>
int launch_fx(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx) {
  const CausalHmcTrajArgs &tj = l.st->traj;
  return bgm_causal_hmc_dispatch(h, l.st, named(h, "HMC kernel with fused effects"), [&](auto s, auto metric) {
    using S = decltype(s);
    if constexpr (decltype(metric)::value)
      return bgm_launch(causal_hmc_traj_mass_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT, OBS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka,
                        l.st->mass, fx, tj);
    else
      return bgm_launch(causal_hmc_traj_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT, OBS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, fx, tj);
  });
}

}  // namespace

// (the panel's dose-response with the observation pattern was refused by the entry point: it has no OBS kernel at all)
int bgm_causal_hmc_traj_fx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, bool binary) {
  if (!binary) return launch_fx<1, false>(h, l, fx);
  return h->hmc_partial ? launch_fx<2, true>(h, l, fx) : launch_fx<2, false>(h, l, fx);
}

int bgm_causal_hmc_traj_rowfx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, const CausalHmcRowFxArgs &rf) {
  const CausalHmcTrajArgs &tj = l.st->traj;
  return bgm_causal_hmc_dispatch(h, l.st, named(h, "HMC kernel with per-row effects"), [&](auto s, auto metric) {
    using S = decltype(s);
    return with_pattern(h, [&](auto obs) {
      constexpr bool OBS = decltype(obs)::value;
      if constexpr (decltype(metric)::value)
        return bgm_launch(causal_hmc_traj_mass_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES, OBS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka,
                          l.st->mass, fx, rf, tj);
      else
        return bgm_launch(causal_hmc_traj_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES, OBS>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, fx, rf, tj);
    });
  });
}
