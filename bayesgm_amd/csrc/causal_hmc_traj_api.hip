// causal_hmc_traj_api.hip -- bgm_causal_hmc_set_trajectory (include/bgm_hip.h) and the launches of the CausalBGM HMC kernels with a
// number of leapfrog steps per chain and iteration (causal_hmc_traj_kernels.h: the TRAJ instantiations of chmc_run), in a translation
// unit of their own, compiled beside those of the other HMC entry points: bgm_causal_hmc_run, bgm_causal_hmc_run_effects and
// bgm_causal_hmc_run_row_effects come here only while an option is set, after their own argument checks.
// Each launch is bgm_causal_hmc_launch_pair (causal_hmc_host.h) with the two kernels of this unit that it names; those that take
// the observation pattern's tag have their OBS twins here too and are chosen by the handle's pattern inside it.
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
  return bgm_causal_hmc_obs_named(h->hmc_partial, std::string(what) + " with a trajectory length per chain");
}

}  // namespace

int bgm_causal_hmc_traj_launch(bgm_handle *h, const CausalHmcLaunch &l) {
  const CausalHmcTrajArgs &tj = l.st->traj;
  return bgm_causal_hmc_launch_pair(
      h, l, named(h, "HMC kernel"), [](auto s, auto obs) { return causal_hmc_traj_kernel<decltype(s)::KT1, MH_WAVES, decltype(obs)::value>; },
      [](auto s, auto obs) { return causal_hmc_traj_mass_kernel<decltype(s)::KT1, MH_WAVES, decltype(obs)::value>; }, tj);
}

namespace {

template <int EFFECT, bool OBS>
int launch_fx(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx) {
  const CausalHmcTrajArgs &tj = l.st->traj;
  return bgm_causal_hmc_launch_pair(
      h, l, named(h, "HMC kernel with fused effects"),
      [](auto s) { using S = decltype(s); return causal_hmc_traj_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT, OBS>; },
      [](auto s) { using S = decltype(s); return causal_hmc_traj_mass_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT, OBS>; }, fx, tj);
}

}  // namespace

// (the panel's dose-response with the observation pattern was refused by the entry point: it has no OBS kernel at all)
int bgm_causal_hmc_traj_fx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, bool binary) {
  if (!binary) return launch_fx<1, false>(h, l, fx);
  return bgm_causal_hmc_with_pattern(h, [&](auto obs) { return launch_fx<2, decltype(obs)::value>(h, l, fx); });
}

int bgm_causal_hmc_traj_rowfx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, const CausalHmcRowFxArgs &rf) {
  const CausalHmcTrajArgs &tj = l.st->traj;
  return bgm_causal_hmc_launch_pair(
      h, l, named(h, "HMC kernel with per-row effects"),
      [](auto s, auto obs) { using S = decltype(s); return causal_hmc_traj_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES, decltype(obs)::value>; },
      [](auto s, auto obs) { using S = decltype(s); return causal_hmc_traj_mass_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES, decltype(obs)::value>; },
      fx, rf, tj);
}
