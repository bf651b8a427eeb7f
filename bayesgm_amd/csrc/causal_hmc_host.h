// causal_hmc_host.h -- host state of the CausalBGM HMC latent sampler, shared by every causal_hmc_*_api.hip: the handle's HmcState, the
// call and launch records of a segment, and the launch of a kernel with its metric twin by shape, metric and observation pattern
// (bgm_causal_hmc_launch_pair).  Host only.
#pragma once
#include "causal_launch.h"
#include "causal_hmc_fx_kernels.h"

// bgm_handle::hmc_state
struct HmcState {
  float *blob_dev = nullptr;       // the dual-access copy of the Gram blob
  size_t blob_cap = 0;
  CausalHmcMeta m{};
  CausalHmcMassArgs mass{};        // bgm_causal_hmc_set_mass; scale = NULL: identity mass
  CausalHmcTrajArgs traj{};        // bgm_causal_hmc_set_trajectory; (0, 0, NULL): the kernels without TRAJ
  bool traj_set() const { return traj.max_traj > 0.0f || traj.jitter != 0 || traj.n_steps != nullptr; }
};

static inline HmcState *bgm_causal_hmc_state(bgm_handle *h) {
  if (!h->hmc_state) h->hmc_state = new HmcState();
  return static_cast<HmcState *>(h->hmc_state);
}

// the trajectory options of the handle while any is set (bgm_causal_hmc_set_trajectory), else NULL
static inline const CausalHmcTrajArgs *bgm_causal_hmc_traj(const bgm_handle *h) {
  const HmcState *st = static_cast<const HmcState *>(h->hmc_state);
  return st && st->traj_set() ? &st->traj : nullptr;
}
// BGM_E_UNSUPPORTED, naming the option, for an entry point whose kernels have no TRAJ twin; the handle stays usable
int bgm_causal_hmc_traj_refuse(const bgm_handle *h, const char *who, const char *kernels);                   // causal_hmc_traj_api.hip
// the launches of the TRAJ kernels (causal_hmc_traj_kernels.h), all of which live in causal_hmc_traj_api.hip: what the entry points
// call while a trajectory option is set, after their own checks and with the kernel arguments they built as always.  The metric and
// the observation pattern (bgm_causal_hmc_set_partial) are read from the handle.
struct CausalHmcLaunch;
struct CausalHmcRowFxArgs;
int bgm_causal_hmc_traj_launch(bgm_handle *h, const CausalHmcLaunch &l);                                      // bgm_causal_hmc_run
int bgm_causal_hmc_traj_fx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, bool binary);      // bgm_causal_hmc_run_effects
int bgm_causal_hmc_traj_rowfx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx,
                                     const CausalHmcRowFxArgs &rf);                                           // bgm_causal_hmc_run_row_effects

// floats of the dual-access blob (causal_hmc_api.hip, hmc_prepare): known from the shape alone, before anything is packed or launched
static inline int bgm_causal_hmc_blob_floats(int KT1, int n_gh) {
  return 3 * (4 * 16 * KT1 * 17 + 64) + n_gh * (CHMC_W64 + 64) + CHMC_W64 + 132 + 2 * (2 * 64 * 17 + 32 + 32 * 17 + 16 + 16 * 17 + 16);
}

// BGM_E_STATE for an unconfigured handle, BGM_E_UNSUPPORTED (naming the path) where the gradient / HMC kernels do not exist
int bgm_causal_hmc_check(bgm_handle *h, const char *who);                                                     // causal_hmc_api.hip
// The arguments every HMC segment takes (bgm_causal_hmc_run and the three entry points with an effect pass; include/bgm_hip.h says
// what each means), in the order of the C ABI.  An entry point fills one from its parameters and passes it on by reference.
struct CausalHmcCall {
  const float *x, *y, *v;
  int64_t n, row_base;
  float *state, *logp, *grad, *step;
  const float *up, *dn;
  int32_t n_table;
  float s_min, s_max;
  int32_t init, it_begin, n_iters, burn_in, n_leapfrog;
  uint64_t seed;
  uint32_t *acc_count;
  float *draws;
  int32_t n_keep;
  hipStream_t stream;
};
// The call record of an extern "C" entry point, from its parameters under the names every bgm_causal_hmc_run* definition gives them
// (those of include/bgm_hip.h without the _dev suffix, and stream_): the parameter lists are the ABI and stay spelled out, the
// bodies name the 24 once, here.
#define BGM_CAUSAL_HMC_CALL                                                                                                              \
  CausalHmcCall {                                                                                                                        \
    x, y, v, n, row_base, state, logp, grad, step, up, dn, n_table, s_min, s_max, init, it_begin, n_iters, burn_in, n_leapfrog, seed,     \
        acc_count, draws, n_keep, (hipStream_t)stream_                                                                                    \
  }

// What preparation makes of a call: the kernel arguments of one launch, the handle's HMC state (blob, meta, metric), the grid and
// the dynamic LDS bytes (the HMC blob; with f's part of the sampling blob behind it after bgm_causal_hmc_fx_prepare)
struct CausalHmcLaunch {
  CausalHmcKArgs ka;
  HmcState *st;
  int grid;
  int lds;
  hipStream_t stream;
};

// the argument checks of bgm_causal_hmc_run (`who` names the entry point), the panel's Gram pre-pass and the dual-access blob, the
// metric's buffers (st->mass, once for every entry point), then the launch record
int bgm_causal_hmc_args(bgm_handle *h, const char *who, const CausalHmcCall &call, CausalHmcLaunch &launch);      // causal_hmc_api.hip
int bgm_causal_hmc_mass_launch(bgm_handle *h, const CausalHmcLaunch &launch);                                     // causal_hmc_mass_api.hip

// bgm_causal_dispatch for a kernel that has a twin with the metric: f(S{}, std::true_type) while a metric is set
// (bgm_causal_hmc_set_mass; it launches the twin with st->mass), f(S{}, std::false_type) otherwise.  `what` names the kernel.
template <class F>
static int bgm_causal_hmc_dispatch(const bgm_handle *h, const HmcState *st, const std::string &what, F &&f) {
  if (st->mass.scale) return bgm_causal_dispatch(h, (what + ", with a diagonal metric").c_str(), [&](auto s) { return f(s, std::true_type{}); });
  return bgm_causal_dispatch(h, what.c_str(), [&](auto s) { return f(s, std::false_type{}); });
}

// f(std::bool_constant<OBS>) by the handle's observation pattern (bgm_causal_hmc_set_partial): the one place that turns
// bgm_handle::hmc_partial into the kernels' OBS template argument, with the words a kernel's name gets for it in an error
template <class F>
static int bgm_causal_hmc_with_pattern(const bgm_handle *h, F &&f) {
  return h->hmc_partial ? f(std::true_type{}) : f(std::false_type{});
}
static inline std::string bgm_causal_hmc_obs_named(bool obs, const std::string &what) {
  return obs ? what + " for partially observed rows" : what;
}

// launch(kernel) for the kernel that `pick` names for the shape tag S: pick(S{}), or pick(S{}, obs) by the handle's observation
// pattern where the lambda takes the tag (a family whose OBS twins live in the same unit).  A pick that returns an int instead of
// a kernel has refused that combination at its site (error set, code returned as it is): nothing is launched and no kernel is
// instantiated for it.
template <class Pick, class S, class L>
static int bgm_causal_hmc_picked(const bgm_handle *h, Pick &pick, S s, L &&launch) {
  auto go = [&](auto kernel) {
    if constexpr (std::is_same_v<decltype(kernel), int>) return kernel;
    else return launch(kernel);
  };
  if constexpr (std::is_invocable_v<Pick &, S>) return go(pick(s));
  else return bgm_causal_hmc_with_pattern(h, [&](auto obs) { return go(pick(s, obs)); });
}

// The launch of a kernel and its twin with the metric, at every site that has both in one translation unit: plain and mass name
// the two instantiations (generic lambdas, bgm_causal_hmc_picked; the unit that writes them is the unit that instantiates them),
// `extra` are the kernel arguments behind l.ka, and the twin takes l.st->mass between the two.  `what` names the kernel in errors.
template <class Plain, class Mass, class... A>
static int bgm_causal_hmc_launch_pair(const bgm_handle *h, const CausalHmcLaunch &l, const std::string &what, Plain plain, Mass mass,
                                      const A &...extra) {
  return bgm_causal_hmc_dispatch(h, l.st, what, [&](auto s, auto metric) {
    if constexpr (decltype(metric)::value)
      return bgm_causal_hmc_picked(h, mass, s, [&](auto k) { return bgm_launch(k, l.grid, MH_WAVES, l.lds, l.stream, l.ka, l.st->mass, extra...); });
    else
      return bgm_causal_hmc_picked(h, plain, s, [&](auto k) { return bgm_launch(k, l.grid, MH_WAVES, l.lds, l.stream, l.ka, extra...); });
  });
}
