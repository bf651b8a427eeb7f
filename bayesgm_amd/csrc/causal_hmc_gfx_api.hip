// causal_hmc_gfx_api.hip -- bgm_causal_hmc_run_group_effects and bgm_ite_group_sums (include/bgm_hip.h): the CausalBGM HMC latent
// sampler with the individual treatment effect summed by row label inside the retained iterations, and the same sums from a stored
// ITE matrix (causal_hmc_gfx_kernels.h: the EFFECT 4 instantiations of chmc_run), in a translation unit of its own, compiled beside
// those of the other HMC entry points.
// replaces: nothing in causalbgm/base.py; infer_from_latent_posterior (:671-763) returns the ITE of every row and draw.
#include <string>

#include "causal_launch.h"
#include "causal_hmc_fx_host.h"
#include "causal_hmc_gfx_kernels.h"

namespace {
const char *WHO = "bgm_causal_hmc_run_group_effects";
const int MAX_LABELS = 64;
}  // namespace

extern "C" int bgm_causal_hmc_run_group_effects(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base,
                                                float *state, float *logp, float *grad, float *step, const float *up, const float *dn,
                                                int32_t n_table, float s_min, float s_max, int32_t init, int32_t it_begin, int32_t n_iters,
                                                int32_t burn_in, int32_t n_leapfrog, uint64_t seed, uint32_t *acc_count, float *draws,
                                                int32_t n_keep, int32_t sample_y, const int32_t *labels, int32_t n_labels,
                                                float *group_partial, void *stream_) {
  if (int rc = bgm_causal_hmc_check(h, WHO)) return rc;
  if (n <= 0 || n_iters <= 0) return BGM_OK;
  if (int rc = bgm_causal_hmc_traj_refuse(h, WHO, "the label-sum kernels")) return rc;
  const std::string who(WHO);
  if (h->hmc_partial) {
    bgm_set_error(who + ": the label sums have no kernel for partially observed rows (bgm_causal_hmc_set_partial); the treatment "
                        "effect of every row has: bgm_causal_hmc_run_effects (BGM_EFFECT_ITE)");
    return BGM_E_UNSUPPORTED;
  }
  if (h->cfg.binary_treatment == 0) {
    bgm_set_error(who + ": the label sums are those of the individual treatment effect of a binary treatment; a continuous treatment "
                        "has its dose-response: bgm_causal_hmc_run_effects (BGM_EFFECT_ADRF)");
    return BGM_E_INVALID;
  }
  if (n_labels < 1 || n_labels > MAX_LABELS) {
    bgm_set_error(who + ": n_labels must be in [1, " + std::to_string(MAX_LABELS) + "]; got " + std::to_string(n_labels));
    return BGM_E_INVALID;
  }
  if (!labels || !group_partial) { bgm_set_error(who + ": labels / group_partial required"); return BGM_E_INVALID; }
  const CausalHmcCall call{x, y, v, n, row_base, state, logp, grad, step, up, dn, n_table, s_min, s_max, init, it_begin, n_iters, burn_in,
                           n_leapfrog, seed, acc_count, draws, n_keep, (hipStream_t)stream_};
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, call, l, fx)) return rc;
  fx.sample_y = sample_y; fx.n_doses = n_labels;      // (the slot's stride: [n_keep][n_labels])
  fx.adrf_partial = group_partial;
  fx.ite = reinterpret_cast<float *>(const_cast<int32_t *>(labels));      // (read only, as int: chmc_run, EFFECT 4)
  return bgm_causal_hmc_dispatch(h, l.st, "HMC kernel with label sums of the treatment effect", [&](auto s, auto metric) {
    using S = decltype(s);
    if constexpr (decltype(metric)::value)
      return bgm_launch(causal_hmc_mass_gfx_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, l.st->mass, fx);
    else
      return bgm_launch(causal_hmc_gfx_kernel<S::KT1, S::KSL1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, fx);
  });
}

extern "C" int bgm_ite_group_sums(bgm_handle *h, const float *ite, const int32_t *labels, int64_t n, int32_t n_keep, int32_t n_labels,
                                  double *out, void *stream_) {
  const std::string who("bgm_ite_group_sums");
  if (!h || !ite || !labels || !out || n <= 0 || n_keep <= 0) { bgm_set_error(who + ": bad argument"); return BGM_E_INVALID; }
  if (n_labels < 1 || n_labels > MAX_LABELS) {
    bgm_set_error(who + ": n_labels must be in [1, " + std::to_string(MAX_LABELS) + "]; got " + std::to_string(n_labels));
    return BGM_E_INVALID;
  }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  const unsigned blocks = (unsigned)(((long long)n_keep + ITE_GROUP_THREADS - 1) / ITE_GROUP_THREADS);
  const size_t lds = (size_t)n_labels * ITE_GROUP_THREADS * sizeof(double);      // <= 32 KiB
  hipLaunchKernelGGL(ite_group_sums_kernel, dim3(blocks), dim3(ITE_GROUP_THREADS), lds, (hipStream_t)stream_, ite, labels, (long long)n,
                     (int)n_keep, (int)n_labels, out);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
