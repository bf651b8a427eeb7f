// causal_hmc_gfx_api.hip -- bgm_causal_hmc_run_group_effects and bgm_ite_group_sums (include/bgm_hip.h): the CausalBGM HMC latent
// sampler with the individual treatment effect summed by row label inside the retained iterations, and the same sums from a stored
// ITE matrix (causal_hmc_gfx_kernels.h: the EFFECT 4 instantiations of chmc_run), in a translation unit of its own, compiled beside
// those of the other HMC entry points.
// Prologue, preparation and the launch of a kernel with its metric twin are those of every entry point with an effect pass
// (causal_hmc_fx_host.h, causal_hmc_host.h); what is this unit's own is its argument checks and the kernels it names.
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
  bool go;
  if (int rc = bgm_causal_hmc_begin(h, WHO, n, n_iters, "the label-sum kernels", go); rc || !go) return rc;
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
  CausalHmcLaunch l{};
  CausalHmcFxArgs fx{};
  if (int rc = bgm_causal_hmc_fx_prepare(h, WHO, BGM_CAUSAL_HMC_CALL, sample_y, n_labels /* the slot's stride: [n_keep][n_labels] */, nullptr, l, fx))
    return rc;
  fx.adrf_partial = group_partial;
  fx.ite = reinterpret_cast<float *>(const_cast<int32_t *>(labels));      // (read only, as int: chmc_run, EFFECT 4)
  return bgm_causal_hmc_launch_pair(
      h, l, "HMC kernel with label sums of the treatment effect", [](auto s) { using S = decltype(s); return causal_hmc_gfx_kernel<S::KT1, S::KSL1, MH_WAVES>; },
      [](auto s) { using S = decltype(s); return causal_hmc_mass_gfx_kernel<S::KT1, S::KSL1, MH_WAVES>; }, fx);
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
