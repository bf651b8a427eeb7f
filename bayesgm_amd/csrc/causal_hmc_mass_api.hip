// causal_hmc_mass_api.hip -- the CausalBGM HMC latent sampler with a diagonal metric per chain (bgm_causal_hmc_set_mass,
// bgm_causal_hmc_mass_update; include/bgm_hip.h): the MASS instantiations of the HMC transition without an effect pass
// (causal_hmc_fx_kernels.h, chmc_run) and the kernel that turns a window's moments into the next scales, in a translation unit of
// their own, compiled beside the others: bgm_causal_hmc_run (causal_hmc_api.hip) comes here only while a metric is set.
// replaces: nothing in causalbgm/base.py; the windowed estimate is the diagonal adaptation of Stan's warm-up, per chain (opt-in).
#include <string>

#include "causal_launch.h"
#include "causal_hmc_host.h"

// End of an estimation window of W draws, one thread per chain, float64 inside:
//   mean_i = S1_i / W,  var_i = max(S2_i / W - mean_i^2, 0),  vbar = mean_i(var_i),  var_r_i = (W var_i + 5e-3 vbar) / (W + 5)
//   s_i = clamp(sqrt(var_r_i) / geomean_j sqrt(var_r_j), 0.05, 20), rounded once to float32
// (Stan's shrinkage -- 5 draws' weight on a variance of 1e-3 -- with the chain's own mean variance as the unit, so it is scale-free.
// The whole of vbar as the target would overwrite what is being estimated: with sd spread over 0.01 .. 1 and W = 2000 it doubles
// the smallest sd.  The geometric mean is divided out, so s carries the shape only and the step keeps the scale.)  vbar zero or not finite -- the chain never moved -- keeps s.  Then ref = state and
// S1 = S2 = 0.  W = 0 only resets.
__global__ __launch_bounds__(256) void causal_hmc_mass_update_kernel(long long n, int q, int W, const float *state, float *scale, float *ref,
                                                                     float *s1, float *s2) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const long long o = row * (long long)q;
  if (W > 0) {
    const double w = (double)W;
    auto var = [&](int i) {
      const double mean = (double)s1[o + i] / w;
      return fmax((double)s2[o + i] / w - mean * mean, 0.0);
    };
    double vbar = 0.0;
    for (int i = 0; i < q; ++i) vbar += var(i);
    vbar /= (double)q;
    if (vbar > 0.0 && vbar < (double)INFINITY) {
      double lg = 0.0;
      for (int i = 0; i < q; ++i) lg += log((w * var(i) + 5e-3 * vbar) / (w + 5.0));
      const double gm = exp(0.5 * lg / (double)q);      // geometric mean of sqrt(var_r)
      for (int i = 0; i < q; ++i) scale[o + i] = (float)fmin(fmax(sqrt((w * var(i) + 5e-3 * vbar) / (w + 5.0)) / gm, 0.05), 20.0);
    }
  }
  for (int i = 0; i < q; ++i) {
    ref[o + i] = state[o + i];
    s1[o + i] = 0.0f;
    s2[o + i] = 0.0f;
  }
}

extern "C" int bgm_causal_hmc_set_mass(bgm_handle *h, const float *scale_dev, const float *ref_dev, float *s1_dev, float *s2_dev,
                                       int32_t accumulate) {
  if (!h) { bgm_set_error("bgm_causal_hmc_set_mass: NULL handle"); return BGM_E_INVALID; }
  if (!scale_dev) {
    if (h->hmc_state) static_cast<HmcState *>(h->hmc_state)->mass = CausalHmcMassArgs{};
    return BGM_OK;
  }
  if (int rc = bgm_causal_hmc_check(h, "bgm_causal_hmc_set_mass")) return rc;
  if (accumulate && (!ref_dev || !s1_dev || !s2_dev)) { bgm_set_error("bgm_causal_hmc_set_mass: accumulate needs ref_dev, s1_dev and s2_dev"); return BGM_E_INVALID; }
  CausalHmcMassArgs &ma = bgm_causal_hmc_state(h)->mass;
  ma.scale = scale_dev; ma.ref = ref_dev; ma.s1 = s1_dev; ma.s2 = s2_dev; ma.accumulate = accumulate ? 1 : 0;
  return BGM_OK;
}

extern "C" int bgm_causal_hmc_mass_update(bgm_handle *h, int64_t n, int32_t n_draws, const float *state_dev, float *scale_dev, float *ref_dev,
                                          float *s1_dev, float *s2_dev, void *stream_) {
  if (int rc = bgm_causal_hmc_check(h, "bgm_causal_hmc_mass_update")) return rc;
  if (n <= 0) return BGM_OK;
  if (!state_dev || !scale_dev || !ref_dev || !s1_dev || !s2_dev) { bgm_set_error("bgm_causal_hmc_mass_update: NULL pointer"); return BGM_E_INVALID; }
  if (n_draws < 0) { bgm_set_error("bgm_causal_hmc_mass_update: n_draws must be >= 0"); return BGM_E_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  hipLaunchKernelGGL(causal_hmc_mass_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (long long)n, h->q, (int)n_draws,
                     state_dev, scale_dev, ref_dev, s1_dev, s2_dev);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

int bgm_causal_hmc_mass_launch(bgm_handle *h, const CausalHmcLaunch &l) {
  return bgm_causal_dispatch(h, "HMC kernel with a diagonal metric", [&](auto s) {
    using S = decltype(s);
    return bgm_launch(causal_hmc_mass_kernel<S::KT1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka, l.st->mass);
  });
}
