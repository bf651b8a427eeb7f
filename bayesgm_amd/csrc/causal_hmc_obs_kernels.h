// causal_hmc_obs_kernels.h -- the CausalBGM log posterior with its gradient and the HMC transitions for rows whose outcome, or outcome
// and treatment, are NOT OBSERVED (gfx950): the OBS instantiations of chmc_logpost_run (causal_hmc_kernels.h) and chmc_run
// (causal_hmc_fx_kernels.h).
//
// replaces: nothing in causalbgm/base.py; the reference's predict takes the training triplet (x, y, v) and has no answer for a new
//   unit.  The target is get_log_posterior :765-817 with the terms of the unobserved variables left out: p(z | x, v) for a row
//   without its outcome, p(z | v) for a row without outcome and treatment.
//
// The observation pattern travels in the data: x[row] / y[row] is NaN where it is not observed (chmc_observed).  There is no further
// kernel argument, struct field or buffer, so the argument structs, the LDS blob, the registers' layout, the RNG streams, the accept
// rule, the step table, the metric and the effect pass are those of the twin kernels without OBS.  The effect pass evaluates f at the
// doses (or at 0 / 1) and never at the row's own x, so it needs nothing of the pattern.
// Instantiated: the log posterior, the plain transition, the fused ITE (EFFECT 2) and the per-row dose-response (ROWS), each with
// and without the metric.  The panel ADRF (EFFECT 1 without ROWS) and the label sums (EFFECT 4) have no OBS twin.
#pragma once
#include "causal_hmc_rowfx_kernels.h"

template <int KT1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_logpost_kernel(const float *blob, CausalHmcMeta m, const float *x, const float *y,
                                                                            const float *uc, const float *z, long long n, float *out_logp,
                                                                            float *out_grad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_logpost_run<KT1, WAVES, true>(lds, blob, m, x, y, uc, z, n, out_logp, out_grad);
}

template <int KT1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_kernel(CausalHmcKArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, 1, WAVES, 0, false, false, true>(lds, a, CausalHmcMassArgs{}, CausalHmcFxArgs{});
}

template <int KT1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_mass_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, 1, WAVES, 0, true, false, true>(lds, a, ma, CausalHmcFxArgs{});
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_ite_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 2, false, false, true>(lds, a, CausalHmcMassArgs{}, fx);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_mass_ite_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 2, true, false, true>(lds, a, ma, fx);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_rowfx_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcRowFxArgs rf) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, false, true, true>(lds, a, CausalHmcMassArgs{}, fx, rf.moments, rf.draws);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_mass_rowfx_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                               CausalHmcRowFxArgs rf) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, true, true, true>(lds, a, ma, fx, rf.moments, rf.draws);
}
