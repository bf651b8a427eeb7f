// causal_hmc_traj_kernels.h -- the HMC transitions of the CausalBGM latent sampler with a number of leapfrog steps per chain and
// iteration (gfx950): the TRAJ instantiations of chmc_run (causal_hmc_fx_kernels.h, where the rule is stated).
//
// replaces: nothing in causalbgm/base.py (the reference samples CausalBGM's latents by random-walk MH only); the options are those of
//   the BGM imputation sampler here (bgm_rowstep_kernels.h, STEP 2), whose kernels must run every wave of a workgroup to the launch's
//   step count.  These kernels need not: a wave's leapfrog loop ends at the largest L_i of its own 16 rows.
//
// Every kernel is its twin without TRAJ -- same argument structs, LDS blob, registers' layout, RNG streams (the jitter uniform is call
// 1 of TAG_HACC, which no other CausalBGM kernel draws), accept rule, step table, metric, observation pattern and effect pass -- with
// CausalHmcTrajArgs as one more kernel argument.  Twins: the plain transition, the fused ADRF (EFFECT 1) and ITE (EFFECT 2) and the
// per-row dose-response (ROWS), each with and without the metric, and with the observation pattern (OBS) wherever an OBS twin
// exists (every one but the panel ADRF).  The tail-buffer kernels (TAILS) and the label sums (EFFECT 4) have no TRAJ twin.
#pragma once
#include "causal_hmc_rowfx_kernels.h"

template <int KT1, int WAVES, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_traj_kernel(CausalHmcKArgs a, CausalHmcTrajArgs tj) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, 1, WAVES, 0, false, false, OBS, false, true>(lds, a, CausalHmcMassArgs{}, CausalHmcFxArgs{}, nullptr, nullptr, nullptr, 0, tj);
}

template <int KT1, int WAVES, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_traj_mass_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcTrajArgs tj) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, 1, WAVES, 0, true, false, OBS, false, true>(lds, a, ma, CausalHmcFxArgs{}, nullptr, nullptr, nullptr, 0, tj);
}

template <int KT1, int KSL1, int WAVES, int EFFECT, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_traj_fx_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcTrajArgs tj) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, EFFECT, false, false, OBS, false, true>(lds, a, CausalHmcMassArgs{}, fx, nullptr, nullptr, nullptr, 0, tj);
}

template <int KT1, int KSL1, int WAVES, int EFFECT, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_traj_mass_fx_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                             CausalHmcTrajArgs tj) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, EFFECT, true, false, OBS, false, true>(lds, a, ma, fx, nullptr, nullptr, nullptr, 0, tj);
}

template <int KT1, int KSL1, int WAVES, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_traj_rowfx_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcRowFxArgs rf,
                                                                           CausalHmcTrajArgs tj) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, false, true, OBS, false, true>(lds, a, CausalHmcMassArgs{}, fx, rf.moments, rf.draws, nullptr, 0, tj);
}

template <int KT1, int KSL1, int WAVES, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_traj_mass_rowfx_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                                CausalHmcRowFxArgs rf, CausalHmcTrajArgs tj) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, true, true, OBS, false, true>(lds, a, ma, fx, rf.moments, rf.draws, nullptr, 0, tj);
}
