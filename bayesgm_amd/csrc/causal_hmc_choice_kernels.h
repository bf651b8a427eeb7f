// causal_hmc_choice_kernels.h -- the per-row dose-response kernels of causal_hmc_rowfx_kernels.h / causal_hmc_obs_kernels.h with the
// CHOICE among the doses kept beside the curve (gfx950): at every retained draw, which dose gives row i its best outcome, what that
// outcome is, and which doses exceed a threshold -- the joint over the doses, without stored draws.
//
// replaces: nothing in causalbgm/base.py; for a continuous treatment the reference has the panel's ADRF only
//   (infer_from_latent_posterior :671-763), no per-row quantity and no comparison between doses.
//
// Moments, tails and contrasts against one baseline describe every dose alone or one pair.  The best dose changes from draw to draw,
// so the doses are compared per retained draw, inside the sampler, where one wave holds all doses of its rows pass by pass.
//
// The kernels are their twins with CHOICE: one body, chmc_run -- same registers, LDS blob, RNG streams, accept rule, step table,
// metric, observation pattern, launch cuts, curve planes and row draws (both record y) -- and ONE difference, inside causal_effects
// (causal_kernels.h, CHOICE).  Two registers, (best, best_k), live across the passes of a draw; everything else is recomputed.
//   moments    [3][n_doses][n] float32: the shifted sums of y, those of causal_hmc_rowfx_kernels.h;
//   draws      [n][n_doses][n_keep] float32 (only when given): y, as there;
//   best_count [n_doses][n] uint32: the retained draws at which dose k was the row's best (sign * y largest; the lowest index on
//     ties).  A column sums to the number of retained draws unless a draw's values were all NaN;
//   best_mom   [2][n] float32: plane 0 = the best y of retained draw 0, plane 1 = s1 += best - ref (the unsigned y, not sign * y);
//   above      [n_doses][n] uint32 (only when given): the retained draws with y > threshold.
// Every element of best_count / best_mom belongs to lane (j, 0) of its row for the whole run, every element of above to the owner
// lane of (row, k); the iteration it == burn_in writes them (zeros included), later ones load, add and store.  Nothing a draw
// contributes outlives the draw in a register, so a run cut at any iteration is the same run bit for bit.
// With sample_y every dose carries its own independent noise word (dose k: word k & 3 of Philox call k >> 2).
// Four kernels per shape: {identity, metric} x {fully observed, OBS}.  No twin with TRAJ, TAILS or CONTRAST.  The metric with OBS at
// KT1 = 2 is not instantiated: hipcc gives it 12 bytes of scratch at 256 VGPRs, and causal_hmc_choice_api.hip refuses the combination.
#pragma once
#include "causal_hmc_obs_kernels.h"

struct CausalHmcChoiceArgs {
  float *moments;                     // [3][n_doses][n]: ref, s1, s2 of y
  float *draws;                       // [n][n_doses][n_keep] of y, or NULL
  CausalChoiceArgs ch;                // best_count, best_mom, above, sign, threshold (causal_kernels.h)
};

template <int KT1, int KSL1, int WAVES, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_choice_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcChoiceArgs rc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, false, true, OBS, false, false, false, true>(lds, a, CausalHmcMassArgs{}, fx, rc.moments, rc.draws, nullptr, 0,
                                                                             CausalHmcTrajArgs{}, nullptr, rc.ch);
}

template <int KT1, int KSL1, int WAVES, bool OBS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_choice_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                            CausalHmcChoiceArgs rc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, true, true, OBS, false, false, false, true>(lds, a, ma, fx, rc.moments, rc.draws, nullptr, 0,
                                                                            CausalHmcTrajArgs{}, nullptr, rc.ch);
}
