// causal_hmc_contrast_kernels.h -- the per-row dose-response kernels of causal_hmc_rowfx_kernels.h / causal_hmc_obs_kernels.h /
// causal_hmc_tails_kernels.h with the CONTRAST of every dose against a baseline dose kept beside the curve (gfx950): what row i gains
// at dose x_k over dose x_0, c_i(k) = y_i(x_k) - y_i(x_0), with its posterior spread and quantiles, without stored draws.
//
// replaces: nothing in causalbgm/base.py; for a continuous treatment the reference has the panel's ADRF only
//   (infer_from_latent_posterior :671-763), no per-row quantity and no difference between doses.
//
// The marginal moments and tails of causal_hmc_rowfx / causal_hmc_tails describe every dose alone.  The spread of a difference needs
// the joint: both doses are evaluated on the same latent draw and are strongly correlated, so the difference is formed per draw,
// inside the sampler, and summarised like the values themselves.
//
// The kernels are their twins with CONTRAST: one body, chmc_run -- same registers, LDS blob, RNG streams, accept rule, step table,
// metric, observation pattern, launch cuts and curve planes -- and ONE difference, inside causal_effects (causal_kernels.h, CONTRAST).
// Dose 0 of x_values is the baseline.  Lane (j, g) owns (row j of the tile, dose k of the pass); dose 0 is finished in pass 0 by lane
// group 0, so after pass 0 every lane of the wave reads y0 from lane j (one cross-lane read by all 64 lanes, outside the branch on
// valid rows and doses) and keeps it in a register over the remaining passes of the draw.  c = y - y0 is one float32 subtraction of
// the two rounded values; y itself reaches the curve planes as in the twins, bit for bit.
//   moments  [3][n_doses][n] float32: the shifted sums of y, those of causal_hmc_rowfx_kernels.h;
//   cmoments [3][n_doses][n] float32: the same rule on c -- plane 0 = c of retained draw 0 (written when it == burn_in, with zeros in
//     the other two), plane 1 = s1 += c - ref, plane 2 = s2 += (c - ref)^2.  At dose 0 c is exactly 0 on every draw;
//   draws [n][n_doses][n_keep] float32 (only when given) and tails [2][k_tail][n_doses][n] float32 (the TAILS kernels) record c, NOT y:
//     layout, owner lanes and row_tail_push are those of the twins.
// With sample_y the two doses of a contrast carry their own independent noise words (dose k: word k & 3 of Philox call k >> 2), as
// the two arms of the binary ITE do: c is then the difference of two independent predictive draws on one latent draw.
// Eight kernels per shape: {identity, metric} x {fully observed, OBS} x {no tails, TAILS}.  No twin with TRAJ.
#pragma once
#include "causal_hmc_tails_kernels.h"

struct CausalHmcContrastArgs {
  float *moments;                     // [3][n_doses][n]: ref, s1, s2 of y
  float *cmoments;                    // [3][n_doses][n]: ref, s1, s2 of c = y - y(dose 0)
  float *draws;                       // [n][n_doses][n_keep] of c, or NULL
  float *tails;                       // [2][k_tail][n_doses][n] of c (TAILS), else unused
  int k_tail;                         // 1 <= k_tail <= n_keep (TAILS)
};

template <int KT1, int KSL1, int WAVES, bool OBS, bool TAILS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_contrast_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcContrastArgs rc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, false, true, OBS, TAILS, false, true>(lds, a, CausalHmcMassArgs{}, fx, rc.moments, rc.draws, rc.tails, rc.k_tail,
                                                                      CausalHmcTrajArgs{}, rc.cmoments);
}

template <int KT1, int KSL1, int WAVES, bool OBS, bool TAILS>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_contrast_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                              CausalHmcContrastArgs rc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, true, true, OBS, TAILS, false, true>(lds, a, ma, fx, rc.moments, rc.draws, rc.tails, rc.k_tail,
                                                                     CausalHmcTrajArgs{}, rc.cmoments);
}
