// causal_hmc_rowfx_kernels.h -- the HMC transitions of causal_hmc_fx_kernels.h with the dose-response of every ROW kept, instead of
// the panel's average (gfx950): per-row curves and their posterior spread without stored draws.
//
// replaces: nothing in causalbgm/base.py; infer_from_latent_posterior (:671-763) reduces y_i(x_k) over the rows of the panel
//   (its .mean()), for a continuous treatment the reference has no per-row quantity at all.
//
// causal_hmc_rowfx_kernel / causal_hmc_mass_rowfx_kernel are causal_hmc_fx_kernel / causal_hmc_mass_fx_kernel with EFFECT == 1 --
// one body, chmc_run: same registers, same LDS blob with f's pieces of the sampling blob behind it, same RNG streams, accept rule,
// step table, metric and launch cuts -- and ONE difference, inside causal_effects (causal_kernels.h, ROWS): at the end of a pass
// lane (j, g) holds y of (row j of the tile, dose k of lane group g).  Where the fused-ADRF kernels reduce it over j and add the
// sum into the wave slot's partial with an atomic, these kernels leave it with the row:
//   moments [3][n_doses][n] float32 (always): plane 0 = ref, the value at retained draw 0 (written when it == burn_in, together
//     with zeros in the other two), plane 1 = s1 += y - ref, plane 2 = s2 += (y - ref)^2 -- the shifted sums of the metric's window
//     moments (ma.ref / s1 / s2).  The 16 lanes of a lane group touch 16 consecutive floats of a plane; every (row, dose) has one
//     owner lane, so plain loads and stores, no atomics.
//   draws [n][n_doses][n_keep] float32 (only when given): draws[(row * n_doses + k) * n_keep + d] = y, the layout
//     bgm_row_mean_quantiles reads and the access pattern of ite[row * n_keep + d].
// Rows beyond n of a ragged tile and doses k >= n_doses of a padded pass write nothing.  The sums live in global memory and are
// carried by nothing else: a run cut at any iteration is the same run bit for bit, and a row's result depends on (seed, global
// row, the row's data) alone -- not on n, the grid, the tile walk or the rank count.
#pragma once
#include "causal_hmc_fx_kernels.h"

struct CausalHmcRowFxArgs {
  float *moments;                     // [3][n_doses][n]: ref, s1, s2
  float *draws;                       // [n][n_doses][n_keep] or NULL
};

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_rowfx_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcRowFxArgs rf) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, false, true>(lds, a, CausalHmcMassArgs{}, fx, rf.moments, rf.draws);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_rowfx_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                           CausalHmcRowFxArgs rf) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, true, true>(lds, a, ma, fx, rf.moments, rf.draws);
}
