// causal_hmc_tails_kernels.h -- the per-row dose-response kernels of causal_hmc_rowfx_kernels.h / causal_hmc_obs_kernels.h with the
// two TAILS of every (row, dose) series kept beside its moments (gfx950): exact quantile bounds per row without stored draws.
//
// replaces: nothing in causalbgm/base.py; the reference's intervals are np.quantile pairs over stored draws (:640-642, :664-666), and a
//   linearly interpolated quantile at level alpha / 2 reads only the K smallest of the m draws, the one at 1 - alpha / 2 only the K
//   largest (K = causal_hmc.tail_size(alpha, m), about alpha / 2 * m + 2).
//
// The four kernels are their twins with TAILS: one body, chmc_run -- same registers, LDS blob, RNG streams, accept rule, step table,
// metric, observation pattern, launch cuts, moments and optional draws -- and ONE difference, inside causal_effects (causal_kernels.h,
// ROWS): lane (j, g), which holds y of (row j of the tile, dose k of lane group g), also pushes it into the series' two buffers of
//   tails [2][k_tail][n_doses][n] float32: tail 0 the k_tail smallest values, tail 1 the k_tail largest, slot-major -- for every slot
//     the 16 lanes of a lane group touch 16 consecutive floats, like the moment planes.  Each tail is a binary heap with its threshold
//     at slot 0 (row_tail_push): a draw that enters neither tail costs one load per tail.
// The buffers live in global memory and are carried by nothing else: draw 0 initialises a series (the buffer need not be zeroed), a
// run cut at any iteration is the same run bit for bit, and a series' buffers depend on its draw sequence alone.  The order inside a
// buffer is the kernel's business; bgm_row_tail_quantiles reads the order statistics it needs.
#pragma once
#include "causal_hmc_obs_kernels.h"

struct CausalHmcTailsArgs {
  float *moments;                     // [3][n_doses][n]: ref, s1, s2
  float *draws;                       // [n][n_doses][n_keep] or NULL
  float *tails;                       // [2][k_tail][n_doses][n]
  int k_tail;                         // 1 <= k_tail <= n_keep
};

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_tails_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcTailsArgs rt) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, false, true, false, true>(lds, a, CausalHmcMassArgs{}, fx, rt.moments, rt.draws, rt.tails, rt.k_tail);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_tails_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                           CausalHmcTailsArgs rt) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, true, true, false, true>(lds, a, ma, fx, rt.moments, rt.draws, rt.tails, rt.k_tail);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_tails_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx, CausalHmcTailsArgs rt) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, false, true, true, true>(lds, a, CausalHmcMassArgs{}, fx, rt.moments, rt.draws, rt.tails, rt.k_tail);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_obs_mass_tails_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx,
                                                                               CausalHmcTailsArgs rt) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 1, true, true, true, true>(lds, a, ma, fx, rt.moments, rt.draws, rt.tails, rt.k_tail);
}
