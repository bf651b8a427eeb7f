// causal_hmc_gfx_kernels.h -- the HMC transitions of causal_hmc_fx_kernels.h with the individual treatment effect of a binary
// treatment summed by ROW LABEL inside the sampler (gfx950): ATE / ATT / ATC and subgroup effects per retained draw without an
// [n x n_keep] matrix.
//
// replaces: nothing in causalbgm/base.py; infer_from_latent_posterior (:671-763) returns the ITE of every row and draw, and the
//   reference's tutorial averages its posterior mean over the rows on the host (a point estimate without an interval).
//
// causal_hmc_gfx_kernel / causal_hmc_mass_gfx_kernel are causal_hmc_fx_kernel / causal_hmc_mass_fx_kernel with EFFECT == 4 -- one
// body, chmc_run: same registers, same LDS blob with f's pieces of the sampling blob behind it, same RNG streams, accept rule,
// step table, metric and launch cuts -- and ONE difference, at the end of causal_effects (causal_kernels.h, EFFECT 4): where the
// ITE kernels store y(1) - y(0) of (row, draw d) into ite[row * n_keep + d], these kernels add it into
//   group_partial [n_slots][n_keep][n_labels] float32 (+=): element (slot, d, c) = sum of the values of the rows with label c over
//     the tiles the wave slot walks -- the layout of adrf_partial with n_labels in place of n_doses, finished by bgm_adrf_reduce.
// A row's label (labels [n] int32, 0 <= c < n_labels; the pointer travels in fx.ite) is read into one register of the row's lanes at
// the effect call.
// Order of the additions (fixed, no two lanes ever add onto one address): the labels present among the valid rows of a tile are
// taken in the order of their lowest row; for each, the values of its rows are reduced over the 16 lanes of lane group 0 by the DPP
// tree of sum_over_j_to_lane15 (the other rows contribute +0.0f) and lane 15 adds the total into the slot; the tiles of a slot
// follow each other in the tile walk, the draws in the iteration loop.  One label in a tile: one reduction; 16 labels: 16.
// Padding lanes of a ragged tile carry the clamped row's label, are not in the ballot and contribute zero; a label outside
// [0, n_labels) is added nowhere.  The partials live in global memory: a run cut at any iteration is the same run bit for bit.  They
// depend on the grid (which tiles share a slot), not on the cuts.
#pragma once
#include "causal_hmc_fx_kernels.h"

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_gfx_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 4, false>(lds, a, CausalHmcMassArgs{}, fx);
}

template <int KT1, int KSL1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_gfx_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, 4, true>(lds, a, ma, fx);
}

// ---------------------------------------------------------------------------
// The same sums from a stored ITE matrix (the MH sampler's fused kernel writes one; an independent check of the kernels above).
// ite [n][n_keep] float32, labels [n] -> out [n_labels][n_keep] float64.  Thread (block b, lane t) owns draw d = 64 b + t and ALL its
// labels: it walks the rows in ascending order and adds ite[row][d] into its own column of an LDS table [n_labels][64] of doubles, so
// every output element has one owner, one order, no atomics, and the result does not depend on the grid.  The 64 lanes of a wave
// read 64 consecutive floats of a row (coalesced along n_keep); the row's label is wave-uniform.  A label outside [0, n_labels) is
// counted nowhere.
// ---------------------------------------------------------------------------
#define ITE_GROUP_THREADS 64

__global__ __launch_bounds__(ITE_GROUP_THREADS) void ite_group_sums_kernel(const float *ite, const int *labels, long long n, int n_keep,
                                                                           int n_labels, double *out) {
  extern __shared__ __attribute__((aligned(16))) double ite_group_acc[];      // [n_labels][ITE_GROUP_THREADS]
  const int t = threadIdx.x;
  const long long d = (long long)blockIdx.x * ITE_GROUP_THREADS + t;
  for (int c = 0; c < n_labels; ++c) ite_group_acc[c * ITE_GROUP_THREADS + t] = 0.0;      // (a thread touches its own column only)
  const bool live = d < n_keep;
  const float *col = ite + (live ? d : 0);
  long long row = 0;
  for (; row + 8 <= n; row += 8) {      // eight loads in flight per lane; the additions stay in row order
    float val[8];
    int lab[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      lab[u] = labels[row + u];
      val[u] = live ? col[(row + u) * (long long)n_keep] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if ((unsigned)lab[u] < (unsigned)n_labels) ite_group_acc[lab[u] * ITE_GROUP_THREADS + t] += (double)val[u];
  }
  for (; row < n; ++row) {
    const int lab = labels[row];
    const float val = live ? col[row * (long long)n_keep] : 0.0f;
    if ((unsigned)lab < (unsigned)n_labels) ite_group_acc[lab * ITE_GROUP_THREADS + t] += (double)val;
  }
  if (live)
    for (int c = 0; c < n_labels; ++c) out[(long long)c * n_keep + d] = ite_group_acc[c * ITE_GROUP_THREADS + t];
}
