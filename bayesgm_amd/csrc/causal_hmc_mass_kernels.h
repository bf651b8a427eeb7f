// causal_hmc_mass_kernels.h -- the HMC transition of causal_hmc_kernels.h with a diagonal metric per chain (gfx950).
//
// replaces: nothing in causalbgm/base.py; tfp's HamiltonianMonteCarlo (bgm/base.py:709-830) has identity mass only.
//
// causal_hmc_mass_kernel is causal_hmc_kernel (same registers, same LDS blob, same RNG streams, same accept rule and step table)
// with the differences described below: both are chmc_run (causal_hmc_fx_kernels.h), MASS is its template argument.  Here: the
// metric's kernel arguments and the load of a chain's scales.
//
#pragma once
#include "causal_hmc_kernels.h"

// The metric (bgm_causal_hmc_set_mass): diagonal, one per chain, in the scaled form.  The chain carries s in R^q (M^-1 = diag(s^2));
// momentum and kinetic energy are those of identity mass and only the step becomes a vector, es_i = eps s_i, in the position step
// and in the kicks.  With s = 1 every product is exact and the run is the identity-mass run bit for bit.  While ma.accumulate is set
// the moments of d = z - ref are added after every decision, S1 += d, S2 = fma(d, d, S2), in global memory ([n x q] each, one owner
// lane per element): ref is the chain's state at the window's start, which removes the cancellation in S2 / W - mean^2 when
// sd << |mean|; causal_hmc_mass_update_kernel turns them into the next s between two launches.
// s is NOT held in registers: causal_hmc_kernel<2, 8> is at 224 of 256 VGPRs, and 8 more live across chmc_logp_grad spill.  It is read
// again from global memory (cache-resident: 4 q bytes per chain) at each of its three uses, 2 n_leapfrog + 1 reads of [q] per
// transition against the hundreds of matrix instructions of one gradient; the memory clobbers of BGM_NO_HOIST keep the reads apart.
// Every [n x q] array is addressed from ONE 64-bit element offset per lane (row q + g; the features of a lane are 16 t + 4 r behind
// it, immediates), passed through an empty asm at each use: otherwise the loop-invariant addresses of all 8 KT1 elements of all four
// arrays are hoisted out of the iteration loop and held in registers (+ 30 VGPRs, spills at KT1 = 2).
struct CausalHmcMassArgs {
  const float *scale;                 // [n x q] s of every chain
  const float *ref;                   // [n x q] reference point of the moments
  float *s1, *s2;                     // [n x q] sums of d and d^2, +=
  int accumulate;
};

// element 16 t + 4 r behind p, the lane's feature 16 t + 4 r + g, for the latent features; 0 behind them (their momentum is 0 too)
template <int KT1>
__device__ __forceinline__ void chmc_mass_load(const float *base, long long off, int q, int g, f32x4 (&v)[KT1]) {
  asm volatile("" : "+v"(off));
  const float *p = base + off;
#pragma unroll
  for (int t = 0; t < KT1; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[t][r] = 0.0f;
      if (16 * t + 4 * r + g < q) v[t][r] = p[16 * t + 4 * r];
    }
}
