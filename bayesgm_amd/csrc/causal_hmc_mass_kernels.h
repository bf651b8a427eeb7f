// causal_hmc_mass_kernels.h -- the HMC transition of causal_hmc_kernels.h with a diagonal metric per chain (gfx950).
//
// replaces: nothing in causalbgm/base.py; tfp's HamiltonianMonteCarlo (bgm/base.py:709-830) has identity mass only.
//
// causal_hmc_mass_kernel is causal_hmc_kernel (same registers, same LDS blob, same RNG streams, same accept rule and step table)
// with the differences described below.  It is a kernel of its own beside the old one, not a flag on a shared body: the
// identity-mass kernels keep their code objects instruction for instruction (scripts/compare_code_objects.py).
//
#pragma once
#include "causal_hmc_kernels.h"

// The metric (bgm_causal_hmc_set_mass): diagonal, one per chain, in the scaled form.  The chain carries s in R^q (M^-1 = diag(s^2));
// momentum and kinetic energy are those of identity mass and only the step becomes a vector, es_i = eps s_i, in the position step
// and in the kicks.  With s = 1 every product is exact and the run is the identity-mass run bit for bit.  While ma.accumulate is set
// the moments of d = z - ref are added after every decision, S1 += d, S2 = fma(d, d, S2), in global memory ([n x q] each, one owner
// lane per element): ref is the chain's state at the window's start, which removes the cancellation in S2 / W - mean^2 when
// sd << |mean|; causal_hmc_mass_update_kernel turns them into the next s between two launches.
// s is NOT held in registers: causal_hmc_kernel<2, 8> is at 223 of 256 VGPRs, and 8 more live across chmc_logp_grad spill.  It is read
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

template <int KT1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CausalHmcMeta &m = a.m;
  lds_fill(lds, a.blob, m.total);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const long long n = a.n, n_tiles = (n + 15) / 16;
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    BGM_NO_HOIST();
    long long row = tile * 16 + j;
    const bool ok = row < n;
    row = ok ? row : n - 1;
    const unsigned rowid = (unsigned)(a.row_base + row);
    float xr, yr, c, lp;
    f32x4 u2[4], z[KT1], gr[KT1];
    chmc_load_row(a.x, a.y, a.uc, n, row, g, xr, yr, u2, c);
    float eps = a.step[row];
    const long long eoff = row * (long long)m.q + g;      // the lane's first element of the row's [q] in scale / ref / s1 / s2
    if (a.init) {      // current_state ~ N(0, 1) (base.py:842), RNG tag 0: the state the MH sampler starts from
#pragma unroll
      for (int t = 0; t < KT1; ++t) {
        const f32x4 e = box_muller4(philox4x32_10(rowid, 0u, (unsigned)(g + 4 * t), TAG_INIT, a.k0, a.k1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 16 * t + 4 * r + g;
          z[t][r] = (f < m.q) ? e[r] : (f == m.q ? xr : 0.0f);
        }
      }
      chmc_logp_grad<KT1>(lds, m, j, g, z, u2, c, xr, yr, lp, gr);
    } else {
      chmc_load_z<KT1>(a.state, m.q, row, g, xr, z);
      chmc_load_z<KT1>(a.grad, m.q, row, g, 0.0f, gr);
      lp = a.logp[row];
    }
    for (int it = a.it_begin; it < a.it_begin + a.n_iters; ++it) {
      BGM_NO_HOIST();
      f32x4 mom[KT1], zc[KT1], gc[KT1], sc[KT1];
      chmc_mass_load<KT1>(ma.scale, eoff, m.q, g, sc);
      float ke0 = 0.0f;
#pragma unroll
      for (int t = 0; t < KT1; ++t) {
        const f32x4 e = box_muller4(philox4x32_10(rowid, (unsigned)it, (unsigned)(g + 4 * t), TAG_MOM, a.k0, a.k1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pm = (16 * t + 4 * r + g < m.q) ? e[r] : 0.0f;
          ke0 = fmaf(pm, pm, ke0);
          mom[t][r] = fmaf(0.5f * (eps * sc[t][r]), gr[t][r], pm);      // first half kick
          zc[t][r] = z[t][r];
          gc[t][r] = gr[t][r];
        }
      }
      ke0 = sum_over_g(ke0);
      float lpc = lp;
      for (int l = 0; l < a.n_leapfrog; ++l) {
        BGM_NO_HOIST();
        chmc_mass_load<KT1>(ma.scale, eoff, m.q, g, sc);
#pragma unroll
        for (int t = 0; t < KT1; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) zc[t][r] = fmaf(eps * sc[t][r], mom[t][r], zc[t][r]);      // (the momentum of x and of the padding is zero)
        chmc_logp_grad<KT1>(lds, m, j, g, zc, u2, c, xr, yr, lpc, gc);
        BGM_NO_HOIST();
        chmc_mass_load<KT1>(ma.scale, eoff, m.q, g, sc);
        const float kick = (l < a.n_leapfrog - 1) ? eps : 0.5f * eps;
#pragma unroll
        for (int t = 0; t < KT1; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) mom[t][r] = fmaf(kick * sc[t][r], gc[t][r], mom[t][r]);      // (0.5 eps) s = 0.5 (eps s): a power of two
      }
      float ke1 = 0.0f;
#pragma unroll
      for (int t = 0; t < KT1; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) ke1 = fmaf(mom[t][r], mom[t][r], ke1);
      ke1 = sum_over_g(ke1);
      float log_ratio = -((-lpc + 0.5f * ke1) - (-lp + 0.5f * ke0));
      log_ratio = (log_ratio == log_ratio && fabsf(log_ratio) != INFINITY) ? log_ratio : -INFINITY;
      const uint4 w4 = philox4x32_10(rowid, (unsigned)it >> 2, 0u, TAG_HACC, a.k0, a.k1);
      const unsigned w_ = (it & 2) ? ((it & 1) ? w4.w : w4.z) : ((it & 1) ? w4.y : w4.x);
      const bool acc = logf(u01_open(w_)) < log_ratio;
#pragma unroll
      for (int t = 0; t < KT1; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          z[t][r] = acc ? zc[t][r] : z[t][r];
          gr[t][r] = acc ? gc[t][r] : gr[t][r];
        }
      lp = acc ? lpc : lp;
      if (a.up != nullptr && it < a.n_table) eps = fminf(fmaxf(eps * (acc ? a.up : a.dn)[it], a.s_min), a.s_max);
      if (a.acc_count) {
        const unsigned cnt = (unsigned)__popcll(__ballot(acc && ok && g == 0));
        if (lane == 0 && cnt) atomicAdd(a.acc_count + it, cnt);
      }
      if (ma.accumulate && ok) {
        long long off = eoff;
        asm volatile("" : "+v"(off));
        const float *rf = ma.ref + off;
        float *s1 = ma.s1 + off, *s2 = ma.s2 + off;
#pragma unroll
        for (int t = 0; t < KT1; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int e = 16 * t + 4 * r;
            if (e + g < m.q) {
              const float d = z[t][r] - rf[e];
              s1[e] += d;
              s2[e] = fmaf(d, d, s2[e]);
            }
          }
      }
      if (a.draws != nullptr && it >= a.burn_in && ok) chmc_store_z<KT1>(a.draws + (long long)(it - a.burn_in) * n * m.q, m.q, row, g, z);
    }
    if (ok) {
      chmc_store_z<KT1>(a.state, m.q, row, g, z);
      chmc_store_z<KT1>(a.grad, m.q, row, g, gr);
      if (g == 0) { a.logp[row] = lp; a.step[row] = eps; }
    }
  }
}
