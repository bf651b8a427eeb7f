// causal_hmc_kernels.h -- CausalBGM log posterior WITH its gradient, and Hamiltonian Monte Carlo with a step size per chain (gfx950).
//
// replaces: nothing in causalbgm/base.py (the reference samples CausalBGM's latents by random-walk MH only, :820-904); the target is
//   get_log_posterior :765-817, the transition is that of bgm/base.py:709-830 (tfp HamiltonianMonteCarlo, identity mass) and the step
//   size is adapted per chain by the Robbins-Monro table of row_adapt.py instead of SimpleStepSizeAdaptation's one step for all chains.
//
// One wave owns 16 chains for the whole launch: z, the momentum, dlogp/dz, the cached log posterior and the step live in registers,
// in the layout one Philox call per lane fills (feature 16 t + 4 r + g in register r of lane group g; the treatment x rides along at
// feature q, as in causal_kernels.h, and is never moved: its momentum and gradient are kept at zero).
// The weights are LDS-resident in the dual-access layout of bgm_kernels.h ([out tile][in row][17], fwd17 / bwd17 / bias17): g's first
// layer and its n_gh hidden layers, the Gram matrix G with [a0 | w_sig | b_sig] (causal_kernels.h, g_last_gram), f and h whole.
// g's Gaussian term is in the anchored Gram form on EVERY shape: with d = a - a0 and y = G d + 2 u,
//     ssq = d . y + c,   dssq/da = 2 y - 2 u,   s_raw = w_sig . a + b_sig
// so neither direction touches the p-wide output layer, G (symmetric: derived in float64, rounded elementwise) is read by fwd17 only,
// and the LDS footprint does not depend on p.  The rows' 2 u and c come from causal_gram_prepass_kernel (65 floats per row, read once
// per launch).  The activation is lrelu_s with the 0.6 folded into the next layer's weights, exactly the network of the Gram copy of
// the sampling blob, so a0 / G / 2 u / c are those of the MH kernel; its derivative is 1 +- BGM_LRS.
// Only the SIGN of every pre-activation is kept for the backward pass (one bit per unit).  The number of hidden layers of g is a
// run-time value: the layer loops are unrolled to CHMC_MAX_GH with wave-uniform guards, so every mask has a register of its own.
// Here: the log posterior with its gradient, the chains' loads and stores and the kernel arguments.  The transition itself, and
// causal_hmc_kernel with it, is chmc_run in causal_hmc_fx_kernels.h.
#pragma once
#include "bgm_kernels.h"

#define CHMC_MAX_GH (BGM_MAX_LAYERS - 1)
#define CHMC_W64 (4 * 64 * 17)      // floats of a 64 -> 64 layer in the dual-access layout

struct CausalHmcMeta {
  int q, p, binary, n_gh;
  float sig2_v, sig2_x, sig2_y;       // fixed variances (sigma^2) if > 0
  // LDS blob offsets (floats); every weight block is [out tile][in row][17]
  int w1g, w1f, w1h;                  // [4][16 KT1][17]: input slot 16 t + 4 g + r holds extended feature 16 t + 4 r + g
  int b1g, b1f, b1h;                  // [64]
  int wg, bg;                         // n_gh x [4][64][17], n_gh x [64]
  int gram, ga;                       // G [4][64][17];  [a0 64 | w_sig 64 | b_sig, 0, 0, 0]
  int wf2, bf2, wf3, bf3, wf4, bf4;   // [2][64][17] / [32];  [1][32][17] / [16];  [1][16][17] / [16]  (tail positions of the sampling blob)
  int wh2, bh2, wh3, bh3, wh4, bh4;
  int total;
};

struct CausalHmcKArgs {
  const float *blob;
  const float *x, *y;
  const float *uc;                    // [n][64] 2 u, then [n] c (causal_gram_prepass_kernel)
  long long n, row_base;
  float *state, *logp, *grad;         // [n x q], [n], [n x q]: in / out (written from the TAG_INIT draw when init = 1)
  float *step;                        // [n] step size of every chain, in / out
  const float *up, *dn;               // [n_table] factor after the decision of iteration it < n_table (moved / did not), or NULL: fixed step
  int n_table;
  float s_min, s_max;
  int init, it_begin, n_iters, burn_in, n_leapfrog;
  unsigned k0, k1;
  unsigned *acc_count;                // [it] += accepted chains, or NULL
  float *draws;                       // [n_keep x n x q] or NULL
  CausalHmcMeta m;
};

template <int NT>
__device__ __forceinline__ unsigned chmc_act(f32x4 (&a)[NT]) {      // a = lrelu_s(a); returns bit 4 t + r = (pre-activation > 0)
  unsigned s = 0u;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s |= (a[t][r] > 0.0f) ? (1u << (4 * t + r)) : 0u;
      a[t][r] = lrelu_s(a[t][r]);
    }
  asm volatile("" : "+v"(s));      // materialise the mask now (else the pre-activations stay live until the backward pass)
  return s;
}
template <int NT>
__device__ __forceinline__ void chmc_dact(f32x4 (&d)[NT], unsigned s) {      // d *= lrelu_s'(pre-activation)
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) d[t][r] *= ((s >> (4 * t + r)) & 1u) ? (1.0f + BGM_LRS) : (1.0f - BGM_LRS);
}
template <int NT>
__device__ __forceinline__ void chmc_zero(f32x4 (&a)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) a[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// Gaussian head with a learned or a fixed variance: nll = r^2 / (2 s2) + dim log(s2) / 2 with rsq = sum of squared residuals;
// returns nll, 1 / s2 and dnll/ds_raw (0 when the variance is fixed)
__device__ __forceinline__ float chmc_gauss(float rsq, float s_raw, float dim, float fixed, float &inv, float &dnll_ds) {
  const bool learned = !(fixed > 0.0f);
  const float s2 = learned ? softplus_f(s_raw) + BGM_EPS : fixed;
  inv = fast_rcp(s2);
  const float sg = fast_rcp(1.0f + fast_exp(-s_raw));      // sigmoid = d softplus / ds
  dnll_ds = learned ? 0.5f * inv * (dim - rsq * inv) * sg : 0.0f;
  return 0.5f * (rsq * inv + dim * fast_log(s2));
}

// the tail of f / h behind the activated first hidden layer a1: 64 -> 32 -> 8 -> (mu, s), the likelihood of the scalar target and the
// gradient back to a1's PRE-activation side (d1 = dlogp/d a1).  which: 0 = f (Gaussian, target y), 1 = h (Gaussian or Bernoulli logit, target x)
// OBS: a row whose target is not observed (has = false; the target may be NaN) has no likelihood term: nll and what enters the
// backward chain are SELECTED to zero -- a product would keep the NaN -- so the chain carries exact zeros and d1 is zero for that row.
template <bool OBS = false>
__device__ __forceinline__ float chmc_tail(const float *lds, int w2, int b2, int w3, int b3, int w4, int b4, int j, int g,
                                           const f32x4 (&a1)[4], float target, bool bernoulli, float fixed, f32x4 (&d1)[4],
                                           bool has = true) {
  f32x4 a2[2], a3[1], a4[1];
  bias17<2>(lds + b2, g, a2);
  fwd17<4, 2>(lds + w2, j, g, a1, a2);
  const unsigned s2m = chmc_act<2>(a2);
  bias17<1>(lds + b3, g, a3);
  fwd17<2, 1>(lds + w3, j, g, a2, a3);
  const unsigned s3m = chmc_act<1>(a3);
  bias17<1>(lds + b4, g, a4);
  fwd17<1, 1>(lds + w4, j, g, a3, a4);
  const float mu = a4[0][0], sr = a4[0][1];      // (the two output columns are replicated for every lane group)
  float nll, dmu, dsr;
  if (bernoulli) {      // sigmoid_cross_entropy_with_logits: max(l, 0) - l x + log1p(exp(-|l|))
    const float e = fast_exp(-fabsf(mu));
    nll = vmax(mu, 0.0f) - mu * target + ((e < 2.44140625e-4f) ? e * (1.0f - 0.5f * e) : fast_log(1.0f + e));
    const float sg = (mu >= 0.0f ? 1.0f : e) * fast_rcp(1.0f + e);
    dmu = target - sg;
    dsr = 0.0f;
  } else {
    const float r = target - mu;
    float inv, dn;
    nll = chmc_gauss(r * r, sr, 1.0f, fixed, inv, dn);
    dmu = r * inv;
    dsr = -dn;
  }
  if constexpr (OBS) nll = has ? nll : 0.0f;
  // dlogp/d(mu, s) enters through lane group 0's copy of the replicated columns only -- and, OBS, only where the row has its target:
  // the mask rides on this select, so the arithmetic that forms dmu and dsr is the one of the kernels without OBS
  const bool enters = OBS ? (g == 0 && has) : (g == 0);
  f32x4 d4[1], d3[1], d2[2];
  d4[0] = f32x4{enters ? dmu : 0.0f, enters ? dsr : 0.0f, 0.0f, 0.0f};
  chmc_zero<1>(d3);
  bwd17<1, 1>(lds + w4, j, g, d4, d3);
  chmc_dact<1>(d3, s3m);
  chmc_zero<2>(d2);
  bwd17<2, 1>(lds + w3, j, g, d3, d2);
  chmc_dact<2>(d2, s2m);
  chmc_zero<4>(d1);
  bwd17<4, 2>(lds + w2, j, g, d2, d1);
  return nll;
}

// log p(z | x, y, v) and dlogp/dz for the 16 chains of a wave.
//   zin : feature 16 t + 4 r + g (z, then x at feature q, then 0)
//   u2  : the row's 2 u in accumulator layout (feature 16 t + 4 g + r);  c: the row's |m0 - v|^2
// logp is replicated over the lane groups; grad has the layout of zin and is zero at every feature >= q.
// OBS (partially observed rows, chmc_observed): the target is p(z | v) or p(z | x, v) -- a row without its outcome (has_y = false)
// has no f term, a row without its treatment (has_x = false; xr is 0 then) no h term; g's term and the prior are those of every row.
// The masked passes add exact zeros to nll and grad, so a row's value does not depend on the patterns of the other rows of its tile.
// No tile skips a net's passes, even where none of its rows has the target: a wave-uniform branch around them was tried in two
// forms and is left out -- it changed hipcc's fused multiply-add choices in the likelihood head, so an
// observed panel was no longer bit-identical to the kernels without OBS, and one form put a kernel into scratch.
template <int KT1, bool OBS = false>
__device__ __forceinline__ void chmc_logp_grad(const float *lds, const CausalHmcMeta &m, int j, int g, const f32x4 (&zin)[KT1],
                                               const f32x4 (&u2)[4], float c, float xr, float yr, float &logp, f32x4 (&grad)[KT1],
                                               bool has_x = true, bool has_y = true) {
  chmc_zero<KT1>(grad);
  float nll;
  // ---- g: Gram form of the covariates' Gaussian term
  {
    unsigned sg[1 + CHMC_MAX_GH];
    f32x4 h[4];
    bias17<4>(lds + m.b1g, g, h);
    fwd17<KT1, 4>(lds + m.w1g, j, g, zin, h);
    sg[0] = chmc_act<4>(h);
#pragma unroll
    for (int l = 0; l < CHMC_MAX_GH; ++l) {
      sg[l + 1] = 0u;
      if (l < m.n_gh) {
        BGM_NO_HOIST();
        f32x4 h2[4];
        bias17<4>(lds + m.bg + l * 64, g, h2);
        fwd17<4, 4>(lds + m.wg + l * CHMC_W64, j, g, h, h2);
        sg[l + 1] = chmc_act<4>(h2);
#pragma unroll
        for (int t = 0; t < 4; ++t) h[t] = h2[t];
      }
    }
    BGM_NO_HOIST();
    const float *a0 = lds + m.ga + 4 * g, *ws = a0 + 64;
    f32x4 d[4], y[4], wsr[4];
    float sp = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 a0t = *reinterpret_cast<const f32x4 *>(a0 + 16 * t);
      wsr[t] = *reinterpret_cast<const f32x4 *>(ws + 16 * t);
      y[t] = u2[t];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d[t][r] = h[t][r] - a0t[r];
        sp = fmaf(wsr[t][r], h[t][r], sp);
      }
    }
    fwd17<4, 4>(lds + m.gram, j, g, d, y);      // y = G d + 2 u
    float ssq = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) ssq = fmaf(d[t][r], y[t][r], ssq);
    ssq = sum_over_g(ssq) + c;
    const float sraw = sum_over_g(sp) + lds[m.ga + 128];
    float inv, dn;
    nll = chmc_gauss(ssq, sraw, (float)m.p, m.sig2_v, inv, dn);
    // dlogp/da = -(dssq/da / (2 s2) + dnll/ds w_sig),  dssq/da = 2 y - 2 u
    f32x4 dh[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[t][r] = -fmaf(inv, y[t][r] - 0.5f * u2[t][r], dn * wsr[t][r]);
#pragma unroll
    for (int l = CHMC_MAX_GH - 1; l >= 0; --l) {
      if (l < m.n_gh) {
        BGM_NO_HOIST();
        chmc_dact<4>(dh, sg[l + 1]);
        f32x4 dp[4];
        chmc_zero<4>(dp);
        bwd17<4, 4>(lds + m.wg + l * CHMC_W64, j, g, dh, dp);
#pragma unroll
        for (int t = 0; t < 4; ++t) dh[t] = dp[t];
      }
    }
    chmc_dact<4>(dh, sg[0]);
    bwd17<KT1, 4>(lds + m.w1g, j, g, dh, grad);
  }
  // ---- f: (z0, z1, x) -> y
  {
    BGM_NO_HOIST();
    f32x4 a1[4], d1[4];
    bias17<4>(lds + m.b1f, g, a1);
    fwd17<KT1, 4>(lds + m.w1f, j, g, zin, a1);
    const unsigned s1 = chmc_act<4>(a1);
    nll += chmc_tail<OBS>(lds, m.wf2, m.bf2, m.wf3, m.bf3, m.wf4, m.bf4, j, g, a1, yr, false, m.sig2_y, d1, has_y);
    chmc_dact<4>(d1, s1);
    bwd17<KT1, 4>(lds + m.w1f, j, g, d1, grad);
  }
  // ---- h: (z0, z2) -> x
  {
    BGM_NO_HOIST();
    f32x4 a1[4], d1[4];
    bias17<4>(lds + m.b1h, g, a1);
    fwd17<KT1, 4>(lds + m.w1h, j, g, zin, a1);
    const unsigned s1 = chmc_act<4>(a1);
    nll += chmc_tail<OBS>(lds, m.wh2, m.bh2, m.wh3, m.bh3, m.wh4, m.bh4, j, g, a1, xr, m.binary != 0, m.sig2_x, d1, has_x);
    chmc_dact<4>(d1, s1);
    bwd17<KT1, 4>(lds + m.w1h, j, g, d1, grad);
  }
  // ---- prior -|z|^2 / 2; the slots behind the latent features (x, padding) carry no gradient
  float zsq = 0.0f;
#pragma unroll
  for (int t = 0; t < KT1; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool lat = 16 * t + 4 * r + g < m.q;
      const float zz = lat ? zin[t][r] : 0.0f;
      zsq = fmaf(zz, zz, zsq);
      grad[t][r] = lat ? grad[t][r] - zz : 0.0f;
    }
  logp = -(nll + 0.5f * sum_over_g(zsq));
}

// the row's x, y, 2 u and c (row clamped by the caller)
__device__ __forceinline__ void chmc_load_row(const float *x, const float *y, const float *uc, long long n, long long row, int g, float &xr,
                                              float &yr, f32x4 (&u2)[4], float &c) {
  xr = x[row];
  yr = y[row];
  const f32x4 *ur = reinterpret_cast<const f32x4 *>(uc + row * 64);
#pragma unroll
  for (int t = 0; t < 4; ++t) u2[t] = ur[4 * t + g];
  c = uc[64 * n + row];
}
// OBS: the observation pattern of a row is carried by its data -- x or y is NaN where it is not observed.  Returns the pattern
// and replaces a missing x by 0, the value its input slot (feature q of z) then holds.
__device__ __forceinline__ void chmc_observed(float &xr, float yr, bool &has_x, bool &has_y) {
  has_x = (xr == xr);
  has_y = (yr == yr);
  xr = has_x ? xr : 0.0f;
}
template <int KT1>
__device__ __forceinline__ void chmc_load_z(const float *z, int q, long long row, int g, float xr, f32x4 (&zin)[KT1]) {
  const float *zr = z + row * (long long)q;
#pragma unroll
  for (int t = 0; t < KT1; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * t + 4 * r + g;
      const float val = zr[f < q ? f : q - 1];      // unconditional in-bounds load, then select
      zin[t][r] = (f < q) ? val : (f == q ? xr : 0.0f);
    }
}
template <int KT1>
__device__ __forceinline__ void chmc_store_z(float *z, int q, long long row, int g, const f32x4 (&zin)[KT1]) {
  float *zr = z + row * (long long)q;
#pragma unroll
  for (int t = 0; t < KT1; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * t + 4 * r + g;
      if (f < q) zr[f] = zin[t][r];
    }
}

// get_log_posterior and its gradient for n rows (one evaluation); OBS: causal_hmc_obs_logpost_kernel (causal_hmc_obs_kernels.h)
template <int KT1, int WAVES, bool OBS = false>
__device__ __forceinline__ void chmc_logpost_run(float *lds, const float *blob, CausalHmcMeta m, const float *x, const float *y,
                                                 const float *uc, const float *z, long long n, float *out_logp, float *out_grad) {
  lds_fill(lds, blob, m.total);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const long long n_tiles = (n + 15) / 16;
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    BGM_NO_HOIST();
    long long row = tile * 16 + j;
    const bool ok = row < n;
    row = ok ? row : n - 1;
    float xr, yr, c, lp;
    f32x4 u2[4], zin[KT1], gr[KT1];
    chmc_load_row(x, y, uc, n, row, g, xr, yr, u2, c);
    bool has_x = true, has_y = true;
    if constexpr (OBS) chmc_observed(xr, yr, has_x, has_y);
    chmc_load_z<KT1>(z, m.q, row, g, xr, zin);
    chmc_logp_grad<KT1, OBS>(lds, m, j, g, zin, u2, c, xr, yr, lp, gr, has_x, has_y);
    if (ok) {
      if (g == 0) out_logp[row] = lp;
      chmc_store_z<KT1>(out_grad, m.q, row, g, gr);
    }
  }
}

template <int KT1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_logpost_kernel(const float *blob, CausalHmcMeta m, const float *x, const float *y,
                                                                        const float *uc, const float *z, long long n, float *out_logp,
                                                                        float *out_grad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_logpost_run<KT1, WAVES>(lds, blob, m, x, y, uc, z, n, out_logp, out_grad);
}
