// causal_kernels.h -- CausalBGM log-posterior / Metropolis-Hastings kernels (gfx950).
//
// replaces (reference file:line, all in src/bayesgm/models/causalbgm/base.py):
//   get_log_posterior            :765-817   -> causal_logp<> (device), causal_logpost_kernel
//   metropolis_hastings_sampler  :820-904   -> causal_mh_kernel (persistent over iterations)
//   infer_from_latent_posterior  :671-763   -> fused into causal_mh_kernel (EFFECT != 0)
//
// One wave owns R groups of 16 chains for the whole segment of iterations: its V
// rows (R x NTL x 4 VGPRs), x, y, the chain state and the cached log-posterior
// stay in registers; the g/f/h weights (about 150 KB fp32 at p = 200) stay in
// LDS, shared by the block's waves.  Per transition only the Philox counters
// change; HBM is touched again only to emit retained draws / effects.
#pragma once
#include <type_traits>
#include <utility>

#include "bgm_device.h"
#include "row_tails.h"

struct CausalMeta {
  int q, p;
  int sig_pc, sig_slot; // g's variance column (feature p) sits at element sig_pc of the LAST output tile = padded column sig_slot
  int binary;
  float sig2_v, sig2_x, sig2_y;  // fixed variances (sigma^2) if > 0
  int n_gh;             // number of hidden->hidden 64x64 layers of g
  // LDS blob offsets (floats)
  int w1g, w1f, w1h, b1g, b1f, b1h;
  int wg, bg;           // n_gh consecutive [64][64] / [64]
  int wgl, bgl;         // last g layer [64][16*NTL] / [16*NTL]  (Gram copy of the blob: G [64][64] / [a0 | w_sig | b_sig], g_last_gram)
  int wf2, bf2, wf3, bf3, wf4, bf4;
  int wh2, bh2, wh3, bh3, wh4, bh4;
  int wxf;              // f L1 x-row, accumulator layout [64]
  // vector-ALU copy of f's layers 3 and 4 (sampling copies only, causal_scale_blob_kernel; read by causal_dose_passes_valu):
  int vf3;              // [lane group g][local input 4 u + r = feature 16 u + 4 g + r][8 outputs], scaled like wf3
  int vf4;              // [8 inputs][2 outputs] scaled like wf4, then layer 3's bias [8], then layer 4's bias [2] (+ 2 of padding)
  int total;            // blob floats
  // First-layer K-steps to issue, bit s = K-step s (extended input features 4 s .. 4 s + 3): the steps in which the net takes at least
  // one feature.  From z_dims alone (causal_pack_forward), never from weight values; every other step multiplies packed zeros.
  // l1f: f (z0, z1, x); l1h: h (z0, z2); l1b: f without the treatment column (causal_effects' dose-free `base`).  g runs every step.
  unsigned l1f, l1h, l1b;
};
// The MH kernel instantiations that keep the unmasked first layers: with the conditional prior and a two-tile first layer (PriorRow's
// registers on top of KT1 = 2) the masked forms made the Gram instances spill 72 bytes per lane where they had 12 (0 -> 12 in the
// event form's transition kernel).  Compile-time; bgm_causal_mh_info counts every K-step for them.
__host__ __device__ constexpr bool causal_l1_masked(int KT1, int PRIOR) { return !(PRIOR != 0 && KT1 > 1); }

// The fused keep instantiations (causal_mh_kernel<EFFECT 1>) that run the tail of f in their dose passes on the vector ALU (VTAILS):
// every one that gained no scratch by it.  Left on the matrix pipe: the Gram instances with a two-tile first layer (0 -> 20 bytes per
// lane), the direct form at 7 output tiles (0 -> 56 and 64 -> 80 bytes; it runs only under BGM_MH_DIRECT_LIKELIHOOD), with the
// per-chain proposal scale also the two-tile first layer at 2 output tiles (0 -> 20), and every instance with the conditional prior
// (0 -> 44 in its Gram instances, 0 -> 28 / 100 at 2 output tiles).  Compile-time, like causal_l1_masked.
__host__ __device__ constexpr bool causal_valu_tails(int KT1, int NTL, bool GRAM, bool ROWADAPT = false) {
  return !(KT1 > 1 && GRAM) && !(NTL == 7 && !GRAM) && !(ROWADAPT && KT1 > 1 && NTL == 2);
}

struct CausalMhKArgs {
  const float *blob;    // packed weights (global)
  const float *x, *y, *v;
  const float *uc;          // Gram form of g's likelihood (GRAM): [n][64] 2 u, then [n] c per local row (causal_gram_prepass_kernel); else NULL
  long long n, row_base;
  float *state, *logp;
  int init, it_begin, n_iters, burn_in;
  float q_sd;
  unsigned k0, k1;
  unsigned *acc_count;
  float *draws;
  int n_keep, sample_y, n_doses;
  const float *x_values;
  float *adrf_partial;
  float *ite;
  unsigned long long *clk;
  const int *seg;           // conditional prior (IdentifiableCausalBGM): segment of every local row, or NULL
  const float *prior_tab;   // [n_segments][q + 2]: mu(u) [q], 1 / sigma^2(u), (q / 2) log sigma^2(u)
  float *eff_cache;         // ADRF kernels with one row tile per wave: [n_slots][ceil(n_doses / 4)][64][2] (mean, sd) of the lane's dose
  int eff_skip;             // 1: a retained iteration in which no chain of the wave moved reuses the cached (mean, sd)
  unsigned long long *eff_stats;   // [0] += retained tile-iterations served from the cache (the total is known on the host), or NULL
  // EFFECT == 3 (causal_event_kernels.h): the retained iterations only append EVENTS -- (chain, first retained draw, state) of every
  // accepted move -- to the wave slot's region; the outcome net runs on dense event tiles afterwards
  float *ev_z;              // [n_slots * ev_cap][q]
  unsigned *ev_meta;        // [n_slots * ev_cap]: (iteration - it_begin) << 4 | chain of the tile
  int *tile_ev;             // [n_tiles][2]: first event of the tile within its slot's region, number of events
  int *slot_cnt;            // [n_slots]: events of the slot
  long long ev_cap;         // events a slot's region holds (a multiple of 16)
  int ev_first;             // 1: every chain emits its state at the launch's first iteration (nothing is carried from an earlier launch)
  CausalMeta m;
  // ROWADAPT (bgm_causal_set_row_scale; behind m: the kernel arguments of the fixed-scale instantiations keep their offsets):
  float *row_scale;         // [n] proposal scale of every local row, in / out (written from q_sd when init = 1)
  const float *ra_up, *ra_dn;   // [ra_n]: factor applied to a chain's scale after iteration it < ra_n, accepted / rejected
  int ra_n;                 // iterations >= ra_n leave the scale alone (burn_in through the classes: the retained chain is plain MH)
  float ra_min, ra_max;     // clamp of the scale
};

// ---------------------------------------------------------------------------
// log p(z | x, y, v) for R x 16 chains held by one wave.
//   zin  : L1 input tiles, feature 16 t + 4 r + g  (z features, then x at index q, then 0)
//   vreg : (bias of g's last layer) - (V row), feature 16 t + 4 g + r (load_v_rows); the variance slot holds the bias alone
//          (GRAM: the row's 2 u and c instead, load_gram_rows / g_last_gram)
// Returns logp[rr] replicated over the four lane groups.
// ---------------------------------------------------------------------------
template <int T0, int KT, int NTL, int R>
__device__ __forceinline__ void g_last_groups(const float *wl, const float *bl, int lane_off, int g,
                                              int sig_r, const f32x4 (&in)[R][KT],
                                              const f32x4 (&vreg)[R][NTL], float (&ssq)[R],
                                              float (&sraw)[R]) {
  if constexpr (T0 < NTL) {
    constexpr int GS = group_size(NTL - T0);
    f32x4 acc[R][NTL];  // only [T0, T0+GS) is touched; the rest is dead and never allocated
    constexpr int K_ROWS = 16 * KT;
    constexpr int NKS = 4 * KT;
    const float *base = wl + K_ROWS * 16 * T0 + lane_off * GS;
    bool done = false;
#ifndef BGM_NO_ASM_DENSE
    if constexpr (R == 1 && KT == 4 && GS == 4) {
      dense_group4_k64_asm_c(lds_byte_addr(base), in[0], vreg[0][T0], vreg[0][T0 + 1], vreg[0][T0 + 2], vreg[0][T0 + 3], acc[0][T0],
                             acc[0][T0 + 1], acc[0][T0 + 2], acc[0][T0 + 3]);
      done = true;
    }
#endif
    if (!done) {       // accumulators start from bias - v
#pragma unroll
      for (int u = 0; u < GS; ++u)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) acc[rr][T0 + u] = vreg[rr][T0 + u];
    }
    if constexpr (R == 1 && NKS * GS <= BGM_PREFETCH_ALL_MAX) {   // the single trailing tile: see dense_groups
      AFrag<GS> af[NKS];
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) af[ks].load(base + (16 * (ks >> 2) + (ks & 3)) * 16 * GS);
      BGM_NO_HOIST();
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int u = 0; u < GS; ++u) acc[0][T0 + u] = BGM_MFMA(af[ks].get(u), in[0][ks >> 2][ks & 3], acc[0][T0 + u]);
      done = true;
    }
    if (!done) {
      AFrag<GS> a_cur, a_nxt;
      a_cur.load(base);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const int t = ks >> 2, r = ks & 3;
        if (ks + 1 < NKS) a_nxt.load(base + (16 * ((ks + 1) >> 2) + ((ks + 1) & 3)) * 16 * GS);
#pragma unroll
        for (int u = 0; u < GS; ++u)
#pragma unroll
          for (int rr = 0; rr < R; ++rr)
            acc[rr][T0 + u] = BGM_MFMA(a_cur.get(u), in[rr][t][r], acc[rr][T0 + u]);
        a_cur = a_nxt;
      }
    }
#pragma unroll
    for (int u = 0; u < GS; ++u) {
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float d = acc[rr][T0 + u][r];            // mu - v
          if (T0 + u == NTL - 1) {  // tile holding the variance column (feature p)
            const bool is_sig = (r == sig_r);
            sraw[rr] = is_sig ? acc[rr][T0 + u][r] : sraw[rr];
            d = is_sig ? 0.0f : d;
          }
          ssq[rr] = fmaf(d, d, ssq[rr]);
        }
      }
    }
    g_last_groups<T0 + GS, KT, NTL, R>(wl, bl, lane_off, g, sig_r, in, vreg, ssq, sraw);
  }
}

// ---------------------------------------------------------------------------
// Gram form of g's Gaussian term (the MH kernel on the shapes where it issues fewer MFMAs, NTL > 2).  With a = g's last hidden
// activation (lrelu_s scaling), W [64 x p] / b the mean columns of the (scaled) output layer, a0 the activation at z = 0 and
// m0 = W^T a0 + b (per model), and per row u = W (m0 - v), c = |m0 - v|^2:
//     |W^T a + b - v|^2 = d^T (G d + 2 u) + c,   d = a - a0,  G = W W^T  [64 x 64]
// so the 16 NTL MFMAs of the output layer become the 16 of one 64 x 64 product.  The anchor a0 keeps the cancellation relative
// to |g(0) - v|^2; d is formed explicitly in fp32 (folding a0 into u would give back the unanchored form).
// LDS (the Gram copy of the sampling blob, bgm_causal_gram_blob): m.wgl = G packed as a hidden layer, m.bgl = [a0 | w_sig | b_sig],
// natural feature order.  vreg: tiles 0-3 = 2 u in accumulator layout (feature 16 t + 4 g + r), tile 4 = (c, 0, 0, 0) in lane
// group 0 and zero elsewhere (load_gram_rows).  Returns per-lane partials of the squared residual (summed over g by the caller)
// and the raw variance output s = w_sig . a + b_sig, valid in every lane.
// ---------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void g_last_gram(const float *lds, const CausalMeta &m, int lane_off, int g, const f32x4 (&h)[R][4],
                                            const f32x4 (&vreg)[R][5], float (&ssq)[R], float (&sraw)[R]) {
  const float *a0 = lds + m.bgl + 4 * g, *ws = a0 + 64;
  f32x4 d[R][4];
  float sp[R];
#pragma unroll
  for (int rr = 0; rr < R; ++rr) sp[rr] = 0.0f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f32x4 a0t = *reinterpret_cast<const f32x4 *>(a0 + 16 * t);
    const f32x4 wst = *reinterpret_cast<const f32x4 *>(ws + 16 * t);
#pragma unroll
    for (int rr = 0; rr < R; ++rr)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d[rr][t][r] = h[rr][t][r] - a0t[r];
        sp[rr] = fmaf(wst[r], h[rr][t][r], sp[rr]);
      }
  }
  f32x4 y[R][4];
  const float *base = lds + m.wgl + lane_off * 4;
  bool done = false;
#ifndef BGM_NO_ASM_DENSE
  if constexpr (R == 1) {
    dense_group4_k64_asm_c(lds_byte_addr(base), d[0], vreg[0][0], vreg[0][1], vreg[0][2], vreg[0][3], y[0][0], y[0][1], y[0][2], y[0][3]);
    done = true;
  }
#endif
  if (!done) {
#pragma unroll
    for (int rr = 0; rr < R; ++rr)
#pragma unroll
      for (int u = 0; u < 4; ++u) y[rr][u] = vreg[rr][u];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      AFrag<4> af;
      af.load(base + (16 * (ks >> 2) + (ks & 3)) * 16 * 4);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) y[rr][u] = BGM_MFMA(af.get(u), d[rr][ks >> 2][ks & 3], y[rr][u]);
    }
  }
  const float bs = lds[m.bgl + 128];
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    float s = vreg[rr][4][0];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) s = fmaf(d[rr][t][r], y[rr][t][r], s);
    ssq[rr] = s;
    sraw[rr] = sum_over_g(sp[rr]) + bs;
  }
}

// f / h tail:  64 -> 32 -> 8 -> 2   (f_units = h_units = [64, 32, 8]); a1 is the
// activated first hidden layer.  Returns the raw outputs (mu, s) of every row group, valid in every lane
// (the sampling blob replicates the two output columns for all lane groups, see above causal_effects).
template <int R>
__device__ __forceinline__ void fh_tail(const float *lds, int w2, int b2, int w3, int b3, int w4,
                                        int b4, int lane_off, int g,
                                        const f32x4 (&a1)[R][4], float (&mu)[R], float (&sr)[R]) {
  f32x4 a2[R][2];
  dense<4, 4, 2, R>(lds + w2, lds + b2, lane_off, g, a1, a2);
  lrelu_s_inplace<2, R>(a2);
  f32x4 a3[R][1];
  dense<2, 4, 1, R>(lds + w3, lds + b3, lane_off, g, a2, a3);
  lrelu_s_inplace<1, R>(a3);
  f32x4 a4[R][1];
  dense<1, 2, 1, R>(lds + w4, lds + b4, lane_off, g, a3, a4);   // two K-steps: see the sampling-blob layout above causal_effects
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    mu[rr] = a4[rr][0][0];
    sr[rr] = a4[rr][0][1];
  }
}

#ifdef BGM_PROF
#define PMARK(i) do { const unsigned long long _t = __builtin_readcyclecounter(); tsec[i] += _t - tlast; tlast = _t; } while (0)
#else
#define PMARK(i)
#endif
template <int KT1, int KSL1, int NTL, int R, bool GRAM = false, bool L1MASK = true>
__device__ __forceinline__ void causal_logp(const float *lds, const CausalMeta &m, int lane_off, int g,
                                            int j, const f32x4 (&zin)[R][KT1],
                                            const f32x4 (&vreg)[R][GRAM ? 5 : NTL], const float (&xr)[R],
                                            const float (&yr)[R], float (&logp)[R]
#ifdef BGM_PROF
                                            , unsigned long long (&tsec)[8], unsigned long long &tlast
#endif
                                            ) {
  // ---- g : z -> (mu_v, s_v), Gaussian NLL over p covariates (base.py:779-801)
  float ssq[R], sraw_v[R];
  {
    f32x4 h[R][4];
    dense<KT1, KSL1, 4, R>(lds + m.w1g, lds + m.b1g, lane_off, g, zin, h);
    lrelu_s_inplace<4, R>(h);
    PMARK(1);
    bool hidden_done = false;
#ifndef BGM_NO_ASM_HIDDEN4
    if constexpr (R == 1) {
      if (m.n_gh == 4) {   // g_units = [64]*5 (every shipped config): all four hidden layers as one scheduled block
        f32x4 q[4];
        dense_hidden4_asm(lds_byte_addr(lds + m.wg + lane_off * 4), lds_byte_addr(lds + m.bg + 4 * g), h[0], q);
        lrelu_s_inplace<4, 1>(h);
        hidden_done = true;
      }
    }
#endif
    if (!hidden_done) {
      for (int l = 0; l < m.n_gh; ++l) {
        BGM_NO_HOIST();
        f32x4 h2[R][4];
        dense<4, 4, 4, R>(lds + m.wg + l * 4096, lds + m.bg + l * 64, lane_off, g, h, h2);
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[rr][t][r] = lrelu_s(h2[rr][t][r]);
      }
    }
    PMARK(2);
#pragma unroll
    for (int rr = 0; rr < R; ++rr) { ssq[rr] = 0.0f; sraw_v[rr] = 0.0f; }
    if constexpr (GRAM) {
      g_last_gram<R>(lds, m, lane_off, g, h, vreg, ssq, sraw_v);
    } else {
      const int pc = m.sig_pc;  // position of the variance column inside the last tile (see bgm_g_last_padded)
      g_last_groups<0, 4, NTL, R>(lds + m.wgl, lds + m.bgl, lane_off, g, pc - 4 * g, h, vreg, ssq, sraw_v);
#pragma unroll
      for (int rr = 0; rr < R; ++rr) sraw_v[rr] = __shfl(sraw_v[rr], j + 16 * (pc >> 2));
    }
    PMARK(3);
  }
  // ---- f : (z0, z1, x) -> (mu_y, s_y)   (base.py:793-798)  and  h : (z0, z2) -> (mu_x | logit, s_x)   (:786-791)
  float mu_y[R], sr_y[R], mu_x[R], sr_x[R];
  if constexpr (R == 1) {   // the two small nets in lock step (see dense_pair)
    f32x4 f1[1][4], h1[1][4];
    if constexpr (L1MASK) dense_pair_masked<KT1, KSL1, 4>(lds + m.w1f, lds + m.b1f, lds + m.w1h, lds + m.b1h, lane_off, g, zin, zin, f1, h1, m.l1f, m.l1h);
    else dense_pair<KT1, KSL1, 4>(lds + m.w1f, lds + m.b1f, lds + m.w1h, lds + m.b1h, lane_off, g, zin, zin, f1, h1);
    lrelu_s_inplace<4, 1>(f1); lrelu_s_inplace<4, 1>(h1);
    f32x4 f2[1][2], h2[1][2];
    dense_pair<4, 4, 2>(lds + m.wf2, lds + m.bf2, lds + m.wh2, lds + m.bh2, lane_off, g, f1, h1, f2, h2);
    lrelu_s_inplace<2, 1>(f2); lrelu_s_inplace<2, 1>(h2);
    f32x4 f3[1][1], h3[1][1];
    dense_pair<2, 4, 1>(lds + m.wf3, lds + m.bf3, lds + m.wh3, lds + m.bh3, lane_off, g, f2, h2, f3, h3);
    lrelu_s_inplace<1, 1>(f3); lrelu_s_inplace<1, 1>(h3);
    f32x4 f4[1][1], h4[1][1];
    dense_pair<1, 2, 1>(lds + m.wf4, lds + m.bf4, lds + m.wh4, lds + m.bh4, lane_off, g, f3, h3, f4, h4);   // two K-steps (permuted layer-3 outputs)
    mu_y[0] = f4[0][0][0]; sr_y[0] = f4[0][0][1];
    mu_x[0] = h4[0][0][0]; sr_x[0] = h4[0][0][1];
  } else {
    {
      f32x4 a1[R][4];
      dense_masked<KT1, KSL1, 4, R>(lds + m.w1f, lds + m.b1f, lane_off, g, zin, a1, m.l1f);
      lrelu_s_inplace<4, R>(a1);
      fh_tail<R>(lds, m.wf2, m.bf2, m.wf3, m.bf3, m.wf4, m.bf4, lane_off, g, a1, mu_y, sr_y);
    }
    {
      f32x4 a1[R][4];
      dense_masked<KT1, KSL1, 4, R>(lds + m.w1h, lds + m.b1h, lane_off, g, zin, a1, m.l1h);
      lrelu_s_inplace<4, R>(a1);
      fh_tail<R>(lds, m.wh2, m.bh2, m.wh3, m.bh3, m.wh4, m.bh4, lane_off, g, a1, mu_x, sr_x);
    }
  }
  PMARK(4);
  // ---- assemble -(loss_v + loss_x + loss_y + |z|^2/2)   (base.py:800-816)
  // the x / y losses are identical in the four lane groups of a row: they are counted once (lane group 0) and
  // folded into the per-lane partial that is summed over g, so one reduction serves all terms.
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    float zsq = 0.0f;
#pragma unroll
    for (int t = 0; t < KT1; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float zz = zin[rr][t][r];
        zsq = (16 * t + 4 * r + g < m.q) ? fmaf(zz, zz, zsq) : zsq;
      }
    const float s2v = (m.sig2_v > 0.0f) ? m.sig2_v : softplus_f(sraw_v[rr]) + BGM_EPS;
    float loss_x;
    if (m.binary) {
      const float l = mu_x[rr];
      const float e = fast_exp(-fabsf(l));
      loss_x = vmax(l, 0.0f) - l * xr[rr] + ((e < 2.44140625e-4f) ? e * (1.0f - 0.5f * e) : fast_log(1.0f + e));
    } else {
      const float s2x = (m.sig2_x > 0.0f) ? m.sig2_x : softplus_f(sr_x[rr]) + BGM_EPS;
      const float dx = xr[rr] - mu_x[rr];
      loss_x = 0.5f * (dx * dx * fast_rcp(s2x) + fast_log(s2x));
    }
    const float s2y = (m.sig2_y > 0.0f) ? m.sig2_y : softplus_f(sr_y[rr]) + BGM_EPS;
    const float dy = yr[rr] - mu_y[rr];
    const float loss_y = 0.5f * (dy * dy * fast_rcp(s2y) + fast_log(s2y));
    float part = 0.5f * (ssq[rr] * fast_rcp(s2v) + zsq);
    part += (g == 0) ? (loss_x + loss_y) : 0.0f;
    logp[rr] = -(sum_over_g(part) + 0.5f * (float)m.p * fast_log(s2v));
  }
}

// ---- helpers to move rows between HBM and the register layouts ---------------
// raw V rows in the same layout (the encoder's input)
template <int NTL, int R>
__device__ __forceinline__ void load_v_rows(const float *v, long long n, int p, long long row0, int j,
                                            int g, f32x4 (&vreg)[R][NTL]) {
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    long long row = row0 + 16 * rr + j;
    row = row < n ? row : n - 1;
    const float *vr = v + row * (long long)p;
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * t + 4 * g + r;
        vreg[rr][t][r] = (c < p) ? vr[c] : 0.0f;
      }
  }
}

// vreg = (bias of g's last layer, from LDS) - (V row): the last layer accumulates on top of it (g_last_groups)
template <int NTL, int R>
__device__ __forceinline__ void load_v_rows(const float *v, const float *bl, long long n, int p, long long row0, int j,
                                            int g, f32x4 (&vreg)[R][NTL]) {
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    long long row = row0 + 16 * rr + j;
    row = row < n ? row : n - 1;
    const float *vr = v + row * (long long)p;
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * t + 4 * g + r;
        vreg[rr][t][r] = bl[c] - ((c < p) ? vr[c] : 0.0f);
      }
  }
}

// Gram form: 2 u (tiles 0-3, accumulator layout, 16-byte loads) and c (tile 4, lane group 0) of the tile's rows (see g_last_gram)
template <int R>
__device__ __forceinline__ void load_gram_rows(const float *uc, long long n, long long row0, int j, int g, f32x4 (&vreg)[R][5]) {
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    long long row = row0 + 16 * rr + j;
    row = row < n ? row : n - 1;
    const f32x4 *ur = reinterpret_cast<const f32x4 *>(uc + row * 64);
#pragma unroll
    for (int t = 0; t < 4; ++t) vreg[rr][t] = ur[4 * t + g];
    const float c = uc[64 * n + row];
    vreg[rr][4] = f32x4{g == 0 ? c : 0.0f, 0.0f, 0.0f, 0.0f};
  }
}

// z row (q floats) + x -> L1 input tiles (feature 16 t + 4 r + g)
template <int KT1, int R>
__device__ __forceinline__ void load_z_rows(const float *z, long long n, int q, long long row0, int j,
                                            int g, const float (&xr)[R], f32x4 (&zin)[R][KT1]) {
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    long long row = row0 + 16 * rr + j;
    row = row < n ? row : n - 1;
    const float *zr = z + row * (long long)q;
#pragma unroll
    for (int t = 0; t < KT1; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * t + 4 * r + g;
        zin[rr][t][r] = (f < q) ? zr[f] : (f == q ? xr[rr] : 0.0f);
      }
  }
}

template <int KT1, int R>
__device__ __forceinline__ void store_z_rows(float *z, long long n, int q, long long row0, int j, int g,
                                             const f32x4 (&zin)[R][KT1]) {
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
    const long long row = row0 + 16 * rr + j;
    if (row < n) {
      float *zr = z + row * (long long)q;
#pragma unroll
      for (int t = 0; t < KT1; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 16 * t + 4 * r + g;
          if (f < q) zr[f] = zin[rr][t][r];
        }
    }
  }
}


// ---------------------------------------------------------------------------
// Conditional latent prior of IdentifiableCausalBGM (models/causalbgm/identifiable.py:195-211, 541-551):
// Z | U ~ N(mu(U), sigma^2(U) I) with U the one-hot segment of the row, so -log p(z | u) = |z - mu|^2 / (2 sigma^2) + (q/2) log sigma^2
// replaces |z|^2 / 2.  causal_logp keeps the standard-normal term; kernels instantiated with PRIOR = 1 hold the row's
// (mu, 1/sigma^2, (q/2) log sigma^2) in registers and add the difference to every log-posterior they evaluate.
// ---------------------------------------------------------------------------
template <int KT1>
struct PriorRow {
  f32x4 mu[KT1];      // feature 16 t + 4 r + g, as the L1 input tiles
  float is2, lc;
  __device__ __forceinline__ void load(const int *seg, const float *tab, long long row, int q, int g) {
    const float *t = tab + (long long)seg[row] * (q + 2);
#pragma unroll
    for (int tt = 0; tt < KT1; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * tt + 4 * r + g;
        const float val = t[f < q ? f : q + 1];       // unconditional in-bounds load (the row has q + 2 entries), then mask: a load under
                                                      // the select makes hipcc 7.2 fail with its "$src_shared_base" illegal-instruction error
        mu[tt][r] = (f < q) ? val : 0.0f;
      }
    is2 = t[q];
    lc = t[q + 1];
  }
  // log p_cond(z) - log p_std(z) = |z|^2 / 2 - is2 |z - mu|^2 / 2 - lc      (same value in the four lane groups)
  __device__ __forceinline__ float correction(const f32x4 (&z)[KT1], int q, int g) const {
    float part = 0.0f;
#pragma unroll
    for (int tt = 0; tt < KT1; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float zz = z[tt][r], d = zz - mu[tt][r];
        const float term = 0.5f * (zz * zz - is2 * d * d);
        part += (16 * tt + 4 * r + g < q) ? term : 0.0f;
      }
    return sum_over_g(part) - lc;
  }
};

// ---------------------------------------------------------------------------
// get_log_posterior for n rows (one evaluation)
// ---------------------------------------------------------------------------
template <int KT1, int KSL1, int NTL, int R, int WAVES, int PRIOR = 0>
__global__ __launch_bounds__(64 * WAVES) void causal_logpost_kernel(const float *blob, CausalMeta m,
                                                                    const float *x, const float *y,
                                                                    const float *v, const float *z,
                                                                    long long n, float *out, const int *seg = nullptr,
                                                                    const float *prior_tab = nullptr) {
  static_assert(PRIOR == 0 || R == 1, "conditional prior: one row tile per wave");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  lds_fill(lds, blob, m.total);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4, lane_off = 64 * g + j;
  const long long n_tiles = (n + 16 * R - 1) / (16 * R);
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < n_tiles;
       tile += (long long)gridDim.x * WAVES) {
    BGM_NO_HOIST();
    const long long row0 = tile * 16 * R;
    float xr[R], yr[R], lp[R];
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      long long row = row0 + 16 * rr + j;
      row = row < n ? row : n - 1;
      xr[rr] = x[row];
      yr[rr] = y[row];
    }
    f32x4 vreg[R][NTL];
    load_v_rows<NTL, R>(v, lds + m.bgl, n, m.p, row0, j, g, vreg);
    f32x4 zin[R][KT1];
    load_z_rows<KT1, R>(z, n, m.q, row0, j, g, xr, zin);
#ifdef BGM_PROF
    unsigned long long tsec[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
    causal_logp<KT1, KSL1, NTL, R>(lds, m, lane_off, g, j, zin, vreg, xr, yr, lp, tsec, tlast);
#else
    causal_logp<KT1, KSL1, NTL, R>(lds, m, lane_off, g, j, zin, vreg, xr, yr, lp);
#endif
    if constexpr (PRIOR) {
      PriorRow<KT1> pr;
      const long long rowc = (row0 + j < n) ? row0 + j : n - 1;
      pr.load(seg, prior_tab, rowc, m.q, g);
      lp[0] += pr.correction(zin[0], m.q, g);
    }
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const long long row = row0 + 16 * rr + j;
      if (g == 0 && row < n) out[row] = lp[rr];
    }
  }
}

// ---------------------------------------------------------------------------
// infer_from_latent_posterior (base.py:671-763) for the R x 16 states held by one wave:
// f first layer once at x = 0, doses as rank-1 updates, DB doses per pass.
//   EFFECT 1: adrf_slot[d * n_doses + k] += sum over the wave's valid rows of y_k   (draw-major: the doses of a retained draw share one
//             or two cache lines, so the 4-lane atomics of its passes are one L2 line instead of one line per dose)
//   EFFECT 2: ite[row * n_keep + d] = y(x=1) - y(x=0)
// Sampling-blob layout of the two small nets' tails (causal_scale_blob_kernel): the 8 outputs of layer 3 sit at tile positions
// 4 (f >> 1) + (f & 1) -- accumulator registers r = 0, 1 of every lane group -- so layer 4 contracts over two K-steps instead of
// four, and the two output columns of layer 4 (mu, s) are replicated at positions 4 g' + {0, 1}: every lane holds (mu, s) of its
// row in registers 0 / 1 of the output tile.
// Dose-response sums (EFFECT 1, one row tile per wave): a pass evaluates four doses at once (independent MFMA chains sharing the
// A fragments); afterwards lane group g owns dose e = g of the pass: ONE softplus / sqrt / noise FMA, ONE DPP row reduction and
// ONE 4-lane atomic per pass instead of four of each.  Outcome noise of dose k = word (k & 3) of Philox(row, it, k >> 2,
// TAG_YNOISE) (oracle/causal.py).  Sixteen doses at a time, lane group g evaluates Philox call 4c + g ONCE and pass p uses its
// word p for dose 16c + 4g + p, so the noise is consumed by the lane group that produced it (2 instead of 5 Philox evaluations
// per kept draw at 20 doses); a remainder of fewer than four calls is evaluated by all lane groups (call t, dose 4t + g = word g).
// ---------------------------------------------------------------------------
// value of the lane's own group: v[g]
__device__ __forceinline__ float pick_by_group(int g, float v0, float v1, float v2, float v3) {
  return g == 0 ? v0 : (g == 1 ? v1 : (g == 2 ? v2 : v3));
}

// ROWS (EFFECT 1, one row tile per wave, grouped; causal_hmc_rowfx_kernels.h): y stays with its row instead of being summed over the
// tile -- lane (j, g) owns (row j, its dose k of the pass) and keeps the shifted moments of y over the retained draws in
// row_mom [3][n_doses][n] (ref = y of draw 0, s1 += y - ref, s2 += (y - ref)^2; plain loads and stores, one owner per element) and,
// when row_y is given, the value itself in row_y[(row * n_doses + k) * n_keep + d].  adrf_slot / ite are not touched.
// EFFECT 4 (R == 1; causal_hmc_gfx_kernels.h): the ITE of EFFECT 2, line for line up to yk[0] - yk[1], summed by row label instead of
// stored.  `label` is the row's label (the same in the four lanes of a row), n_doses carries n_labels, adrf_slot is the wave's slot
// [n_keep][n_labels]: adrf_slot[d * n_labels + c] += sum over the tile's valid rows with label c, the labels present in the tile taken
// in the order of their lowest row, each by ONE DPP row reduction and ONE addition from lane 15.  ite is not touched.
// TAILS (ROWS only; causal_hmc_tails_kernels.h): the lane also keeps the k_tail smallest and the k_tail largest values of its series
// in row_tails [2][k_tail][n_doses][n] (row_tail_push, row_tails.h).
// CONTRAST (ROWS only; causal_hmc_contrast_kernels.h): besides the curve, the difference to the baseline dose, c = y(x_k) - y(x_0), is
// kept per (row, dose).  Dose 0 of a draw is finished in pass 0 by lane group 0 (own or shared pass alike), so after pass 0 every lane
// reads y0 from the lane of group 0 that holds its row -- one cross-lane read executed by all 64 lanes, outside the valid branch --
// and keeps it in a register over the draw's remaining passes.  c is ONE float32 subtraction of the two rounded values (y is pinned
// first, so it cannot be folded into the fmaf that forms y, and row_mom receives the y it always did); its shifted moments go to
// row_cmom [3][n_doses][n] by the rule of row_mom, and row_y / row_tails record c instead of y.  At dose 0 c is exactly 0.  With
// sample_y the two doses carry their own independent noise words, as the two arms of the binary ITE do.
// CHOICE (ROWS only; causal_hmc_choice_kernels.h): besides the curve, which dose is the row's best at every retained draw.  y is pinned
// as under CONTRAST.  The owner lane of (row, k) counts y > threshold in ch.above [n_doses][n] (when given).  Every lane keeps the pair
// (best, best_k) of sign * y over ITS OWN doses of the draw -- valid rows and k < n_doses only: a padded lane evaluates the last dose
// again and must never win --, -inf and an invalid index to begin with; sign = +-1, so the product is exact.  After the last pass one
// exchange over the four lane groups (xor 16, xor 32; all 64 lanes, outside the valid branch) leaves in every lane of row j the
// row's best value and the LOWEST dose index that attains it: the rule compares k, it does not rest on the order the doses arrive
// in (own passes visit k = 4 (c4 + g) + p4, shared passes k = 4 kb + g).  NaN never wins; a row of NaNs counts nothing.  Lane (j, 0)
// owns column [:, row] of ch.best_count [n_doses][n] and of ch.best_mom [2][n] for the whole run: at draw 0 it zeroes its n_doses
// counters and writes ref = best (the unsigned y) and s1 = 0, afterwards s1 += best - ref, and best_count[best_k][row] += 1 by plain
// load and store.  No atomics, and no access of one lane is ordered against another's.
struct CausalChoiceArgs {
  unsigned *best_count;               // [n_doses][n]
  float *best_mom;                    // [2][n]: ref, s1 of the draw's best y
  unsigned *above;                    // [n_doses][n], or NULL
  float sign, threshold;              // +1 maximise / -1 minimise; y > threshold is counted
};
// ---------------------------------------------------------------------------
// VTAILS: the dose passes of the grouped dose-response sums with the 32 -> 8 -> 2 tail of f on the vector ALU (the MH kernels'
// retained phase).  On the matrix pipe the tail of a pass is 40 of its 168 instructions for 1 088 MACs per chain: half of the M
// rows of 32 -> 8 and fourteen of the sixteen of 8 -> 2 are padding.  Here
//   layer 3: after layer 2 lane (j, g) holds features 16 u + 4 g + r of chain j for the pass's four doses -- 8 of the 32 inputs.  It
//            forms the 8 partial outputs over its own inputs (64 FMAs per dose, weights m.vf3), then two exchange steps with a fixed
//            addition order sum the partials AND hand each dose to its owner: with lane ^ 32 (v_permlane32_swap: lanes 0-31 keep
//            doses 0 / 1, lanes 32-63 doses 2 / 3), then with lane ^ 16 (v_permlane16_swap: lane group g keeps dose g).  Every owner
//            adds ((g0 + g2) + (g1 + g3)), then the bias;
//   layer 4: 8 lrelu_s and 16 FMAs in the owner (weights m.vf4): (mu, s) of its own dose and chain, what the grouped finish wants.
// The tail and the finish of pass kb - 1 are written, K-step by K-step, between the layer-2 MFMAs of pass kb (vt_tail_step<S> after
// K-step S), so they issue in the gaps of this wave's own matrix instructions; the last pass drains after the loop.  Noise words,
// cache entries, reduction over the rows and the atomics are those of causal_effects' GROUPED finish, so causal_effects_cached
// replays a pass bit for bit.  EVAL_ONLY (causal_event_f_kernel) stops at the (mean, sd) pairs: the same instructions up to there, so
// the event form of the retained phase stays bit-identical to the fused kernel it stands in for.
// ---------------------------------------------------------------------------
template <int... S, class F>
__device__ __forceinline__ void vt_static_for(std::integer_sequence<int, S...>, F &&f) { (f(std::integral_constant<int, S>{}), ...); }

struct VtTail {
  float act[4][8];      // lrelu_s of the pass's layer-2 outputs: [dose][local input 4 u + r]
  float p[4][8];        // layer-3 partials [dose][output]; after the exchanges p[0][.] = the owner's sums
  float mu, sr, tot;     // raw outputs of layer 4; the (masked) y of the lane's dose, then its sum over the rows
  int k;                // the dose this lane group owns in the pass
  bool own;             // its noise word comes from the lane group's own Philox call
};

// sum of v0 and v1 across the lane pairs of a swap: the owner of v0's dose (low half / even row) and the owner of v1's
__device__ __forceinline__ float vt_swap32_add(float v0, float v1) {
  const auto s = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v0), __builtin_bit_cast(unsigned, v1), false, false);
  return __builtin_bit_cast(float, (unsigned)s[0]) + __builtin_bit_cast(float, (unsigned)s[1]);
}
__device__ __forceinline__ float vt_swap16_add(float v0, float v1) {
  const auto s = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v0), __builtin_bit_cast(unsigned, v1), false, false);
  return __builtin_bit_cast(float, (unsigned)s[0]) + __builtin_bit_cast(float, (unsigned)s[1]);
}

// Step S (0 .. 15) of the tail + finish of one pass.  Steps 0-10: three (input, dose) groups of 8 layer-3 FMAs each (32 groups);
// 11: exchange with lane ^ 32; 12: exchange with lane ^ 16, bias; 13: layer 4; 14: softplus / sqrt / noise; 15: the row reduction.
template <int S, bool CACHE, bool EVAL_ONLY>
__device__ __forceinline__ void vt_tail_step(VtTail &T, const float *w3v, const float *w4v, int lane, int pass, float sig2_y, int sample_y,
                                             bool valid, int nd, f32x4 &nz, int g, float2 *cache) {
  if constexpr (S <= 10) {
#pragma unroll
    for (int grp = 3 * S; grp < (3 * S + 3 < 32 ? 3 * S + 3 : 32); ++grp) {
      const int l = grp >> 2, e = grp & 3;
      const f32x4 wa = *reinterpret_cast<const f32x4 *>(w3v + 8 * l), wb = *reinterpret_cast<const f32x4 *>(w3v + 8 * l + 4);
      const float a = T.act[e][l];
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const float w = o < 4 ? wa[o & 3] : wb[o & 3];
        T.p[e][o] = l == 0 ? w * a : fmaf(w, a, T.p[e][o]);
      }
    }
  } else if constexpr (S == 11) {
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      T.p[0][o] = vt_swap32_add(T.p[0][o], T.p[2][o]);
      T.p[1][o] = vt_swap32_add(T.p[1][o], T.p[3][o]);
    }
  } else if constexpr (S == 12) {
    const f32x4 ba = *reinterpret_cast<const f32x4 *>(w4v + 16), bb = *reinterpret_cast<const f32x4 *>(w4v + 20);
#pragma unroll
    for (int o = 0; o < 8; ++o) T.p[0][o] = vt_swap16_add(T.p[0][o], T.p[1][o]) + (o < 4 ? ba[o & 3] : bb[o & 3]);
  } else if constexpr (S == 13) {
    const f32x4 b4 = *reinterpret_cast<const f32x4 *>(w4v + 24);
    float mu = b4[0], sr = b4[1];
#pragma unroll
    for (int o4 = 0; o4 < 4; ++o4) {
      const f32x4 w = *reinterpret_cast<const f32x4 *>(w4v + 4 * o4);      // rows 2 o4, 2 o4 + 1 of [8][2]
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float a = lrelu_s(T.p[0][2 * o4 + h]);
        mu = fmaf(w[2 * h], a, mu);
        sr = fmaf(w[2 * h + 1], a, sr);
      }
    }
    T.mu = mu; T.sr = sr;
  } else if constexpr (S == 14) {
    const float s2 = (sig2_y > 0.0f) ? sig2_y : softplus_f(T.sr) + BGM_EPS;
    const float sd_m = __builtin_sqrtf(s2);
    if constexpr (CACHE) cache[pass * 64 + lane] = make_float2(T.mu, sd_m);        // for causal_effects_cached
    if constexpr (EVAL_ONLY) return;                                               // (causal_event_f_kernel: the pairs are all that is wanted)
    const float noise = T.own ? nz[0] : pick_by_group(g, nz[0], nz[1], nz[2], nz[3]);
    if (T.own) nz = f32x4{nz[1], nz[2], nz[3], nz[0]};
    const float y = sample_y ? fmaf(sd_m, noise, T.mu) : T.mu;
    T.tot = (valid && T.k < nd) ? y : 0.0f;
  } else if constexpr (!EVAL_ONLY) {
    T.tot = sum_over_j_to_lane15(T.tot);
  }
}

// layer 2 of one pass (64 -> 32 at the doses xk, first-layer activations formed at their K-step as in causal_effects); fill(S) is
// written after the MFMAs of K-step S
template <class F>
__device__ __forceinline__ void vt_layer2(const float *lds, const CausalMeta &m, int lane_off, int g, const f32x4 (&base)[4],
                                          const f32x4 (&wx)[4], const float (&xk)[4], f32x4 (&a2)[4][2], F &&fill) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const f32x4 b = *reinterpret_cast<const f32x4 *>(lds + m.bf2 + 16 * u + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) a2[e][u] = b;
  }
  const float *w2 = lds + m.wf2 + lane_off * 2;
  vt_static_for(std::make_integer_sequence<int, 16>{}, [&](auto S) {
    constexpr int s = decltype(S)::value, t = s >> 2, r = s & 3;
    AFrag<2> af;
    af.load(w2 + (16 * t + r) * 16 * 2);
    float bop[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bop[e] = lrelu_s_pinned(fmaf(wx[t][r], xk[e], base[t][r]));
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) a2[e][u] = BGM_MFMA(af.get(u), bop[e], a2[e][u]);
    fill(S);
  });
}

template <bool CACHE, bool EVAL_ONLY>
__device__ __forceinline__ void causal_dose_passes_valu(const float *lds, const CausalMeta &m, int lane_off, int g, int j, int lane,
                                                        const f32x4 (&base)[4], const f32x4 (&wx)[4], unsigned rowid, bool valid,
                                                        unsigned it, long long d, int sample_y, int nd, const float *x_values,
                                                        float *adrf_slot, unsigned k0, unsigned k1, float2 *cache) {
  const int n_calls = (nd + 3) >> 2, n_own = n_calls & ~3;
  if (n_calls == 0) return;
  const float *w3v = lds + m.vf3 + 64 * g, *w4v = lds + m.vf4;
  f32x4 nz = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 a2[4][2];
  VtTail T;
  auto doses = [&](int kb, float (&xk)[4]) {
    const bool own = kb < n_own;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = own ? 4 * ((kb & ~3) + e) + (kb & 3) : 4 * kb + e;
      xk[e] = x_values[k < nd ? k : nd - 1];
    }
  };
  // outcome noise of pass kb: its lane group's own call (renewed every fourth pass), or the call shared by the remainder passes
  auto noise = [&](int kb) {
    const bool own = kb < n_own;
    if (!EVAL_ONLY && sample_y && (!own || (kb & 3) == 0)) nz = box_muller4(philox4x32_10(rowid, it, (unsigned)(own ? (kb & ~3) + g : kb), TAG_YNOISE, k0, k1));
  };
  auto open_tail = [&](int pass) {       // the pass whose layer 2 is in a2
    T.own = pass < n_own;
    T.k = T.own ? 4 * ((pass & ~3) + g) + (pass & 3) : 4 * pass + g;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int l = 0; l < 8; ++l) T.act[e][l] = lrelu_s(a2[e][l >> 2][l & 3]);
  };
  auto emit = [&]() {
    if constexpr (EVAL_ONLY) return;
    if (j == 15 && T.k < nd) unsafeAtomicAdd(adrf_slot + (long long)d * nd + T.k, T.tot);
  };
  {
    float xk[4];
    doses(0, xk);
    vt_layer2(lds, m, lane_off, g, base, wx, xk, a2, [](auto) {});
    noise(0);
  }
  for (int kb = 1; kb < n_calls; ++kb) {
    BGM_NO_HOIST();
    float xk[4];
    doses(kb, xk);
    open_tail(kb - 1);
    vt_layer2(lds, m, lane_off, g, base, wx, xk, a2, [&](auto S) {
      vt_tail_step<decltype(S)::value, CACHE, EVAL_ONLY>(T, w3v, w4v, lane, kb - 1, m.sig2_y, sample_y, valid, nd, nz, g, cache);
    });
    emit();
    noise(kb);
  }
  BGM_NO_HOIST();
  open_tail(n_calls - 1);
  vt_static_for(std::make_integer_sequence<int, 16>{}, [&](auto S) {
    vt_tail_step<decltype(S)::value, CACHE, EVAL_ONLY>(T, w3v, w4v, lane, n_calls - 1, m.sig2_y, sample_y, valid, nd, nz, g, cache);
  });
  emit();
}

template <int KT1, int KSL1, int R, int EFFECT, bool GROUPING = true, bool CACHE = false, bool EVAL_ONLY = false, bool L1MASK = true,
          bool ROWS = false, bool TAILS = false, bool VTAILS = false, bool CONTRAST = false, bool CHOICE = false>
__device__ __forceinline__ void causal_effects(const float *lds, const CausalMeta &m, int lane_off, int g, int j,
                                               int lane, const f32x4 (&zs)[R][KT1], const unsigned (&rowid)[R],
                                               const bool (&valid)[R], long long row0, long long n, unsigned it,
                                               long long d, int n_keep, int sample_y, int n_doses,
                                               const float *x_values, float *adrf_slot, float *ite, unsigned k0,
                                               unsigned k1, float2 *cache = nullptr, float *ite_c = nullptr,
                                               float *row_mom = nullptr, float *row_y = nullptr, int label = 0,
                                               float *row_tails = nullptr, int k_tail = 0, float *row_cmom = nullptr,
                                               const CausalChoiceArgs &ch = CausalChoiceArgs{}) {
  // ite_c (EFFECT == 2, one row tile per wave, CACHE): [4] registers of the caller receiving (mean, sd) of the two arms
  static_assert(!ROWS || (EFFECT == 1 && R == 1 && GROUPING && !CACHE && !EVAL_ONLY), "ROWS: the grouped finish of the dose-response sums");
  static_assert(EFFECT != 4 || (R == 1 && !CACHE && !EVAL_ONLY && !ROWS), "EFFECT 4: the label sums of one row tile per wave");
  static_assert(!TAILS || ROWS, "TAILS: the tail buffers of the per-row dose-response");
  static_assert(!CONTRAST || ROWS, "CONTRAST: the contrasts of the per-row dose-response against its dose 0");
  static_assert(!CHOICE || (ROWS && !TAILS && !CONTRAST), "CHOICE: the best dose of the per-row dose-response; no twin with TAILS or CONTRAST");
  constexpr bool ARMS = (EFFECT == 2 || EFFECT == 4);   // the two arms x = 1, x = 0 of a binary treatment
  BGM_NO_HOIST();
  f32x4 z0in[R][KT1];
#pragma unroll
  for (int rr = 0; rr < R; ++rr)
#pragma unroll
    for (int t = 0; t < KT1; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) z0in[rr][t][r] = (16 * t + 4 * r + g == m.q) ? 0.0f : zs[rr][t][r];
  f32x4 base[R][4];
  if constexpr (L1MASK) dense_masked<KT1, KSL1, 4, R>(lds + m.w1f, lds + m.b1f, lane_off, g, z0in, base, m.l1b);   // x is zeroed: the treatment column's K-step too
  else dense<KT1, KSL1, 4, R>(lds + m.w1f, lds + m.b1f, lane_off, g, z0in, base);
  f32x4 wx[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) wx[t] = *reinterpret_cast<const f32x4 *>(lds + m.wxf + 16 * t + 4 * g);
  const int nd = ARMS ? (CACHE && n_doses == 0 ? 0 : 2) : n_doses;     // (CACHE: n_doses = 0 switches the evaluation off)
  constexpr int DB = ARMS ? 2 : 4;  // doses evaluated per pass (independent MFMA chains)
  constexpr bool GROUPED = (EFFECT == 1 && R == 1 && GROUPING);   // lane group g finishes dose e = g of a pass (see above)
  if constexpr (VTAILS) {     // the same passes with f's tail on the vector ALU, one pass behind layer 2 (above)
    static_assert(GROUPED && !ROWS && (CACHE || !EVAL_ONLY), "VTAILS: the grouped dose-response sums of the MH kernels and of their event form");
    causal_dose_passes_valu<CACHE, EVAL_ONLY>(lds, m, lane_off, g, j, lane, base[0], wx, rowid[0], valid[0], it, d, sample_y, nd, x_values, adrf_slot,
                                   k0, k1, cache);
    return;
  }
  const int n_calls = (nd + 3) >> 2, n_own = GROUPED ? (n_calls & ~3) : 0;   // Philox calls [0, n_own) in groups of four
  f32x4 nz[R];
#pragma unroll
  for (int rr = 0; rr < R; ++rr) nz[rr] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  [[maybe_unused]] float y0 = 0.0f;            // (CONTRAST: y of the lane's row at dose 0 of this draw, from pass 0 on)
  [[maybe_unused]] float best = -__builtin_inff();     // (CHOICE: the largest sign * y among the lane's own doses of this draw ...
  [[maybe_unused]] int best_k = 0x7fffffff;            //  ... and the lowest dose index attaining it)
  for (int kb = 0; kb < n_calls; ++kb) {       // one pass of DB doses per Philox call
    BGM_NO_HOIST();
    const bool own = kb < n_own;
    const int c4 = kb & ~3, p4 = kb & 3;
    if (!EVAL_ONLY && sample_y && (!own || p4 == 0)) {
#pragma unroll
      for (int rr = 0; rr < R; ++rr) nz[rr] = box_muller4(philox4x32_10(rowid[rr], it, (unsigned)(own ? c4 + g : kb), TAG_YNOISE, k0, k1));
    }
    float xk[DB];
#pragma unroll
    for (int e = 0; e < DB; ++e) {
      const int k = own ? 4 * (c4 + e) + p4 : 4 * kb + e;
      xk[e] = ARMS ? (e == 0 ? 1.0f : 0.0f) : x_values[k < nd ? k : nd - 1];
    }
    float mu[DB * R], sr[DB * R];
#ifndef BGM_NO_JIT_EFFECTS
    if constexpr (R == 1) {
      // The dose-specific first-layer activations a1[e] = lrelu_s(base + wx * x_e) are never materialised: element
      // (t, r) is the B operand of K-step 4t + r of the second layer, so it is computed right there, between the
      // MFMAs of the same wave (the two waves of a SIMD share its VALU issue slots as well as its matrix pipe: a
      // separate 768-instruction VALU block per 4 doses cost its full issue time, VALU placed inside the MFMA stream
      // of the same wave is covered by it).  Same for the LeakyReLU feeding layers 3 and 4.
      f32x4 a2[DB][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(lds + m.bf2 + 16 * u + 4 * g);
#pragma unroll
        for (int e = 0; e < DB; ++e) a2[e][u] = b;
      }
      const float *w2 = lds + m.wf2 + lane_off * 2;
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int t = s >> 2, r = s & 3;
        AFrag<2> af;
        af.load(w2 + (16 * t + r) * 16 * 2);
        float bop[DB];
#pragma unroll
        for (int e = 0; e < DB; ++e) bop[e] = lrelu_s_pinned(fmaf(wx[t][r], xk[e], base[0][t][r]));
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int e = 0; e < DB; ++e) a2[e][u] = BGM_MFMA(af.get(u), bop[e], a2[e][u]);
        // (Forcing MFMA, VALU, VALU, MFMA ... with sched_group_barrier -- with or without software-pipelining the
        // next step's operands and fragment -- produced the intended instruction stream and was 2-3 % SLOWER than
        // leaving the placement to the compiler: measured 5.30-5.36 s vs 5.18 s for the keep phase.)
      }
      f32x4 a3[DB];
      {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(lds + m.bf3 + 4 * g);
#pragma unroll
        for (int e = 0; e < DB; ++e) a3[e] = b;
      }
      const float *w3 = lds + m.wf3 + lane_off;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int t = s >> 2, r = s & 3;
        const float af = w3[(16 * t + r) * 16];
#pragma unroll
        for (int e = 0; e < DB; ++e) a3[e] = BGM_MFMA(af, lrelu_s(a2[e][t][r]), a3[e]);
      }
      f32x4 a4[DB];
      {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(lds + m.bf4 + 4 * g);
#pragma unroll
        for (int e = 0; e < DB; ++e) a4[e] = b;
      }
      const float *w4 = lds + m.wf4 + lane_off;
#pragma unroll
      for (int s = 0; s < 2; ++s) {        // the 8 inputs occupy K-steps 0 and 1 (permuted layer-3 outputs)
        const float af = w4[s * 16];
#pragma unroll
        for (int e = 0; e < DB; ++e) a4[e] = BGM_MFMA(af, lrelu_s(a3[e][s]), a4[e]);
      }
#pragma unroll
      for (int e = 0; e < DB; ++e) { mu[e] = a4[e][0]; sr[e] = a4[e][1]; }
    } else
#endif
    {
      f32x4 a1[DB * R][4];
#pragma unroll
      for (int e = 0; e < DB; ++e)
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) a1[e * R + rr][t][r] = lrelu_s(fmaf(wx[t][r], xk[e], base[rr][t][r]));
      fh_tail<DB * R>(lds, m.wf2, m.bf2, m.wf3, m.bf3, m.wf4, m.bf4, lane_off, g, a1, mu, sr);
    }
    if constexpr (GROUPED) {
      const int k = own ? 4 * (c4 + g) + p4 : 4 * kb + g;          // this lane group's dose of the pass ...
      const float mu_m = pick_by_group(g, mu[0], mu[1], mu[2], mu[3]), sr_m = pick_by_group(g, sr[0], sr[1], sr[2], sr[3]);
      const float s2 = (m.sig2_y > 0.0f) ? m.sig2_y : softplus_f(sr_m) + BGM_EPS;
      const float sd_m = __builtin_sqrtf(s2);
      if constexpr (CACHE) cache[kb * 64 + lane] = make_float2(mu_m, sd_m);        // for causal_effects_cached below
      if constexpr (EVAL_ONLY) continue;                                             // (causal_event_f_kernel: the pairs are all that is wanted)
      // ... and its noise word: word p4 of its own call (rotated into word 0 pass by pass), or word g of the shared call
      const float noise = own ? nz[0][0] : pick_by_group(g, nz[0][0], nz[0][1], nz[0][2], nz[0][3]);
      if (own) nz[0] = f32x4{nz[0][1], nz[0][2], nz[0][3], nz[0][0]};
      float y = sample_y ? fmaf(sd_m, noise, mu_m) : mu_m;
      if constexpr (ROWS) {
        [[maybe_unused]] float c = 0.0f;
        if constexpr (CONTRAST) {
          asm volatile("" : "+v"(y));                 // the rounded y, as the curve planes receive it
          if (kb == 0) y0 = __shfl(y, j);             // (wave-uniform) lane j = (row j, lane group 0) holds dose 0: all 64 lanes read
          c = y - y0;
        }
        const float rec = CONTRAST ? c : y;           // what the draws and the tails record
        if constexpr (CHOICE) {
          asm volatile("" : "+v"(y));                 // the rounded y, as the curve planes and row_y receive it
          const float sy = ch.sign * y;               // exact
          if (valid[0] && k < nd && (sy > best || (sy == best && k < best_k))) { best = sy; best_k = k; }
        }
        if (valid[0] && k < nd) {
          const long long row = row0 + j, plane = (long long)nd * n;
          long long off = (long long)k * n + row;
          asm volatile("" : "+v"(off));
          float *rf = row_mom + off;
          if (d == 0) {
            rf[0] = y; rf[plane] = 0.0f; rf[2 * plane] = 0.0f;
          } else {
            const float dv = y - rf[0];
            rf[plane] += dv;
            rf[2 * plane] = fmaf(dv, dv, rf[2 * plane]);
          }
          if constexpr (CONTRAST) {
            float *cf = row_cmom + off;
            if (d == 0) {
              cf[0] = c; cf[plane] = 0.0f; cf[2 * plane] = 0.0f;
            } else {
              const float dv = c - cf[0];
              cf[plane] += dv;
              cf[2 * plane] = fmaf(dv, dv, cf[2 * plane]);
            }
          }
          if constexpr (CHOICE) if (ch.above) {       // (wave-uniform)
            unsigned *ab = ch.above + off;
            const unsigned hit = y > ch.threshold ? 1u : 0u;
            if (d == 0) ab[0] = hit;
            else ab[0] += hit;
          }
          if (row_y) row_y[(row * nd + k) * (long long)n_keep + d] = rec;
          if constexpr (TAILS) {
            const long long series = plane;          // floats between two slots of a series: [2][k_tail][n_doses][n]
            float *t0 = row_tails + off;
            row_tail_push<true>(t0, series, k_tail, d, rec);
            row_tail_push<false>(t0 + (long long)k_tail * series, series, k_tail, d, rec);
          }
        }
        continue;
      }
      y = (valid[0] && k < nd) ? y : 0.0f;
      const float tot = sum_over_j_to_lane15(y);
      if (j == 15 && k < nd) unsafeAtomicAdd(adrf_slot + (long long)d * nd + k, tot);
      continue;
    }
    float yk[DB][R];
#pragma unroll
    for (int e = 0; e < DB; ++e)
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        const float s2 = (m.sig2_y > 0.0f) ? m.sig2_y : softplus_f(sr[e * R + rr]) + BGM_EPS;
        const float sd = __builtin_sqrtf(s2);
        if constexpr (CACHE && EFFECT == 2 && R == 1) { ite_c[2 * e] = mu[e * R + rr]; ite_c[2 * e + 1] = sd; }
        yk[e][rr] = sample_y ? fmaf(sd, nz[rr][e], mu[e * R + rr]) : mu[e * R + rr];
      }
    if constexpr (EVAL_ONLY) continue;             // (causal_event_f_ite_kernel: the two arms' (mean, sd) in ite_c are all that is wanted)
    if constexpr (EFFECT == 1) {
#pragma unroll
      for (int e = 0; e < DB; ++e) {
        float tot = 0.0f;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) tot += valid[rr] ? yk[e][rr] : 0.0f;
        tot = sum_over_j_to_lane15(tot);  // values are valid in lane group 0 -> lane 15
        const int k = 4 * kb + e;
        if (lane == 15 && k < nd) unsafeAtomicAdd(adrf_slot + (long long)d * nd + k, tot);
      }
    } else if constexpr (EFFECT == 4) {
      const float v = valid[0] ? yk[0][0] - yk[1][0] : 0.0f;     // (a padding lane carries the clamped row's label and adds nothing)
      unsigned rest = (unsigned)__ballot(valid[0] && g == 0);    // the tile's rows (lanes 0 .. 15) whose label has not been summed yet
      while (rest) {
        const int c = __builtin_amdgcn_readlane(label, __builtin_ctz(rest));     // the label of the lowest remaining row
        const bool mine = label == c;
        const float tot = sum_over_j_to_lane15(mine ? v : 0.0f);
        if (lane == 15 && (unsigned)c < (unsigned)n_doses) unsafeAtomicAdd(adrf_slot + (long long)d * n_doses + c, tot);
        rest &= ~(unsigned)__ballot(mine);
      }
    } else {
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        const long long row = row0 + 16 * rr + j;
        if (g == 0 && row < n) ite[row * (long long)n_keep + d] = yk[0][rr] - yk[1][rr];
      }
    }
  }
  if constexpr (CHOICE) {                        // after the draw's last pass: the row's best over the four lane groups
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {        // all 64 lanes
      const float ob = __shfl_xor(best, sh);
      const int ok = __shfl_xor(best_k, sh);
      const bool take = (ob > best) | ((ob == best) & (ok < best_k));
      best = take ? ob : best;
      best_k = take ? ok : best_k;
    }
    // Lane (j, 0) is the one owner of column [:, row] of both planes.  The tile's first row is the same in all lanes: taken as a scalar,
    // every address below is a scalar base plus the lane's 4 j bytes, so the block needs no 64-bit address per lane (registers: DESIGN 4ai).
    const long long r0 = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(row0 >> 32)) << 32) |
                                     (unsigned)__builtin_amdgcn_readfirstlane((int)row0));
    unsigned jb = 4u * (unsigned)j;
    asm volatile("" : "+v"(jb));                   // formed here, not hoisted to the kernel's entry and held as three 64-bit addresses
    const bool owner = valid[0] && g == 0;
    const float bv = ch.sign * best;               // the unsigned y again (exact)
    float *bm_ref = reinterpret_cast<float *>(reinterpret_cast<char *>(ch.best_mom + r0) + jb);
    float *bm_s1 = reinterpret_cast<float *>(reinterpret_cast<char *>(ch.best_mom + r0 + n) + jb);
    if (d == 0) {                                  // (wave-uniform) the first retained draw writes every element, zeros included
#pragma nounroll
      for (int kk = 0; kk < nd; ++kk)
        if (owner) *reinterpret_cast<unsigned *>(reinterpret_cast<char *>(ch.best_count + r0 + (long long)kk * n) + jb) = 0u;
      if (owner) { *bm_ref = bv; *bm_s1 = 0.0f; }
    }
    const bool counts = owner && best_k < nd;      // (a row whose values were all NaN counts nothing)
    if (counts && d != 0) *bm_s1 += bv - *bm_ref;
    // (owners have g == 0, lanes 0 .. 15: the low word of the ballot holds them all)
    unsigned rest = (unsigned)__ballot(counts);    // the tile's rows whose best dose has not been counted yet
    while (rest) {                                 // one trip per distinct best dose of the tile: its plane's base is a scalar
      const int kq = __builtin_amdgcn_readlane(best_k, __builtin_ctz(rest));
      const bool mine = counts && best_k == kq;
      if (mine) *reinterpret_cast<unsigned *>(reinterpret_cast<char *>(ch.best_count + r0 + (long long)kq * n) + jb) += 1u;
      rest &= ~(unsigned)__ballot(mine);
    }
  }
}

// The ADRF contribution of a retained iteration in which none of the wave's 16 chains moved.  The outcome net is a deterministic
// function of the chain state, so (mean, sd) of every dose are those of the previous retained iteration -- causal_effects left them in
// `cache` ([pass][lane]: the dose this lane group finishes in that pass) -- and only the outcome noise is new: same Philox calls, same
// fma, same reduction order as the GROUPED path of causal_effects, i.e. bit-identical sums without the 20 dose evaluations.  (With the
// reference's q_sd = 1 a trained model accepts 2-10 % of its proposals: 27-80 % of the tiles see no move in an iteration.)
__device__ __forceinline__ void causal_effects_cached(int g, int j, int lane, unsigned rowid, bool valid, unsigned it, long long d,
                                                      int sample_y, int n_doses, float *adrf_slot, unsigned k0, unsigned k1,
                                                      const float2 *cache) {
  const int nd = n_doses;
  const int n_calls = (nd + 3) >> 2, n_own = n_calls & ~3;
  f32x4 nz = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float2 c = cache[lane];
  for (int kb = 0; kb < n_calls; ++kb) {
    const float2 cn = cache[(kb + 1 < n_calls ? kb + 1 : kb) * 64 + lane];     // next pass's pair under this pass's Philox call
    const bool own = kb < n_own;
    const int c4 = kb & ~3, p4 = kb & 3;
    if (sample_y && (!own || p4 == 0)) nz = box_muller4(philox4x32_10(rowid, it, (unsigned)(own ? c4 + g : kb), TAG_YNOISE, k0, k1));
    const int k = own ? 4 * (c4 + g) + p4 : 4 * kb + g;
    const float noise = own ? nz[0] : pick_by_group(g, nz[0], nz[1], nz[2], nz[3]);
    if (own) nz = f32x4{nz[1], nz[2], nz[3], nz[0]};
    float y = sample_y ? fmaf(c.y, noise, c.x) : c.x;
    y = (valid && k < nd) ? y : 0.0f;
    const float tot = sum_over_j_to_lane15(y);
    if (j == 15 && k < nd) unsafeAtomicAdd(adrf_slot + (long long)d * nd + k, tot);
    c = cn;
  }
}

// The same for the individual treatment effects of a binary treatment (EFFECT == 2): y(1) - y(0) of a retained iteration in which no
// chain of the wave moved, from the (mean, sd) of the two arms kept in registers; the ungrouped noise plan of causal_effects (one
// Philox call, word e for arm e).
__device__ __forceinline__ void causal_ite_cached(int g, int j, unsigned rowid, long long row, long long n, unsigned it, long long d,
                                                  int n_keep, int sample_y, float *ite, unsigned k0, unsigned k1, const float (&c)[4]) {
  f32x4 nz = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  if (sample_y) nz = box_muller4(philox4x32_10(rowid, it, 0u, TAG_YNOISE, k0, k1));
  const float y1 = sample_y ? fmaf(c[1], nz[0], c[0]) : c[0];
  const float y0 = sample_y ? fmaf(c[3], nz[1], c[2]) : c[2];
  if (g == 0 && row < n) ite[row * (long long)n_keep + d] = y1 - y0;
}

// Event form of the retained phase (causal_event_kernels.h): the chains of a wave whose flag `ev` is set append (chain, iteration,
// state) to the wave slot's region, in lane order; ev_cnt is the slot's running event count (wave-uniform).
template <int KT1>
__device__ __forceinline__ void causal_event_append(const CausalMhKArgs &a, int q, long long slot, int &ev_cnt, bool ev, int g, int j,
                                                    const f32x4 (&z)[KT1], int it) {
  const unsigned m16 = (unsigned)(__ballot(ev && g == 0) & 0xFFFFull);
  if (m16 == 0u) return;
  if (ev) {
    const long long e = slot * a.ev_cap + ev_cnt + __popc(m16 & ((1u << j) - 1u));
    float *ez = a.ev_z + e * (long long)q;
#pragma unroll
    for (int t = 0; t < KT1; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * t + 4 * r + g;
        if (f < q) ez[f] = z[t][r];
      }
    if (g == 0) a.ev_meta[e] = ((unsigned)(it - a.it_begin) << 4) | (unsigned)j;
  }
  ev_cnt += __popc(m16);
}

// ---------------------------------------------------------------------------
// Persistent random-walk Metropolis-Hastings over a segment of iterations.
// ---------------------------------------------------------------------------
// GRAM: g's Gaussian term in the Gram form (g_last_gram; a.blob / a.m are the Gram copy of the sampling blob, a.uc the rows' 2 u, c)
// ROWADAPT: every chain proposes with a scale of its own (a.row_scale), multiplied after each of the first a.ra_n accept decisions by a
// host-made factor -- a.ra_up[it] if the chain moved, a.ra_dn[it] if not -- and clamped: ONE fp32 multiply, no exp, so float32 on the
// host reproduces the scale bit for bit.  A scale depends on (seed, global row, the row's data) only.  It lives in one register per
// chain (sc[rr], replicated over the four lane groups like lp), loaded from a.row_scale at tile start (a.q_sd when a.init) and stored
// back beside state / logp at tile end; the factor is ONE per-lane load of (accepted ? a.ra_up : a.ra_dn)[it] after the decision (the
// lanes of a chain read the same word).  No LDS is used for it.  The variants that were compiled and rejected -- the scale in LDS, both
// factors by wave-uniform loads ahead of the networks -- and the register figures are in DESIGN.md section 4m.  Compile-time, so that
// the fixed-scale instantiations keep their bits.
// VTAILS (EFFECT 1, one row tile per wave): the retained phase's dose passes run f's 32 -> 8 -> 2 tail on the vector ALU
// (causal_dose_passes_valu); the transition, and with it every chain, is the same code either way.
template <int KT1, int KSL1, int NTL, int R, int WAVES, int EFFECT, int PRIOR = 0, bool GRAM = false, bool ROWADAPT = false, bool VTAILS = false>
__global__ __launch_bounds__(64 * WAVES) void causal_mh_kernel(CausalMhKArgs a) {
  static_assert(PRIOR == 0 || R == 1, "conditional prior: one row tile per wave");
  static_assert(!VTAILS || (EFFECT == 1 && R == 1), "VTAILS: the grouped dose-response sums");
  constexpr bool L1M = causal_l1_masked(KT1, PRIOR);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CausalMeta &m = a.m;
  lds_fill(lds, a.blob, m.total);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4, lane_off = 64 * g + j;
  const long long n = a.n;
  const long long n_tiles = (n + 16 * R - 1) / (16 * R);
  const long long slot = (long long)blockIdx.x * WAVES + wave;
  const long long n_slots = (long long)gridDim.x * WAVES;
  const unsigned long long clk_c0 = __builtin_readcyclecounter(), clk_r0 = __builtin_amdgcn_s_memrealtime();
#ifdef BGM_PROF
  unsigned long long tsec[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
#endif
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  // [WAVES] progress counters after the blob.  An LDS-typed pointer: as a generic one its volatile accesses stay FLAT, and the
  // "{offset, src_shared_base} != null" test that comes with them is what hipcc 7.2 intermittently fails to encode ("$src_shared_base"
  // illegal instruction) when unrelated code in the kernel changes
  volatile __attribute__((address_space(3))) int *prog =
      (volatile __attribute__((address_space(3))) int *)((__attribute__((address_space(3))) float *)lds + m.total);
  if (lane == 0) prog[wave_u] = 0;
  int tiles_done = 0;
  [[maybe_unused]] int ev_cnt = 0;          // EFFECT == 3: events this wave slot has appended

  for (long long tile = slot; tile < n_tiles; tile += n_slots) {
    const long long row0 = tile * 16 * R;
    float xr[R], yr[R], lp[R];
    unsigned rowid[R];
    bool valid[R];
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      long long row = row0 + 16 * rr + j;
      valid[rr] = row < n;
      row = row < n ? row : n - 1;
      xr[rr] = a.x[row];
      yr[rr] = a.y[row];
      rowid[rr] = (unsigned)(a.row_base + row);
    }
    f32x4 vreg[R][GRAM ? 5 : NTL];
    if constexpr (GRAM) load_gram_rows<R>(a.uc, n, row0, j, g, vreg);
    else load_v_rows<NTL, R>(a.v, lds + m.bgl, n, m.p, row0, j, g, vreg);
    PriorRow<KT1> pr;
    if constexpr (PRIOR) pr.load(a.seg, a.prior_tab, (row0 + j < n) ? row0 + j : n - 1, m.q, g);
    f32x4 zs[R][KT1];
    if (a.init) {
      // current_state ~ N(0,1)  (base.py:842), RNG spec tag 0
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
#pragma unroll
        for (int t = 0; t < KT1; ++t) {
          const f32x4 e = box_muller4(philox4x32_10(rowid[rr], 0u, (unsigned)(g + 4 * t), TAG_INIT, a.k0, a.k1));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int f = 16 * t + 4 * r + g;
            zs[rr][t][r] = (f < m.q) ? e[r] : (f == m.q ? xr[rr] : 0.0f);
          }
        }
#ifdef BGM_PROF
      { unsigned long long tsec0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast0 = 0;
        causal_logp<KT1, KSL1, NTL, R, GRAM, L1M>(lds, m, lane_off, g, j, zs, vreg, xr, yr, lp, tsec0, tlast0); }
#else
      causal_logp<KT1, KSL1, NTL, R, GRAM, L1M>(lds, m, lane_off, g, j, zs, vreg, xr, yr, lp);
#endif
      if constexpr (PRIOR) lp[0] += pr.correction(zs[0], m.q, g);
    } else {
      load_z_rows<KT1, R>(a.state, n, m.q, row0, j, g, xr, zs);
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        long long row = row0 + 16 * rr + j;
        row = row < n ? row : n - 1;
        lp[rr] = a.logp[row];
      }
    }

    [[maybe_unused]] float sc[R];        // ROWADAPT: the chains' proposal scales
    if constexpr (ROWADAPT) {
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        long long row = row0 + 16 * rr + j;
        row = row < n ? row : n - 1;
        const float s_in = a.row_scale[row];       // (unconditional in-bounds load, then select: see PriorRow::load)
        sc[rr] = a.init ? a.q_sd : s_in;
      }
    }

    uint4 uacc[R];
    [[maybe_unused]] const int ev_tile0 = ev_cnt;
    bool eff_cached = false;      // the slot's cache holds the outcome-net values of the tile's current states
    unsigned n_eff_skipped = 0u;
    float ite_c[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // EFFECT == 2: (mean, sd) of the two arms at the tile's current states
#ifdef BGM_PROF
    tlast = __builtin_readcyclecounter();
#endif
    for (int it = a.it_begin; it < a.it_begin + a.n_iters; ++it) {
      BGM_NO_HOIST();
      PMARK(7);
      // The two waves that share a SIMD (w, w+4) are arbitrated oldest-first: left alone the older one
      // runs ahead, finishes ~30 % early and leaves the younger wave by itself on the SIMD at low MFMA
      // utilisation (measured: waves 0-3 done at 45 ms, waves 4-7 at 63 ms).  Each wave publishes its
      // progress in LDS and raises its priority only while it is behind its partner.
      // The two waves that share a SIMD (w, w+4) are arbitrated oldest-first: left alone the older one runs
      // ahead, finishes ~30 % early and leaves the younger wave by itself on the SIMD (measured: waves 0-3 done
      // at 45 ms, waves 4-7 at 63 ms).  Each wave publishes its progress in LDS and raises its priority only
      // while it is behind its partner.
      if constexpr (WAVES == 8) {
        const int mine = tiles_done * a.n_iters + (it - a.it_begin);
        if (lane == 0) prog[wave_u] = mine;
        const int other = __builtin_amdgcn_readfirstlane(prog[wave_u ^ 4]);
        if (mine < other) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
      }
      // ---- proposal  z' = z + q_sd * eps   (base.py:862)
      f32x4 zp[R][KT1];
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
#pragma unroll
        for (int t = 0; t < KT1; ++t) {
          float qs;
          if constexpr (ROWADAPT) qs = sc[rr]; else qs = a.q_sd;
          const f32x4 e = box_muller4(philox4x32_10(rowid[rr], (unsigned)it, (unsigned)(g + 4 * t), TAG_PROP, a.k0, a.k1));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int f = 16 * t + 4 * r + g;
            zp[rr][t][r] = (f < m.q) ? fmaf(qs, e[r], zs[rr][t][r]) : zs[rr][t][r];
          }
        }
      float lpp[R];
      PMARK(0);
#ifdef BGM_PROF
      causal_logp<KT1, KSL1, NTL, R, GRAM, L1M>(lds, m, lane_off, g, j, zp, vreg, xr, yr, lpp, tsec, tlast);
#else
      causal_logp<KT1, KSL1, NTL, R, GRAM, L1M>(lds, m, lane_off, g, j, zp, vreg, xr, yr, lpp);
#endif
      if constexpr (PRIOR) lpp[0] += pr.correction(zp[0], m.q, g);
      PMARK(5);
      // ---- accept / reject   (base.py:868-871).  u(it) = word (it & 3) of Philox(row, it >> 2, 0, TAG_ACC)
      if ((it & 3) == 0 || it == a.it_begin) {
#pragma unroll
        for (int rr = 0; rr < R; ++rr) uacc[rr] = philox4x32_10(rowid[rr], (unsigned)it >> 2, 0u, TAG_ACC, a.k0, a.k1);
      }
      unsigned long long accmask = 0ull;
      [[maybe_unused]] bool moved[R];      // (the same in the four lanes of a chain: lp / lpp are replicated over the lane groups)
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        const unsigned w = (it & 2) ? ((it & 1) ? uacc[rr].w : uacc[rr].z) : ((it & 1) ? uacc[rr].y : uacc[rr].x);
        const float u = u01_open(w);
        const float ratio = fast_exp(fminf(lpp[rr] - lp[rr], 0.0f));
        const bool acc = u < ratio;
        moved[rr] = acc;
#pragma unroll
        for (int t = 0; t < KT1; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) zs[rr][t][r] = acc ? zp[rr][t][r] : zs[rr][t][r];
        lp[rr] = acc ? lpp[rr] : lp[rr];
        if constexpr (ROWADAPT) {
          if (it < a.ra_n) sc[rr] = fminf(fmaxf(sc[rr] * (acc ? a.ra_up : a.ra_dn)[it], a.ra_min), a.ra_max);
        }
        accmask += __popcll(__ballot(acc && valid[rr] && g == 0));
      }
      // per-(wave slot, iteration) counter, slot-private: a shared per-iteration word would take ~1e8
      // atomics/s on one address and saturate it (measured: -30 % kernel throughput)
      // (fire-and-forget atomic: the read-modify-write form made the wave wait for the load of its own counter every iteration)
      if (a.acc_count != nullptr && lane == 0) atomicAdd(&a.acc_count[slot * (long long)a.n_iters + (it - a.it_begin)], (unsigned)accmask);

      PMARK(6);
      if (it >= a.burn_in) {
        const long long d = it - a.burn_in;
        if (a.draws != nullptr) {  // samples.append(current_state.copy())  (base.py:896)
#pragma unroll
          for (int rr = 0; rr < R; ++rr) {
            const long long row = row0 + 16 * rr + j;
            if (row < n) {
              float *dr = a.draws + (d * n + row) * (long long)m.q;
#pragma unroll
              for (int t = 0; t < KT1; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const int f = 16 * t + 4 * r + g;
                  if (f < m.q) dr[f] = zs[rr][t][r];
                }
            }
          }
        }
        if constexpr (EFFECT == 3) {
          // event mode: a chain whose proposal was accepted (or every chain at the launch's first iteration, ev_first) appends
          // (chain, iteration, state) to the slot's region, in time order; nothing else happens at a retained iteration
          static_assert(R == 1, "event mode: one row tile per wave");
          causal_event_append<KT1>(a, m.q, slot, ev_cnt, valid[0] && (moved[0] || (a.ev_first && it == a.it_begin)), g, j, zs[0], it);
        } else if constexpr (EFFECT == 1 && R == 1) {
          float2 *cache = reinterpret_cast<float2 *>(a.eff_cache) + slot * (long long)((a.n_doses + 3) >> 2) * 64;
          float *adrf_slot = a.adrf_partial + slot * (long long)a.n_doses * a.n_keep;
          const bool skip = a.eff_skip && eff_cached && accmask == 0ull;                // wave-uniform: nobody moved
          // (the evaluation is switched off through its trip count: its first layer -- 4 MFMAs per K-step of m.l1b -- still runs)
          causal_effects<KT1, KSL1, R, EFFECT, true, true, false, L1M, false, false, VTAILS>(lds, m, lane_off, g, j, lane, zs, rowid, valid, row0, n, (unsigned)it, d, a.n_keep,
                                                            a.sample_y, skip ? 0 : a.n_doses, a.x_values, adrf_slot, a.ite, a.k0, a.k1, cache);
          if (skip) causal_effects_cached(g, j, lane, rowid[0], valid[0], (unsigned)it, d, a.sample_y, a.n_doses, adrf_slot, a.k0, a.k1, cache);
          eff_cached = true;
          n_eff_skipped += skip ? 1u : 0u;
        } else if constexpr (EFFECT == 2 && R == 1) {
          const bool skip = a.eff_skip && eff_cached && accmask == 0ull;                // wave-uniform: nobody moved
          causal_effects<KT1, KSL1, R, EFFECT, true, true, false, L1M>(lds, m, lane_off, g, j, lane, zs, rowid, valid, row0, n, (unsigned)it, d, a.n_keep,
                                                            a.sample_y, skip ? 0 : 2, a.x_values, a.adrf_partial, a.ite, a.k0, a.k1, nullptr, ite_c);
          if (skip) causal_ite_cached(g, j, rowid[0], row0 + j, n, (unsigned)it, d, a.n_keep, a.sample_y, a.ite, a.k0, a.k1, ite_c);
          eff_cached = true;
          n_eff_skipped += skip ? 1u : 0u;
        } else if constexpr (EFFECT != 0) {
          causal_effects<KT1, KSL1, R, EFFECT, true, false, false, L1M>(lds, m, lane_off, g, j, lane, zs, rowid, valid, row0, n, (unsigned)it, d,
                                                a.n_keep, a.sample_y, a.n_doses, a.x_values,
                                                a.adrf_partial + slot * (long long)((EFFECT == 2) ? 2 : a.n_doses) * a.n_keep,
                                                a.ite, a.k0, a.k1);
        }
      }
    }
    if constexpr (EFFECT != 0 && R == 1) {
      if (a.eff_stats != nullptr && lane == 0 && n_eff_skipped != 0u) atomicAdd(&a.eff_stats[0], (unsigned long long)n_eff_skipped);
    }
    if constexpr (EFFECT == 3) {
      if (lane == 0) { a.tile_ev[2 * tile] = ev_tile0; a.tile_ev[2 * tile + 1] = ev_cnt - ev_tile0; }
    }
    // ---- write the chain state back
    store_z_rows<KT1, R>(a.state, n, m.q, row0, j, g, zs);
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const long long row = row0 + 16 * rr + j;
      if (g == 0 && row < n) a.logp[row] = lp[rr];
      if constexpr (ROWADAPT) {
        if (g == 0 && row < n) a.row_scale[row] = sc[rr];
      }
    }
    ++tiles_done;
  }
  if (lane == 0) prog[wave_u] = 0x7fffffff;   // finished: the partner never needs to catch up
  if constexpr (EFFECT == 3) {
    if (lane == 0) a.slot_cnt[slot] = ev_cnt;
  }
#ifdef BGM_PROF
  if (a.clk != nullptr && lane == 0 && slot == 0) for (int i = 0; i < 8; ++i) a.clk[4ll * gridDim.x * WAVES + i] = tsec[i];
#endif
  if (a.clk != nullptr && lane == 0) {   // [n_slots][4]: cycles, 100 MHz ticks, start tick, XCC id
    a.clk[4 * slot + 0] = __builtin_readcyclecounter() - clk_c0;
    a.clk[4 * slot + 1] = __builtin_amdgcn_s_memrealtime() - clk_r0;
    a.clk[4 * slot + 2] = clk_r0;
    a.clk[4 * slot + 3] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));   // HW_REG_XCC_ID[3:0]
  }
}

// ---------------------------------------------------------------------------
// evaluate (base.py:534-570): reconstruction errors of g, h, f at the given latent matrix and the
// plug-in causal estimate (ITE per row, or the dose-response curve summed over rows).
// sums[0..2] += sum |v - mu_v|^2, sum (x - x_pred)^2, sum (y - mu_y)^2   (x_pred = sigmoid(logit) if binary)
// ---------------------------------------------------------------------------
struct CausalEvalKArgs {
  const float *blob, *x, *y, *v, *z;
  long long n;
  double *sums;
  const float *x_values;
  int n_doses;
  float *adrf_partial;   // [n_slots][n_doses]
  float *ite;            // [n]
  CausalMeta m;
};

template <int KT1, int KSL1, int NTL, int WAVES, int EFFECT>
__global__ __launch_bounds__(64 * WAVES) void causal_eval_kernel(CausalEvalKArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CausalMeta &m = a.m;
  lds_fill(lds, a.blob, m.total);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4, lane_off = 64 * g + j;
  const long long n = a.n, n_tiles = (n + 15) / 16;
  const long long slot = (long long)blockIdx.x * WAVES + wave;
  double sv = 0.0, sx = 0.0, sy = 0.0;
  for (long long tile = slot; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    BGM_NO_HOIST();
    const long long row0 = tile * 16;
    long long row = row0 + j;
    bool valid[1] = {row < n};
    row = row < n ? row : n - 1;
    float xr[1] = {a.x[row]}, yr[1] = {a.y[row]};
    unsigned rowid[1] = {0u};
    f32x4 vreg[1][NTL];
    load_v_rows<NTL, 1>(a.v, lds + m.bgl, n, m.p, row0, j, g, vreg);
    f32x4 zin[1][KT1];
    load_z_rows<KT1, 1>(a.z, n, m.q, row0, j, g, xr, zin);
    float ssq[1] = {0.0f}, sraw[1] = {0.0f};
    {
      f32x4 h[1][4];
      dense<KT1, KSL1, 4, 1>(lds + m.w1g, lds + m.b1g, lane_off, g, zin, h);
      lrelu_s_inplace<4, 1>(h);
      for (int l = 0; l < m.n_gh; ++l) {
        BGM_NO_HOIST();
        f32x4 h2[1][4];
        dense<4, 4, 4, 1>(lds + m.wg + l * 4096, lds + m.bg + l * 64, lane_off, g, h, h2);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) h[0][t][r] = lrelu_s(h2[0][t][r]);
      }
      const int pc = m.sig_pc;
      g_last_groups<0, 4, NTL, 1>(lds + m.wgl, lds + m.bgl, lane_off, g, pc - 4 * g, h, vreg, ssq, sraw);
    }
    float mu_y[1], sr_y[1], mu_x[1], sr_x[1];
    {
      f32x4 a1[1][4];
      dense<KT1, KSL1, 4, 1>(lds + m.w1f, lds + m.b1f, lane_off, g, zin, a1);
      lrelu_s_inplace<4, 1>(a1);
      fh_tail<1>(lds, m.wf2, m.bf2, m.wf3, m.bf3, m.wf4, m.bf4, lane_off, g, a1, mu_y, sr_y);
    }
    {
      f32x4 a1[1][4];
      dense<KT1, KSL1, 4, 1>(lds + m.w1h, lds + m.b1h, lane_off, g, zin, a1);
      lrelu_s_inplace<4, 1>(a1);
      fh_tail<1>(lds, m.wh2, m.bh2, m.wh3, m.bh3, m.wh4, m.bh4, lane_off, g, a1, mu_x, sr_x);
    }
    if (valid[0]) {
      sv += (double)ssq[0];   // every lane group holds its own partial of |v - mu|^2
      if (g == 0) {
        const float xp = m.binary ? 1.0f / (1.0f + expf(-mu_x[0])) : mu_x[0];
        sx += (double)((xr[0] - xp) * (xr[0] - xp));
        sy += (double)((yr[0] - mu_y[0]) * (yr[0] - mu_y[0]));
      }
    }
    if constexpr (EFFECT != 0)
      causal_effects<KT1, KSL1, 1, EFFECT>(lds, m, lane_off, g, j, lane, zin, rowid, valid, row0, n, 0u, 0, 1, 0,
                                           a.n_doses, a.x_values, a.adrf_partial + slot * (long long)a.n_doses,
                                           a.ite, 0u, 0u);
  }
  for (int off = 32; off > 0; off >>= 1) {
    sv += __shfl_xor(sv, off);
    sx += __shfl_xor(sx, off);
    sy += __shfl_xor(sy, off);
  }
  if (lane == 0) {
    atomicAdd(a.sums + 0, sv);
    atomicAdd(a.sums + 1, sx);
    atomicAdd(a.sums + 2, sy);
  }
}

// ---------------------------------------------------------------------------
// infer_from_latent_posterior (base.py:671-763) on a GIVEN tensor of posterior draws [n_keep x n x q]: the same
// effect routine and the same noise counters (iteration = burn_in + d) as the pass fused into the MH kernel, so
// both routes give the same numbers for the same draws.
// ---------------------------------------------------------------------------
struct CausalEffKArgs {
  const float *blob, *x, *draws;
  long long n, row_base;
  int n_keep, burn_in, sample_y, n_doses;
  const float *x_values;
  float *adrf_partial;   // [n_slots][n_keep][n_doses]
  float *ite;            // [n][n_keep]
  unsigned k0, k1;
  CausalMeta m;
};

template <int KT1, int KSL1, int WAVES, int EFFECT>
__global__ __launch_bounds__(64 * WAVES) void causal_effects_kernel(CausalEffKArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CausalMeta &m = a.m;
  lds_fill(lds, a.blob, m.total);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4, lane_off = 64 * g + j;
  const long long n = a.n, n_tiles = (n + 15) / 16;
  const long long slot = (long long)blockIdx.x * WAVES + wave;
  for (long long tile = slot; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    const long long row0 = tile * 16;
    long long row = row0 + j;
    bool valid[1] = {row < n};
    row = row < n ? row : n - 1;
    float xr[1] = {a.x[row]};
    unsigned rowid[1] = {(unsigned)(a.row_base + row)};
    for (int d = 0; d < a.n_keep; ++d) {
      BGM_NO_HOIST();
      f32x4 zin[1][KT1];
      load_z_rows<KT1, 1>(a.draws + (long long)d * n * m.q, n, m.q, row0, j, g, xr, zin);
      causal_effects<KT1, KSL1, 1, EFFECT>(lds, m, lane_off, g, j, lane, zin, rowid, valid, row0, n, (unsigned)(a.burn_in + d), d,
                                           a.n_keep, a.sample_y, a.n_doses, a.x_values,
                                           a.adrf_partial + slot * (long long)a.n_doses * a.n_keep /* unused when EFFECT == 2 */, a.ite,
                                           a.k0, a.k1);
    }
  }
}

// acc[it_begin + i] += sum over wave slots of scratch[slot][i].  A block of 1024 threads takes 64 consecutive iterations: thread
// (i & 63, slot group) adds every 16th slot (rows of 256 contiguous bytes), the 16 groups are combined in LDS (integer sums: any order).
static __global__ __launch_bounds__(1024) void acc_reduce_kernel(const unsigned *scratch, int n_slots, int n_iters, unsigned *acc) {
  __shared__ unsigned part[16][64];
  const int ti = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + ti;
  unsigned s = 0;
  if (i < n_iters)
    for (int k = sg; k < n_slots; k += 16) s += scratch[(long long)k * n_iters + i];
  part[sg][ti] = s;
  __syncthreads();
  if (sg == 0 && i < n_iters) {
#pragma unroll
    for (int u = 1; u < 16; ++u) s += part[u][ti];
    acc[i] += s;
  }
}
