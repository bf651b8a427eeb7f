// causal_hmc_fx_kernels.h -- the HMC transition of the CausalBGM latent sampler (gfx950), chmc_run: ONE body behind all eight
// kernels -- identity mass or the diagonal metric of causal_hmc_mass_kernels.h (MASS), without an effect pass (EFFECT 0:
// causal_hmc_kernel, causal_hmc_mass_kernel) or with it inside the sampler (causal_hmc_fx_kernel, causal_hmc_mass_fx_kernel; the
// per-row and label-sum kernels of causal_hmc_rowfx_kernels.h / causal_hmc_gfx_kernels.h), where no retained draws are needed to
// estimate the dose-response curve or the treatment effects.  The kernels are thin wrappers; which of them a translation unit
// instantiates is decided by its dispatch lambdas.
//
// replaces: nothing in causalbgm/base.py for the transition (the reference samples CausalBGM's latents by random-walk MH only; the
//   transition is that of bgm/base.py:709-830, tfp HamiltonianMonteCarlo); infer_from_latent_posterior (causalbgm/base.py:671-763)
//   for the effect pass, which the reference computes from stored MH draws.
//
// One chain per row, persistent over a segment of iterations.  state, logp, grad and step travel between launches, so a run cut at
// any iteration is the same run.  After the decision of iteration it < n_table the chain's step is multiplied by up[it] (it moved)
// or dn[it] (it did not) and clamped: ONE fp32 multiply (row_adapt.py).
// EFFECT != 0: after the decision of every retained iteration the outcome net is evaluated on the chain's state by causal_effects
// (causal_kernels.h), the routine bgm_causal_effects runs over stored draws; registers, LDS blob, RNG streams, accept rule, step
// table and metric are those of EFFECT 0.
// z is already in its register layout (feature 16 t + 4 r + g, x at feature q), the grid and the tile walk are those of
// causal_effects_kernel (slot = blockIdx.x * WAVES + wave, stride gridDim.x * WAVES), and the noise counters are (row, it): element
// (slot, d, k) of adrf_partial receives the same additions in the same order on both routes, so the fused result IS the two-pass one.
// causal_effects reads f in the layout of the SAMPLING blob (not the dual-access one of the gradient): f's pieces of that blob --
// w1f, b1f, wf2 .. bf4, wxf, 3008 + 1024 KT1 floats -- are copied behind the HMC blob in LDS, byte for byte from where
// bgm_causal_effects reads them.  The call sits where mom / zc / gc are dead.
#pragma once
#include <type_traits>

#include "causal_hmc_mass_kernels.h"
#include "causal_kernels.h"

#define CHMC_FX_PIECES 4

struct CausalHmcFxArgs {
  const float *sblob;                 // the sampling blob (bgm_causal_sampling_blob), global
  int src[CHMC_FX_PIECES];            // f's pieces: cnt floats from sblob + src to lds_f + dst (all multiples of 4)
  int dst[CHMC_FX_PIECES];
  int cnt[CHMC_FX_PIECES];
  CausalMeta mf;                      // offsets of w1f, b1f, wf2 .. bf4, wxf relative to lds_f; q, sig2_y, l1b of the handle's meta
  int n_keep, sample_y, n_doses;
  const float *x_values;
  float *adrf_partial;                // [n_slots][n_keep][n_doses], += (EFFECT 1)
  float *ite;                         // [n][n_keep] (EFFECT 2)
};

// TRAJ (causal_hmc_traj_kernels.h; bgm_causal_hmc_set_trajectory): the number of leapfrog steps of every chain and iteration.  Only
// the TRAJ kernels receive it.
struct CausalHmcTrajArgs {
  float max_traj;                     // cap on eps x L_i (> 0), or 0: none
  int jitter;                         // 0 / 1: L_i uniform on 1 .. cap, drawn per chain and iteration
  int *n_steps;                       // [n] += L_i of every iteration >= burn_in of this launch, or NULL
};

// floats of f's part of the sampling blob
__host__ __device__ constexpr int chmc_fx_floats(int KT1) { return 3008 + 1024 * KT1; }

__device__ __forceinline__ void chmc_fx_fill(float *lds_f, const CausalHmcFxArgs &fx) {
#pragma unroll
  for (int p = 0; p < CHMC_FX_PIECES; ++p) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(fx.sblob + fx.src[p]);
    f32x4 *dst = reinterpret_cast<f32x4 *>(lds_f + fx.dst[p]);
    for (int i = threadIdx.x; i < fx.cnt[p] / 4; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
}

// ROWS (causal_hmc_rowfx_kernels.h, EFFECT 1): the values stay with their rows, in row_mom / row_y (causal_effects, ROWS); fx.adrf_partial
// and fx.ite are not used.
// EFFECT 4 (causal_hmc_gfx_kernels.h): the ITE summed by row label.  fx.n_doses = n_labels, fx.adrf_partial = group_partial
// [n_slots][n_keep][n_labels], and fx.ite, which no ITE is stored through, carries the labels [n] int: as a kernel argument of its
// own the pointer left the KT1 = 1 kernel with a metric a 20-byte private segment.  A row's label is read at the effect call, where
// mom / zc / gc are dead, not held across the leapfrog loop.
// EFFECT 0: no copy of f's pieces, no causal_effects call, fx unused.
// How the body receives the kernel's argument structs decides the code hipcc makes of it: by const
// reference for the kernels with an effect pass (by value every one of them changes), by value for the two kernels without -- with
// references those load every kernel argument in the prologue and hold it in SGPRs (causal_hmc_kernel<1, 8>: 198 -> 199 VGPRs,
// + 167 instructions).
template <class T, int EFFECT>
using chmc_arg = std::conditional_t<EFFECT == 0, T, const T &>;

// OBS (causal_hmc_obs_kernels.h): rows whose outcome, or outcome and treatment, are not observed (NaN in y / x): chmc_logp_grad
// leaves their f / h terms out; nothing else of the transition or of the effect pass, which never reads a row's own x or y, differs.
// TAILS (causal_hmc_tails_kernels.h, with ROWS): the rows' values also enter the two tail buffers of their series, row_tails
// [2][k_tail][n_doses][n] (causal_effects, TAILS); nothing else differs.
// TRAJ (causal_hmc_traj_kernels.h): a number of leapfrog steps per chain and iteration.  From the launch's n_leapfrog = L and the
// chain's step eps as it stands, in fp32 and without a quotient: cap = #{l in 0 .. L-1 : l == 0 or float(l) * eps < max_traj}
// (max_traj = 0: cap = L; with a metric still from eps alone, the scales have geometric mean 1), and with jitter L_i = 1 + min(cap
// - 1, int(u * float(cap))), u = word it & 3 of Philox(row, it >> 2, 1, TAG_HACC) (the accept uniform is call 0), else L_i = cap.
// Every wave owns its 16 chains and chmc_logp_grad holds no barrier, so the wave's loop runs to the largest L_i of its own real
// rows, a uniform value.  A lane past its L_i drifts by 0 and kicks by 0 -- no selects on zc, mom, gc or lpc --: it re-evaluates
// the point of its step L_i - 1 and reproduces that step's gradient and log posterior, so what reaches the accept decision is the
// L_i-step proposal.  L_i depends on (eps, global row, it, seed) only, never on z or the momentum.
// CONTRAST (causal_hmc_contrast_kernels.h, with ROWS): the rows' differences to dose 0 are kept beside their curves, in row_cmom
// [3][n_doses][n], and row_y / row_tails record them instead of the values (causal_effects, CONTRAST); nothing else differs.
// CHOICE (causal_hmc_choice_kernels.h, with ROWS): which dose is the row's best at every retained draw is counted beside its curve, in
// the planes of ch (causal_effects, CHOICE); nothing else differs.
template <int KT1, int KSL1, int WAVES, int EFFECT, bool MASS, bool ROWS = false, bool OBS = false, bool TAILS = false, bool TRAJ = false,
          bool CONTRAST = false, bool CHOICE = false>
__device__ __forceinline__ void chmc_run(float *lds, chmc_arg<CausalHmcKArgs, EFFECT> a, chmc_arg<CausalHmcMassArgs, EFFECT> ma,
                                         chmc_arg<CausalHmcFxArgs, EFFECT> fx, float *row_mom = nullptr, float *row_y = nullptr,
                                         float *row_tails = nullptr, int k_tail = 0,
                                         chmc_arg<CausalHmcTrajArgs, EFFECT> tj = CausalHmcTrajArgs{}, float *row_cmom = nullptr,
                                         chmc_arg<CausalChoiceArgs, EFFECT> ch = CausalChoiceArgs{}) {
  static_assert(!TAILS || ROWS, "TAILS: the tail buffers of the per-row dose-response");
  static_assert(!CONTRAST || (ROWS && !TRAJ), "CONTRAST: the per-row dose-response; no twin with TRAJ");
  static_assert(!CHOICE || (ROWS && !TAILS && !TRAJ && !CONTRAST), "CHOICE: the per-row dose-response; no twin with TAILS, TRAJ or CONTRAST");
  static_assert(!TRAJ || (!TAILS && EFFECT != 4), "TRAJ: no twin of the tail-buffer and label-sum kernels");
  const CausalHmcMeta &m = a.m;
  const CausalMeta &mf = fx.mf;
  lds_fill(lds, a.blob, m.total);
  const float *lds_f = lds + m.total;
  if constexpr (EFFECT != 0) chmc_fx_fill(lds + m.total, fx);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4, lane_off = 64 * g + j;
  const long long n = a.n, n_tiles = (n + 15) / 16;
  const long long slot = (long long)blockIdx.x * WAVES + wave;
  for (long long tile = slot; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    BGM_NO_HOIST();
    const long long row0 = tile * 16;
    long long row = row0 + j;
    const bool ok = row < n;
    row = ok ? row : n - 1;
    const unsigned rowid[1] = {(unsigned)(a.row_base + row)};
    const bool valid[1] = {ok};
    float xr, yr, c, lp;
    f32x4 u2[4], z[1][KT1], gr[KT1];
    chmc_load_row(a.x, a.y, a.uc, n, row, g, xr, yr, u2, c);
    bool has_x = true, has_y = true;
    if constexpr (OBS) chmc_observed(xr, yr, has_x, has_y);
    float eps = a.step[row];
    const long long eoff = row * (long long)m.q + g;      // the lane's first element of the row's [q] in scale / ref / s1 / s2
    if (a.init) {      // current_state ~ N(0, 1) (base.py:842), RNG tag 0: the state the MH sampler starts from
#pragma unroll
      for (int t = 0; t < KT1; ++t) {
        const f32x4 e = box_muller4(philox4x32_10(rowid[0], 0u, (unsigned)(g + 4 * t), TAG_INIT, a.k0, a.k1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 16 * t + 4 * r + g;
          z[0][t][r] = (f < m.q) ? e[r] : (f == m.q ? xr : 0.0f);
        }
      }
      chmc_logp_grad<KT1, OBS>(lds, m, j, g, z[0], u2, c, xr, yr, lp, gr, has_x, has_y);
    } else {
      chmc_load_z<KT1>(a.state, m.q, row, g, xr, z[0]);
      chmc_load_z<KT1>(a.grad, m.q, row, g, 0.0f, gr);
      lp = a.logp[row];
    }
    [[maybe_unused]] int n_taken = 0;      // (TRAJ: the sum of L_i over this launch's retained iterations)
    for (int it = a.it_begin; it < a.it_begin + a.n_iters; ++it) {
      BGM_NO_HOIST();
      f32x4 mom[KT1], zc[KT1], gc[KT1], sc[KT1];
      if constexpr (MASS) chmc_mass_load<KT1>(ma.scale, eoff, m.q, g, sc);
      float ke0 = 0.0f;
#pragma unroll
      for (int t = 0; t < KT1; ++t) {
        const f32x4 e = box_muller4(philox4x32_10(rowid[0], (unsigned)it, (unsigned)(g + 4 * t), TAG_MOM, a.k0, a.k1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pm = (16 * t + 4 * r + g < m.q) ? e[r] : 0.0f;
          ke0 = fmaf(pm, pm, ke0);
          if constexpr (MASS) mom[t][r] = fmaf(0.5f * (eps * sc[t][r]), gr[t][r], pm);      // first half kick
          else mom[t][r] = fmaf(0.5f * eps, gr[t][r], pm);
          zc[t][r] = z[0][t][r];
          gc[t][r] = gr[t][r];
        }
      }
      ke0 = sum_over_g(ke0);
      float lpc = lp;
      [[maybe_unused]] int n_loop = 0;             // (TRAJ: the wave's loop bound)
      [[maybe_unused]] int li = a.n_leapfrog;      // (TRAJ: this chain's steps of this transition, from eps as it stands)
      if constexpr (TRAJ) {
        if (tj.max_traj > 0.0f) {
          li = 1;
          for (int l = 1; l < a.n_leapfrog; ++l) li += ((float)l * eps < tj.max_traj) ? 1 : 0;
        }
        if (tj.jitter) {
          const uint4 j4 = philox4x32_10(rowid[0], (unsigned)it >> 2, 1u, TAG_HACC, a.k0, a.k1);
          const unsigned jw = (it & 2) ? ((it & 1) ? j4.w : j4.z) : ((it & 1) ? j4.y : j4.x);
          const int k = (int)(u01_open(jw) * (float)li);
          li = 1 + (k < li - 1 ? k : li - 1);
        }
        if (it >= a.burn_in) n_taken += li;
        // the largest L_i among the wave's real rows (a row's four lane groups agree; a clamped padding row counts 1)
        int lm = ok ? li : 1;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) lm = max(lm, __shfl_xor(lm, off));
        n_loop = __builtin_amdgcn_readfirstlane(lm);
      }
      for (int l = 0; TRAJ ? l < n_loop : l < a.n_leapfrog; ++l) {
        BGM_NO_HOIST();
        if constexpr (MASS) chmc_mass_load<KT1>(ma.scale, eoff, m.q, g, sc);
        float drift = eps;
        if constexpr (TRAJ) drift = l < li ? eps : 0.0f;      // (past L_i: the same point again)
#pragma unroll
        for (int t = 0; t < KT1; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {      // (the momentum of x and of the padding is zero)
            if constexpr (MASS) zc[t][r] = fmaf(drift * sc[t][r], mom[t][r], zc[t][r]);
            else zc[t][r] = fmaf(drift, mom[t][r], zc[t][r]);
          }
        chmc_logp_grad<KT1, OBS>(lds, m, j, g, zc, u2, c, xr, yr, lpc, gc, has_x, has_y);
        if constexpr (MASS) {
          BGM_NO_HOIST();
          chmc_mass_load<KT1>(ma.scale, eoff, m.q, g, sc);
        }
        float kick = (l < a.n_leapfrog - 1) ? eps : 0.5f * eps;
        if constexpr (TRAJ) kick = (l < li - 1) ? eps : (l == li - 1) ? 0.5f * eps : 0.0f;      // (its half kick at its last step, none after)
#pragma unroll
        for (int t = 0; t < KT1; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (MASS) mom[t][r] = fmaf(kick * sc[t][r], gc[t][r], mom[t][r]);      // (0.5 eps) s = 0.5 (eps s): a power of two
            else mom[t][r] = fmaf(kick, gc[t][r], mom[t][r]);
          }
      }
      float ke1 = 0.0f;
#pragma unroll
      for (int t = 0; t < KT1; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) ke1 = fmaf(mom[t][r], mom[t][r], ke1);
      ke1 = sum_over_g(ke1);
      float log_ratio = -((-lpc + 0.5f * ke1) - (-lp + 0.5f * ke0));
      log_ratio = (log_ratio == log_ratio && fabsf(log_ratio) != INFINITY) ? log_ratio : -INFINITY;
      const uint4 w4 = philox4x32_10(rowid[0], (unsigned)it >> 2, 0u, TAG_HACC, a.k0, a.k1);
      const unsigned w_ = (it & 2) ? ((it & 1) ? w4.w : w4.z) : ((it & 1) ? w4.y : w4.x);
      const bool acc = logf(u01_open(w_)) < log_ratio;
#pragma unroll
      for (int t = 0; t < KT1; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          z[0][t][r] = acc ? zc[t][r] : z[0][t][r];
          gr[t][r] = acc ? gc[t][r] : gr[t][r];
        }
      lp = acc ? lpc : lp;
      if (a.up != nullptr && it < a.n_table) eps = fminf(fmaxf(eps * (acc ? a.up : a.dn)[it], a.s_min), a.s_max);
      if (a.acc_count) {
        const unsigned cnt = (unsigned)__popcll(__ballot(acc && ok && g == 0));
        if (lane == 0 && cnt) atomicAdd(a.acc_count + it, cnt);
      }
      if constexpr (MASS) {
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
                const float d = z[0][t][r] - rf[e];
                s1[e] += d;
                s2[e] = fmaf(d, d, s2[e]);
              }
            }
        }
      }
      if (a.draws != nullptr && it >= a.burn_in && ok) chmc_store_z<KT1>(a.draws + (long long)(it - a.burn_in) * n * m.q, m.q, row, g, z[0]);
      if constexpr (EFFECT != 0) if (it >= a.burn_in) {    // (wave-uniform) infer_from_latent_posterior on the state the chain holds after this decision
        int label = 0;
        if constexpr (EFFECT == 4) label = reinterpret_cast<const int *>(fx.ite)[row];
        causal_effects<KT1, KSL1, 1, EFFECT, true, false, false, true, ROWS, TAILS, false, CONTRAST, CHOICE>(
            lds_f, mf, lane_off, g, j, lane, z, rowid, valid, row0, n, (unsigned)it, (long long)(it - a.burn_in), fx.n_keep, fx.sample_y,
            fx.n_doses, fx.x_values,
            ROWS ? nullptr : fx.adrf_partial + slot * (long long)fx.n_doses * fx.n_keep /* unused when EFFECT == 2 */, fx.ite, a.k0, a.k1,
            nullptr, nullptr, row_mom, row_y, label, row_tails, k_tail, row_cmom, ch);
      }
    }
    if (ok) {
      chmc_store_z<KT1>(a.state, m.q, row, g, z[0]);
      chmc_store_z<KT1>(a.grad, m.q, row, g, gr);
      if (g == 0) { a.logp[row] = lp; a.step[row] = eps; }
      if constexpr (TRAJ)
        if (g == 0 && tj.n_steps != nullptr) tj.n_steps[row] += n_taken;
    }
  }
}

template <int KT1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_kernel(CausalHmcKArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, 1, WAVES, 0, false>(lds, a, CausalHmcMassArgs{}, CausalHmcFxArgs{});
}

template <int KT1, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, 1, WAVES, 0, true>(lds, a, ma, CausalHmcFxArgs{});
}

template <int KT1, int KSL1, int WAVES, int EFFECT>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_fx_kernel(CausalHmcKArgs a, CausalHmcFxArgs fx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, EFFECT, false>(lds, a, CausalHmcMassArgs{}, fx);
}

template <int KT1, int KSL1, int WAVES, int EFFECT>
__global__ __launch_bounds__(64 * WAVES) void causal_hmc_mass_fx_kernel(CausalHmcKArgs a, CausalHmcMassArgs ma, CausalHmcFxArgs fx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  chmc_run<KT1, KSL1, WAVES, EFFECT, true>(lds, a, ma, fx);
}
