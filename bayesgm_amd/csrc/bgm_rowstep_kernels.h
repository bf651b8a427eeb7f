// bgm_rowstep_kernels.h -- BGM Hamiltonian Monte Carlo with a step size per chain, adapted by that chain alone during burn-in (gfx950).
//
// replaces: the one scalar step of tfp.mcmc.SimpleStepSizeAdaptation in tfp_mcmc_sampler (bgm/base.py:798-821), opt-in; the transition
//   is bgm_hmc_kernel's (bgm_kernels.h) and the rule is causal_hmc_kernel's (causal_hmc_kernels.h): the Robbins-Monro table of
//   row_adapt.py, ONE fp32 multiply and a clamp after the accept decision.  One body, bgm_hmc_run<..., STEP>, serves the four kernels.
//
// STEP 1 (bgm_hmc_rows_kernel) adds to the scalar-step transition: eps is read from row_step[row] when a wave takes up a row tile,
// lives in a VGPR, is updated after the decision of iteration it < n_table and written back with the state.  state, logp, grad and
// step travel between launches, so a run cut at any iteration is the same run.
// STEP 2 (bgm_hmc_rows_traj_kernel; opt-in, bgm_bgm_hmc_run_rows_traj) adds a number of leapfrog steps per chain.  From the launch's
// n_leapfrog = L and the chain's current eps, in fp32 and without a quotient: cap = #{l in 0 .. L-1 : l == 0 or float(l) * eps <
// max_traj} (max_traj = 0: cap = L), and with jitter L_i = 1 + min(cap - 1, int(u * float(cap))), u = word it & 3 of Philox(row,
// it >> 2, 1, TAG_HACC) (the accept uniform is call 0), else L_i = cap.  The loop still runs to L for the whole wave -- 16 chains share
// an MFMA tile and the streamed variants need every wave of the workgroup to make the same number of bgm_logp_grad calls -- but a chain
// past its L_i drifts by 0 and kicks by 0: it re-evaluates the point of step L_i - 1 and reproduces that step's gradient and log
// posterior, so what reaches the accept decision is the L_i-step proposal.  L_i depends on (eps, row, it, seed) only, never on z or the
// momentum; n_steps[row] collects the sum of L_i.
// STEP 3 (bgm_hmc_rows_impute_kernel; opt-in, bgm_bgm_hmc_run_rows_impute, fp32) adds to STEP 2 a decode pass after the decision of every
// retained iteration: the predictive value of every missing cell of the state the chain is left in, summed into shifted moments per
// (row, cell) -- bgm_impute_decode below.  The chain itself is STEP 2's (STEP 1's with the trajectory options off), bit for bit.
// STEP 4 (bgm_hmc_rows_impute_tails_kernel; opt-in, bgm_bgm_hmc_run_rows_impute_tails, fp32) adds to STEP 3 the two tails of every missing
// cell that has a slot: the k_tail smallest and the k_tail largest of its predictive values, two heaps in global memory (row_tail_push,
// row_tails.h), from which bgm_row_tail_quantiles gives the quantile pair of the stored cells bit for bit.  Chain, planes and cells are
// STEP 3's.
#pragma once
#include "bgm_kernels.h"
#include "row_tails.h"

struct BgmRowHmcKArgs : BgmHmcKArgs {      // STEP 1 (BgmHmcKArgs::step is not read)
  float *row_step;           // [n] step size of every chain, in / out
  const float *up, *dn;      // [n_table] factor after the decision of iteration it < n_table (moved / did not), or NULL: fixed steps
  int n_table;
  float s_min, s_max;
};
struct BgmTrajHmcKArgs : BgmRowHmcKArgs {  // STEP 2
  float max_traj;            // cap on eps x L_i (> 0), or 0: none
  int jitter;                // 0 / 1: L_i uniform on 1 .. cap, drawn per chain and iteration
  int *n_steps;              // [n] += the leapfrog steps the chain took over this launch's iterations, or NULL
};
struct BgmImputeHmcKArgs : BgmTrajHmcKArgs {  // STEP 3
  float *moments;            // [3][n][p]: ref (the predictive value at retained draw 0), sum (x - ref), sum (x - ref)^2; missing cells only
  float *cells;              // [(row * k_slots + slot) * n_keep + d] as bgm_predict_kernel's, or NULL
  const int *slot;           // [n x p] (read only with cells)
  int k_slots, n_keep;
  int add_noise;             // 0: the head's mean instead of a draw
};
struct BgmImputeTailsHmcKArgs : BgmImputeHmcKArgs {  // STEP 4 (slot and k_slots are required)
  float *tails;              // [2][k_tail][n][k_slots]: tail t, heap slot s of series row * k_slots + slot[row * p + c]; in / out, never read at d = 0
  int k_tail;                // 1 .. n_keep
};

// STEP 3: the predictive value of every MISSING cell of the state a retained transition ends on, summarised where it is made.  The
// trunk, the head tile and the noise are bgm_predict_kernel's (bgm_kernels.h) -- copied, not shared: that kernel's lambda also serves
// full / var_full and its code object must stay what it is -- with Philox counter (row, it, 4 tx + g, TAG_XNOISE), it = burn_in + d, so a
// value is bit for bit what bgm_bgm_predict_draws makes of the stored draw d.  Lane (j, g), register r owns cell c = 16 tx + 4 g + r of
// row j and no other lane touches it: plain loads and stores.  Shifted sums as in causal_hmc_rowfx_kernels.h: plane 0 holds the value at
// it == burn_in, planes 1 / 2 the sums of (x - ref) and (x - ref)^2 over the retained iterations, so launches cut anywhere add up to the
// same bits.  Streamed variant: one walk of the head stream exactly as a gradient evaluation makes it, by EVERY wave of the workgroup.
// TAILS (STEP 4, Args = BgmImputeTailsHmcKArgs): after the tile's moment stores the owner of a missing cell with a slot pushes the value
// into the cell's two heaps, tail 0 (max-heap) first.  The series of cell (row, slot) is row * k_slots + slot, the default route's
// [n, k_slots] indexing, and two heap slots of a series lie n * k_slots floats apart.  Nothing is carried over the iterations: d, k_tail
// and the buffer are the whole state.  The tails add no step of the head stream.
template <int KTQ, int NTX, int NH, bool TAILS = false, class Args, class HS>
__device__ __forceinline__ void bgm_impute_decode(const Args &a, const float *lds, HS &hs, int j, int g, const f32x4 (&z)[KTQ],
                                                  const BgmX<NTX> &xs, long long row, unsigned rowid, bool ok, int it) {
  const BgmMeta &m = a.m;
  f32x4 h[4], h2[4];
  bias17<4>(lds + m.b1, g, h);
  fwd17<KTQ, 4>(lds + m.w1, j, g, z, h);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) h[t][r] = lrelu(h[t][r]);
  for (int l = 1; l < NH; ++l) {
    BGM_NO_HOIST();
    bias17<4>(lds + m.bh + (l - 1) * 64, g, h2);
    fwd17<4, 4>(lds + m.wh + (l - 1) * (4 * 64 * 17), j, g, h, h2);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) h[t][r] = lrelu(h2[t][r]);
  }
  const long long plane = a.n * (long long)m.p;
  auto head = [&](int tx, const float *wl, f32x4 xv) {
    // (g and the data values do not change over the iterations: without this empty asm statement the column tests, the missing-cell
    // tests, the cell addresses and the first Philox round of every tile are formed once at kernel entry and stay live -- DESIGN 4aa)
    asm volatile("" : "+v"(g), "+v"(xv));
    const long long cell0 = row * (long long)m.p + 16 * tx + 4 * g;
    // the tile's loads first, all of them and ahead of the head product, then the arithmetic, then the stores: a cell at a time every
    // wave waits out three dependent round trips to memory per cell (measured: the decode then costs 2.5 gradient evaluations at p = 500)
    float *mo = a.moments + cell0;
    const bool first = it == a.burn_in;
    bool mine[4];
    float ref[4], s1[4], s2[4];
    int sl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mine[r] = ok && 16 * tx + 4 * g + r < m.p && xv[r] != xv[r];      // (NaN = missing; an observed cell and a column beyond p are never touched)
      ref[r] = s1[r] = s2[r] = 0.0f;
      sl[r] = -1;
      if (mine[r] && !first) { ref[r] = mo[r]; s1[r] = mo[plane + r]; s2[r] = mo[2 * plane + r]; }
      if (mine[r] && (TAILS || a.cells != nullptr)) sl[r] = a.slot[cell0 + r];
    }
    f32x4 ms[2];
    ms[0] = *reinterpret_cast<const f32x4 *>(lds + m.bhd + 16 * tx + 4 * g);
    ms[1] = *reinterpret_cast<const f32x4 *>(lds + m.bhd + 16 * (m.ntx + tx) + 4 * g);
    heads_fwd17(wl, j, g, h, ms);
    const f32x4 e = box_muller4(philox4x32_10(rowid, (unsigned)it, (unsigned)(4 * tx + g), TAG_XNOISE, a.k0, a.k1));
    [[maybe_unused]] float xt[4];      // (TAILS: the tile's values, pushed after its stores)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = softplus_f(ms[1][r]) + BGM_EPS;
      const float xp = a.add_noise ? fmaf(__builtin_sqrtf(v), e[r], ms[0][r]) : ms[0][r];
      if constexpr (TAILS) xt[r] = xp;
      if (mine[r]) {
        if (first) {
          mo[r] = xp; mo[plane + r] = 0.0f; mo[2 * plane + r] = 0.0f;
        } else {
          const float d = xp - ref[r];
          mo[plane + r] = s1[r] + d;
          mo[2 * plane + r] = fmaf(d, d, s2[r]);
        }
        if (sl[r] >= 0 && (!TAILS || a.cells != nullptr)) a.cells[(row * (long long)a.k_slots + sl[r]) * a.n_keep + (it - a.burn_in)] = xp;
      }
    }
    if constexpr (TAILS) {
      const long long series = a.n * (long long)a.k_slots;      // floats between two heap slots of a series
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (mine[r] && sl[r] >= 0) {
          float *t0 = a.tails + row * (long long)a.k_slots + sl[r];
          row_tail_push<true>(t0, series, a.k_tail, (long long)(it - a.burn_in), xt[r]);
          row_tail_push<false>(t0 + (long long)a.k_tail * series, series, a.k_tail, (long long)(it - a.burn_in), xt[r]);
        }
      }
    }
  };
  if constexpr (NTX > 0) {
#pragma unroll
    for (int tx = 0; tx < NTX; ++tx) {
      BGM_NO_HOIST();
      head(tx, lds + m.whd + tx * BGM_PAIR, xs.r[tx]);
    }
  } else {
#pragma unroll 1
    for (int tx = 0; tx < m.ntx; ++tx) {      // (tile 0 is current on entry and again on exit, as around bgm_logp_grad)
      BGM_NO_HOIST();
      hs.fetch(tx + 1 < m.ntx ? tx + 1 : 0);
      f32x4 xv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * tx + 4 * g + r;
        xv[r] = (c < m.p) ? xs.row[c] : 0.0f;
      }
      head(tx, hs.tile(), xv);
      hs.commit();
    }
  }
}

// The transition of the four kernels below, once: bgm_hmc_kernel's (bgm_kernels.h) line for line, and under if constexpr what a rule adds.
// STEP 1 (BgmRowHmcKArgs): the step per chain.  STEP 2 (BgmTrajHmcKArgs): STEP 1 and the number of leapfrog steps per chain -- the
// lines on li, n_taken, drift, kick and want_lp, and n_steps written back.  With every step equal and no table STEP 1 gives
// bgm_hmc_kernel's bits; with max_traj = 0 and no jitter STEP 2 gives STEP 1's.  STEP 3 (BgmImputeHmcKArgs): STEP 2 and the decode pass of
// bgm_impute_decode after the decision of every retained iteration; the chain is STEP 2's.  STEP 4 (BgmImputeTailsHmcKArgs): STEP 3 with
// the tails of bgm_impute_decode<..., TAILS>.
template <int KTQ, int NTX, int NH, int WAVES, int PREC, bool X4, int STEP, class Args, class HS>
__device__ __forceinline__ void bgm_hmc_run(Args a, float *lds, HS &hs) {
  const BgmMeta &m = a.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const long long n = a.n, n_tiles = (n + 15) / 16, passes = bgm_block_passes(n_tiles, WAVES);
  for (long long ps = 0; ps < passes; ++ps) {
    // Wide variant: tiles are dealt wave-major (wave w of every block before wave w + 1 of any), so the tiles of a partly filled last
    // round spread over ALL blocks as whole waves; a wave without a tile only keeps the block's head stream moving (no matrix work).
    // The round then costs what its ceil(active waves / 4) waves per SIMD cost instead of a full round on some CUs.
    long long tile = NTX == 0 ? (ps * WAVES + wave) * gridDim.x + blockIdx.x : (ps * gridDim.x + blockIdx.x) * WAVES + wave;
    const bool tile_ok = tile < n_tiles;
    if (NTX > 0 && !tile_ok) break;
    if constexpr (NTX == 0) {
      if (!tile_ok) {
        int evals = (a.init ? 1 : 0) + a.n_iters * a.n_leapfrog;
        if constexpr (STEP >= 3) {      // (one more walk of the stream per retained iteration of this launch: the decode pass)
          const int first = a.it_begin > a.burn_in ? a.it_begin : a.burn_in, kept = a.it_begin + a.n_iters - first;
          evals += kept > 0 ? kept : 0;
        }
        const int n_steps = PREC == 0 ? m.ntx : (m.ntx + BGM_X3_STEP - 1) / BGM_X3_STEP + (PREC == 2 ? 2 * ((NH + BGM_X3_STEP - 1) / BGM_X3_STEP) : 0);      // (steps of the stream per evaluation)
        for (int e = 0; e < evals; ++e)
          for (int tx = 0; tx < n_steps; ++tx) { hs.fetch(tx + 1 < n_steps ? tx + 1 : 0); hs.commit(); }
        continue;
      }
    }
    tile = tile_ok ? tile : n_tiles - 1;
    long long row = tile * 16 + j;
    const bool ok = tile_ok && row < n;
    row = row < n ? row : n - 1;
    const unsigned rowid = (unsigned)(a.row_base + row);
    BgmX<NTX> xr;
    f32x4 z[KTQ], gr[KTQ];
    bgm_load_x<NTX>(a.x, n, m.p, row, g, xr);
    if constexpr (PREC >= 1) hs.x_valid = false;       // (a new row: nothing of it has been requested ahead)
    float eps = a.row_step[row];      // (every pass: the rows are new)
    float lp;
    int n_taken = 0;      // (STEP 2: leapfrog steps of this chain over the launch)
    if (a.init) {   // initial_state ~ N(0,1)  (bgm/base.py:778), RNG tag 0
#pragma unroll
      for (int t = 0; t < KTQ; ++t) {
        const f32x4 e = box_muller4(philox4x32_10(rowid, 0u, (unsigned)(g + 4 * t), TAG_INIT, a.k0, a.k1));
#pragma unroll
        for (int r = 0; r < 4; ++r) z[t][r] = (16 * t + 4 * r + g < m.q) ? e[r] : 0.0f;
      }
      bgm_logp_grad<KTQ, NTX, NH, true, PREC, HS>(lds, m, j, g, z, xr, hs, lp, gr);
    } else {
      bgm_load_z<KTQ>(a.state, m.q, row, g, z);
      bgm_load_z<KTQ>(a.grad, m.q, row, g, gr);
      lp = a.logp[row];
    }
    for (int it = a.it_begin; it < a.it_begin + a.n_iters; ++it) {
      BGM_NO_HOIST();
      f32x4 mom[KTQ], zc[KTQ], gc[KTQ];
      float ke0 = 0.0f;
#pragma unroll
      for (int t = 0; t < KTQ; ++t) {
        const f32x4 e = box_muller4(philox4x32_10(rowid, (unsigned)it, (unsigned)(g + 4 * t), TAG_MOM, a.k0, a.k1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pm = (16 * t + 4 * r + g < m.q) ? e[r] : 0.0f;
          ke0 = fmaf(pm, pm, ke0);
          mom[t][r] = fmaf(0.5f * eps, gr[t][r], pm);   // first half kick
          zc[t][r] = z[t][r];
        }
      }
      ke0 = sum_over_g(ke0);
      float lpc = lp;
      int li = a.n_leapfrog;      // (STEP 2: this chain's steps of this transition, from eps as it stands)
      if constexpr (STEP >= 2) {
        if (a.max_traj > 0.0f) {
          li = 1;
          for (int l = 1; l < a.n_leapfrog; ++l) li += ((float)l * eps < a.max_traj) ? 1 : 0;
        }
        if (a.jitter) {
          const uint4 j4 = philox4x32_10(rowid, (unsigned)it >> 2, 1u, TAG_HACC, a.k0, a.k1);
          const unsigned jw = (it & 2) ? ((it & 1) ? j4.w : j4.z) : ((it & 1) ? j4.y : j4.x);
          const int k = (int)(u01_open(jw) * (float)li);
          li = 1 + (k < li - 1 ? k : li - 1);
        }
        n_taken += li;
      }
      for (int l = 0; l < a.n_leapfrog; ++l) {
        BGM_NO_HOIST();
        float drift = eps;
        if constexpr (STEP >= 2) drift = l < li ? eps : 0.0f;      // (past L_i: the same point again)
#pragma unroll
        for (int t = 0; t < KTQ; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) zc[t][r] = fmaf(drift, mom[t][r], zc[t][r]);
        // (STEP 2: the value of the log posterior from this chain's last step on; its half kick there, none after)
        bool want_lp = PREC == 0 || l == a.n_leapfrog - 1;
        if constexpr (STEP >= 2) want_lp = PREC == 0 || l >= li - 1;
        bgm_logp_grad<KTQ, NTX, NH, true, PREC, HS>(lds, m, j, g, zc, xr, hs, lpc, gc, want_lp);
        float kick = (l < a.n_leapfrog - 1) ? eps : 0.5f * eps;
        if constexpr (STEP >= 2) kick = (l < li - 1) ? eps : (l == li - 1) ? 0.5f * eps : 0.0f;
#pragma unroll
        for (int t = 0; t < KTQ; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) mom[t][r] = fmaf(kick, gc[t][r], mom[t][r]);
      }
      float ke1 = 0.0f;
#pragma unroll
      for (int t = 0; t < KTQ; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) ke1 = fmaf(mom[t][r], mom[t][r], ke1);
      ke1 = sum_over_g(ke1);
      float log_ratio = -((-lpc + 0.5f * ke1) - (-lp + 0.5f * ke0));
      log_ratio = (log_ratio == log_ratio && fabsf(log_ratio) != INFINITY) ? log_ratio : -INFINITY;
      const uint4 w4 = philox4x32_10(rowid, (unsigned)it >> 2, 0u, TAG_HACC, a.k0, a.k1);
      const unsigned w_ = (it & 2) ? ((it & 1) ? w4.w : w4.z) : ((it & 1) ? w4.y : w4.x);
      const float u = u01_open(w_);
      const bool acc = logf(u) < log_ratio;
#pragma unroll
      for (int t = 0; t < KTQ; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          z[t][r] = acc ? zc[t][r] : z[t][r];
          gr[t][r] = acc ? gc[t][r] : gr[t][r];
        }
      lp = acc ? lpc : lp;
      if (a.up != nullptr && it < a.n_table) eps = fminf(fmaxf(eps * (acc ? a.up : a.dn)[it], a.s_min), a.s_max);
      // per-iteration statistics for SimpleStepSizeAdaptation and the acceptance report
      {
        float pa = (ok && g == 0) ? expf(fminf(log_ratio, 0.0f)) : 0.0f;
        for (int off = 8; off > 0; off >>= 1) pa += __shfl_xor(pa, off);
        const unsigned cnt = (unsigned)__popcll(__ballot(acc && ok && g == 0));
        if (lane == 0) {
          if (a.acc_prob_sum) atomicAdd(a.acc_prob_sum + it, (double)pa);
          if (a.acc_count) atomicAdd(a.acc_count + it, cnt);
        }
      }
      if (a.draws != nullptr && it >= a.burn_in && ok)
        bgm_store_z<KTQ>(a.draws + (long long)(it - a.burn_in) * n * m.q, m.q, row, g, z);
      if constexpr (STEP >= 3) {      // (mom, zc and gc are dead here; it >= burn_in is the same for every wave of the launch)
        if (it >= a.burn_in) bgm_impute_decode<KTQ, NTX, NH, (STEP >= 4)>(a, lds, hs, j, g, z, xr, row, rowid, ok, it);
      }
    }
    if (ok) {
      bgm_store_z<KTQ>(a.state, m.q, row, g, z);
      bgm_store_z<KTQ>(a.grad, m.q, row, g, gr);
      if (g == 0) { a.logp[row] = lp; a.row_step[row] = eps; }
      if constexpr (STEP >= 2)
        if (g == 0 && a.n_steps != nullptr) a.n_steps[row] += n_taken;
    }
  }
}

// The text of the kernels.  The LDS fill and the head stream's begin stay in the kernel itself: they read blockDim.x, and hipcc
// folds that read to the workgroup size only where it meets it in a kernel before the first common-subexpression pass -- inside
// bgm_hmc_run the streamed fp32 kernels kept a select on the workgroup id in the stream's fetch loops.
#define BGM_HMC_KERNEL(STEP)                                                   \
  extern __shared__ __attribute__((aligned(16))) float lds[];                  \
  lds_fill(lds, a.blob, a.m.lds_resident);                                     \
  typename bgm_stream_of<PREC, WAVES, X4>::type hs;                            \
  if constexpr (PREC >= 1) hs.begin(a.hx3, a.m, lds);                          \
  else if constexpr (NTX == 0) hs.begin(a.blob, a.m, lds);                     \
  bgm_hmc_run<KTQ, NTX, NH, WAVES, PREC, X4, STEP>(a, lds, hs);

template <int KTQ, int NTX, int NH, int WAVES, int PREC = 0, bool X4 = false>
__global__ __launch_bounds__(64 * WAVES) void bgm_hmc_rows_kernel(BgmRowHmcKArgs a) { BGM_HMC_KERNEL(1) }

template <int KTQ, int NTX, int NH, int WAVES, int PREC = 0, bool X4 = false>
__global__ __launch_bounds__(64 * WAVES) void bgm_hmc_rows_traj_kernel(BgmTrajHmcKArgs a) { BGM_HMC_KERNEL(2) }

// fp32 only (instantiated in bgm_impute_api.hip)
template <int KTQ, int NTX, int NH, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void bgm_hmc_rows_impute_kernel(BgmImputeHmcKArgs a) {
  constexpr int PREC = 0;
  constexpr bool X4 = false;
  BGM_HMC_KERNEL(3)
}

// fp32 only (instantiated in bgm_impute_tails_api.hip)
template <int KTQ, int NTX, int NH, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void bgm_hmc_rows_impute_tails_kernel(BgmImputeTailsHmcKArgs a) {
  constexpr int PREC = 0;
  constexpr bool X4 = false;
  BGM_HMC_KERNEL(4)
}
