// bnw_api.hip -- host side of the any-width sampling / evaluation path of CausalBGM with Bayesian networks (bnw_kernels.h).  Entered
// from the bgm_bnn_* entry points (bnn_sample_api.hip) when no LDS-fragment family holds the session's shape (bnn_sample_host.h).
#include <algorithm>
#include <cstring>
#include <string>

#include "bgm_host.h"
#include "bnn_state.h"
#include "bnw_kernels.h"

struct BnwState {
  float *dw = nullptr, *ws = nullptr, *loct = nullptr;
  BnwNets *nets = nullptr;      // [2]: the nets of the call's sets, the outcome net's own
  size_t dw_cap = 0, ws_cap = 0, loct_cap = 0;
  float *st = nullptr;          // batch statistics (params['bnn_norm'] = "batch"), doubles: [2 parities][n_blocks][256] | x [n_blocks][2] | v [2][p]
  size_t st_cap = 0;
};

void bnw_free(void *p) {
  BnwState *b = static_cast<BnwState *>(p);
  if (!b) return;
  if (b->dw) hipFree(b->dw);
  if (b->ws) hipFree(b->ws);
  if (b->loct) hipFree(b->loct);
  if (b->nets) hipFree(b->nets);
  if (b->st) hipFree(b->st);
  delete b;
}

namespace {
int bnw_need(BnnState *s, const char *who) {
  if (s->cfg.norm_mode != 1 && s->q > 64) {
    bgm_set_error(std::string(who) + ": batch statistics (params['bnn_norm'] = 'batch') hold at most 64 latent columns");
    return BGM_E_UNSUPPORTED;
  }
  for (int k = 0; k < 4; ++k)
    if (s->net[k].n_layers < 1) { bgm_set_error(std::string(who) + ": bad network"); return BGM_E_UNSUPPORTED; }
  return BGM_OK;
}
// sets of this launch hold the nets listed in ids (order = layout)
void bnw_nets(const BnnState *s, const int *ids, int n_ids, BnwNets &m) {
  std::memset(&m, 0, sizeof(m));
  for (int k = 0; k < 4; ++k) { m.net[k] = s->net[k]; m.net[k].bn_fixed = 1; m.noff[k] = -1; }      // ("batch": every call is given its block's statistics, BnwStats)
  long long off = 0;
  for (int i = 0; i < n_ids; ++i) { m.noff[ids[i]] = (int)off; off += (s->net[ids[i]].eoff[s->net[ids[i]].n_layers] + 3) & ~3; }
  m.set_floats = off;
  m.theta = s->theta_dev;
  m.q = s->q; m.p = s->p; m.z0 = s->cfg.z_dims[0]; m.z1 = s->cfg.z_dims[1]; m.z2 = s->cfg.z_dims[2]; m.binary = s->cfg.binary_treatment;
  const BnnSig2 sig2 = bnn_sig2(s->cfg);
  m.sig2[0] = sig2.v; m.sig2[1] = sig2.x; m.sig2[2] = sig2.y;
}
const int kGhf[3] = {BNN_G, BNN_H, BNN_F}, kGhfe[4] = {BNN_G, BNN_H, BNN_F, BNN_E}, kF[1] = {BNN_F};
int bnw_tiles(int bs) { return (bs + BNW_RT - 1) / BNW_RT; }      // row tiles of a block

#define BNW_LDS_BYTES (sizeof(float) * 2 * BNW_STAGE_FLOATS)      // the double-buffered stage of bnw_gemm2
struct BnwPlan { BnwState *b; int grid; long long ws_stride; };
int bnw_plan(bgm_handle *h, BnnState *s, const BnwNets &m, long long n_sets_total, int n_items, BnwPlan &pl, hipStream_t stream) {
  if (!s->bnw) s->bnw = new BnwState();
  BnwState *b = static_cast<BnwState *>(s->bnw);
  pl.b = b;
  pl.grid = std::max(1, std::min(n_items, 4 * h->n_cus));
  pl.ws_stride = (long long)((bnw_ws_floats(m) + 63) & ~(size_t)63);
  int rc = bnn_reserve(b->ws, b->ws_cap, (size_t)pl.ws_stride * (size_t)(4 * h->n_cus), stream);
  if (rc) return rc;
  rc = bnn_reserve(b->dw, b->dw_cap, (size_t)n_sets_total * (size_t)m.set_floats + 64, stream);
  if (rc) return rc;
  rc = bnn_reserve(b->loct, b->loct_cap, 2 * (size_t)m.set_floats + 128, stream);      // the call's sets and the outcome net's own sets
  if (rc || (rc = bnn_pair(s))) return rc;
  if (!b->nets) {
    BGM_HIP_CHECK(hipMalloc((void **)&b->nets, 2 * sizeof(BnwNets)));
    if ((rc = bgm_set_lds(bnw_rows_kernel, (int)BNW_LDS_BYTES)) || (rc = bgm_set_lds(bnw_effects_kernel, (int)BNW_LDS_BYTES))) return rc;
  }
  return BGM_OK;
}
// transposed posterior means of the nets of m's sets at loct + at (the launches of one call read them; theta may change between calls)
int bnw_pack(BnwState *b, BnwNets &m, size_t at, hipStream_t stream) {
  float *dst = b->loct + at;
  long long mx = 0;
  for (int k = 0; k < 4; ++k) if (m.noff[k] >= 0) mx = std::max<long long>(mx, m.net[k].eoff[m.net[k].n_layers]);
  hipLaunchKernelGGL(bnw_pack_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(256, (mx + 255) / 256))), dim3(256), 0, stream, m, dst);
  BGM_HIP_CHECK(hipGetLastError());
  m.locT = dst;
  m.dev = b->nets + (at ? 1 : 0);      // the kernels' copy of the nets (device memory: bnw_kernels.h BnwRowsArgs::mp)
  static_assert(sizeof(BnwNets) % 4 == 0, "BnwNets is copied in words");
  hipLaunchKernelGGL(bnw_store_nets_kernel, dim3(1), dim3(64), 0, stream, m, b->nets + (at ? 1 : 0));
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
// batch statistics: zeroed buffers of this call; stats(par) = the parity a launch accumulates into
struct BnwBatch {
  bool on = false;
  double *stats = nullptr, *xstats = nullptr, *vstats = nullptr;
  int n_blocks = 0;
  const double *parity(int par) const { return on ? stats + (long long)par * n_blocks * 256 : nullptr; }
};
int bnw_batch(BnnState *s, BnwState *b, int n_blocks, BnwBatch &bt, hipStream_t stream) {
  bt.on = s->cfg.norm_mode != 1;
  bt.n_blocks = n_blocks;
  if (!bt.on) return BGM_OK;
  const size_t doubles = (size_t)2 * n_blocks * 256 + (size_t)2 * n_blocks + (size_t)2 * s->p + 16;
  int rc = bnn_reserve(b->st, b->st_cap, 2 * doubles, stream);
  if (rc) return rc;
  bt.stats = reinterpret_cast<double *>(b->st);
  bt.xstats = bt.stats + (size_t)2 * n_blocks * 256;
  bt.vstats = bt.xstats + (size_t)2 * n_blocks;
  BGM_HIP_CHECK(hipMemsetAsync(b->st, 0, sizeof(double) * doubles, stream));
  return BGM_OK;
}
// Statistics pass: column sums of the states sa.z (slot 1) and of their proposals of iteration sa.it (slot 0) into parity sa.par; with
// sa.xstats, the treatment column sa.x too.  The fields a call fixes:
BnwStatArgs bnw_stat_args(const BnwBatch &bt, const BnnRows &r, int q, uint64_t seed) {
  BnwStatArgs sa{};
  sa.n = r.n; sa.row_base = r.row_base; sa.q = q; sa.bs = r.bs; sa.wg_per_block = (r.bs + 255) / 256;
  sa.k0 = (uint32_t)seed; sa.k1 = (uint32_t)(seed >> 32); sa.stats = bt.stats; sa.n_blocks = bt.n_blocks;
  return sa;
}
void bnw_stats(const BnwStatArgs &sa, hipStream_t stream) {
  hipLaunchKernelGGL(bnw_stats_kernel, dim3((unsigned)(sa.n_blocks * sa.wg_per_block)), dim3(256), 0, stream, sa);
}
// one set per block and call; call c draws from stream stream0 + c
void bnw_noise(const BnwNets &m, float *dw, const BnnRows &r, int n_calls, uint64_t seed, uint32_t stream0, hipStream_t stream) {
  BnwNoiseArgs na{};
  na.m = m; na.dw = dw; na.n_calls = n_calls; na.block0 = r.block0;
  na.k0 = (uint32_t)seed; na.k1 = (uint32_t)(seed >> 32); na.stream0 = stream0; na.stream_stride = 1u;
  long long mx = 0;
  for (int k = 0; k < 4; ++k) if (m.noff[k] >= 0) mx = std::max<long long>(mx, m.net[k].eoff[m.net[k].n_layers]);
  const int gx = (int)std::max<long long>(1, std::min<long long>(64, (mx / 4 + 255) / 256));
  hipLaunchKernelGGL(bnw_noise_kernel, dim3(gx, r.n_blocks * n_calls), dim3(256), 0, stream, na);
}
// the fields a call fixes of its bnw_rows_kernel launches (a.m is the caller's: bnw_nets, bnw_pack)
void bnw_rows_args(BnwRowsArgs &a, const BnwPlan &pl, const BnnRows &r, int n_calls, uint64_t seed) {
  a.mp = a.m.dev; a.dw = pl.b->dw; a.n_calls = n_calls; a.n = r.n; a.row_base = r.row_base; a.bs = r.bs; a.block0 = r.block0;
  a.tiles_per_block = bnw_tiles(r.bs); a.n_items = r.n_blocks * a.tiles_per_block;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.ws = pl.b->ws; a.ws_stride = pl.ws_stride;
}
void bnw_launch_rows(const BnwPlan &pl, const BnwRowsArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(bnw_rows_kernel, dim3(pl.grid), dim3(BNN_THREADS), BNW_LDS_BYTES, stream, a);
}

// the effects launches of one call: everything but the draw.  dw: where the outcome net's sets (one per block and dose) go
struct BnwEffects { BnwEffArgs e; BnnRows r; uint64_t seed; int grid; };
BnwEffects bnw_effects_begin(const BnwNets &mf, const BnwPlan &pl, float *dw, const BnnRows &r, uint64_t seed, int sample_y) {
  BnwEffects x{BnwEffArgs{}, r, seed, pl.grid};
  BnwEffArgs &e = x.e;
  e.m = mf; e.mp = mf.dev; e.dw = dw; e.n = r.n; e.row_base = r.row_base; e.bs = r.bs; e.block0 = r.block0;
  e.tiles_per_block = bnw_tiles(r.bs); e.n_items = r.n_blocks * e.tiles_per_block;
  e.k0 = (uint32_t)seed; e.k1 = (uint32_t)(seed >> 32); e.sample_y = sample_y;
  e.ws = pl.b->ws; e.ws_stride = pl.ws_stride;
  return x;
}
// effects of ONE draw (states z; stats: their batch statistics, or NULL)
int bnw_effects_of(BnwEffects &x, const BnnEffectSlot &sl, const float *z, const double *stats, uint32_t it_noise, hipStream_t stream) {
  BnwEffArgs &e = x.e;
  bnw_noise(e.m, const_cast<float *>(e.dw), x.r, sl.n_doses, x.seed, sl.stream0, stream);
  e.stats = stats; e.z = z; e.n_doses = sl.n_doses; e.xvals = sl.xvals; e.stream0 = sl.stream0; e.it_noise = it_noise;
  e.sum_out = sl.sum_out; e.sum_stride = sl.stride; e.ite_out = sl.ite_out; e.ite_stride = sl.stride;
  hipLaunchKernelGGL(bnw_effects_kernel, dim3(std::max(1, std::min(e.n_items, x.grid))), dim3(BNN_THREADS), BNW_LDS_BYTES, stream, e);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
}  // namespace

int bnw_logpost(bgm_handle *h, BnnState *s, const BnnLogpostCall &c, hipStream_t stream) {
  int rc = bnw_need(s, "bgm_bnn_logpost");
  if (rc) return rc;
  BnwRowsArgs a{};
  bnw_nets(s, kGhf, 3, a.m);
  const BnnRows r = bnn_rows(c.n, c.block_rows, c.block0, 0);
  BnwPlan pl;
  rc = bnw_plan(h, s, a.m, r.n_blocks, r.n_blocks * bnw_tiles(r.bs), pl, stream);
  if (rc) return rc;
  if ((rc = bnw_pack(pl.b, a.m, 0, stream))) return rc;
  bnw_noise(a.m, pl.b->dw, r, 1, c.seed, c.stream_id, stream);
  BnwBatch bt;
  rc = bnw_batch(s, pl.b, r.n_blocks, bt, stream);
  if (rc) return rc;
  if (bt.on) {                          // the call's batch = a block of rows: its statistics (slot 1 = the states themselves)
    BnwStatArgs sa = bnw_stat_args(bt, r, s->q, c.seed);
    sa.z = c.z; sa.x = c.x; sa.xstats = bt.xstats;
    bnw_stats(sa, stream);
    a.stats = bt.parity(0); a.xstats = bt.xstats;
  }
  if (s->bp_on) {                       // conditional prior: one noisy call of the prior net for this evaluation (bprior_api.hip)
    if ((rc = bprior_rows(h, s, c.n, r.bs, c.block0, c.seed, c.stream_id, 1, stream))) return rc;
    a.prior = s->bp_rows; a.prior_stride = 0;
  }
  bnw_rows_args(a, pl, r, 1, c.seed);
  a.x = c.x; a.y = c.y; a.v = c.v; a.z = const_cast<float *>(c.z); a.mode = 0; a.stream0 = c.stream_id; a.out = c.out;
  bnw_launch_rows(pl, a, stream);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

int bnw_mh_run(bgm_handle *h, BnnState *s, const bgm_bnn_mh_args &g, hipStream_t stream) {
  int rc = bnw_need(s, "bgm_bnn_mh_run");
  if (rc) return rc;
  BnwRowsArgs a{};
  bnw_nets(s, kGhf, 3, a.m);
  BnwNets mf;
  bnw_nets(s, kF, 1, mf);
  const BnnRows r = bnn_rows(g);
  const int n_blocks = r.n_blocks, q = s->q, n_doses = bnn_effect_doses(g.effect, g.n_doses);
  BnwPlan pl;
  // one buffer: [2 sets per block of g | h | f] then [n_doses sets per block of f]
  const size_t mh_floats = (size_t)2 * n_blocks * a.m.set_floats, eff_floats = (size_t)n_blocks * n_doses * mf.set_floats;
  rc = bnw_plan(h, s, a.m, (long long)((mh_floats + eff_floats) / std::max<long long>(1, a.m.set_floats) + 2), n_blocks * bnw_tiles(r.bs), pl, stream);
  if (rc) return rc;
  if ((rc = bnw_pack(pl.b, a.m, 0, stream)) || (rc = bnw_pack(pl.b, mf, ((size_t)a.m.set_floats + 63) & ~(size_t)63, stream))) return rc;
  bnw_rows_args(a, pl, r, 2, g.seed);
  a.x = g.x_dev; a.y = g.y_dev; a.v = g.v_dev; a.z = g.state_dev; a.mode = 1;
  a.q_sd = g.q_sd; a.q_sd_blocks = g.q_sd_blocks_dev; a.acc_count = g.acc_count_dev;
  BnwBatch bt;
  rc = bnw_batch(s, pl.b, n_blocks, bt, stream);
  if (rc) return rc;
  a.xstats = bt.xstats;
  BnwStatArgs sa = bnw_stat_args(bt, r, q, g.seed);
  sa.z = g.state_dev; sa.q_sd = g.q_sd; sa.q_sd_blocks = g.q_sd_blocks_dev; sa.x = g.x_dev;
  // effects of the draw kept by iteration it_kept; batch statistics: those of the states AFTER its accept step = slot 1 of the
  // statistics pass in front of the next iteration (parity `par`)
  BnwEffects eff = bnw_effects_begin(mf, pl, pl.b->dw + ((mh_floats + 63) & ~(size_t)63), r, g.seed, g.sample_y);
  auto effects = [&](int it_kept, int par) -> int {
    return bnw_effects_of(eff, bnn_effect_slot(g, s->pair_dev, it_kept - g.burn_in), g.state_dev, bt.parity(par), (uint32_t)it_kept, stream);
  };
  for (int i = 0; i < g.n_iters; ++i) {
    const int it = g.it_begin + i;
    bnw_noise(a.m, pl.b->dw, r, 2, g.seed, 2u * (uint32_t)it, stream);
    a.it = it; a.init = (i == 0 && g.init) ? 1 : 0;
    if (bt.on) {
      sa.it = it; sa.init = a.init; sa.par = i & 1; sa.xstats = i == 0 ? bt.xstats : nullptr;
      bnw_stats(sa, stream);
      if (i > 0 && bnn_kept_effect(g, it - 1) && (rc = effects(it - 1, i & 1))) return rc;
      a.stats = bt.parity(i & 1);
    }
    if (s->bp_on) {                     // the two evaluations' own calls of the prior net (streams 2 it, 2 it + 1)
      if ((rc = bprior_rows(h, s, r.n, r.bs, g.block0, g.seed, 2u * (uint32_t)it, 2, stream))) return rc;
      a.prior = s->bp_rows; a.prior_stride = r.n * (long long)(q + 2);
    }
    a.acc_blocks = g.acc_blocks_dev ? g.acc_blocks_dev + (long long)i * n_blocks : nullptr;
    bnw_launch_rows(pl, a, stream);
    if ((rc = bnn_keep_draw(g, bnn_kept(g, it), q, stream))) return rc;
    if (!bt.on && bnn_kept_effect(g, it) && (rc = effects(it, 0))) return rc;
  }
  if (bt.on && g.n_iters > 0 && bnn_kept_effect(g, g.it_begin + g.n_iters - 1)) {      // statistics of the final states: one more pass (its proposals are not used)
    const int i = g.n_iters;
    sa.it = g.it_begin + i; sa.init = 0; sa.par = i & 1; sa.xstats = nullptr;
    bnw_stats(sa, stream);
    if ((rc = effects(g.it_begin + i - 1, i & 1))) return rc;
  }
  BGM_HIP_CHECK(hipGetLastError());
#ifdef BNW_PROF
  {
    unsigned long long acc[8], zero[8] = {0};
    BGM_HIP_CHECK(hipStreamSynchronize(stream));
    BGM_HIP_CHECK(hipMemcpyFromSymbol(acc, HIP_SYMBOL(bnw_prof_acc), sizeof(acc)));
    BGM_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(bnw_prof_acc), zero, sizeof(zero)));
    const double tot = (double)(acc[0] + acc[1] + acc[2]);
    fprintf(stderr, "BNW_PROF net calls: signs %.3f  input normalisation %.3f  layers %.3f  (of %.3e cycles inside calls)\n", acc[0] / tot, acc[1] / tot, acc[2] / tot, tot);
    fprintf(stderr, "BNW_PROF layer products: first fetch %.3f  chunk loops %.3f  epilogues %.3f of the calls' cycles; %.0f cycles per chunk of 16 K, %.0f per epilogue, %.1f chunks per pass\n",
            acc[3] / tot, acc[4] / tot, acc[5] / tot, (double)acc[4] / (double)acc[6], (double)acc[5] / (double)acc[7], (double)acc[6] / (double)acc[7]);
  }
#endif
  return BGM_OK;
}

int bnw_effects(bgm_handle *h, BnnState *s, const BnnEffectsCall &c, hipStream_t stream) {
  int rc = bnw_need(s, "bgm_bnn_effects");
  if (rc) return rc;
  BnwNets mf;
  bnw_nets(s, kF, 1, mf);
  const BnnRows r = bnn_rows(c);
  const int nd = bnn_effect_doses(c.effect, c.n_doses), q = s->q;
  BnwPlan pl;
  rc = bnw_plan(h, s, mf, (long long)r.n_blocks * nd, r.n_blocks * bnw_tiles(r.bs), pl, stream);
  if (rc) return rc;
  if ((rc = bnw_pack(pl.b, mf, 0, stream))) return rc;
  BnwBatch bt;
  rc = bnw_batch(s, pl.b, r.n_blocks, bt, stream);
  if (rc) return rc;
  BnwStatArgs sa = bnw_stat_args(bt, r, q, c.seed);
  BnwEffects eff = bnw_effects_begin(mf, pl, pl.b->dw, r, c.seed, c.sample_y);
  for (int d = 0; d < c.n_keep; ++d) {
    const float *zd = c.draws + (long long)d * c.n * q;
    if (bt.on) { sa.z = zd; sa.it = d; sa.par = d & 1; bnw_stats(sa, stream); }      // statistics of this draw (slot 1)
    if ((rc = bnw_effects_of(eff, bnn_effect_slot(c, s->pair_dev, d), zd, bt.parity(d & 1), (uint32_t)(c.it0 + d), stream))) return rc;
  }
  return BGM_OK;
}

int bnw_evaluate(bgm_handle *h, BnnState *s, const BnnEvalCall &c, hipStream_t stream) {
  int rc = bnw_need(s, "bgm_bnn_evaluate");
  if (rc) return rc;
  BnwRowsArgs a{};
  bnw_nets(s, kGhfe, 4, a.m);
  BnwNets mf;
  bnw_nets(s, kF, 1, mf);
  const long long n = c.n;
  const int nd = c.dose_sums ? c.n_doses : (c.ite ? 2 : 0);
  const BnnRows r = bnn_rows(n, (int)n, 0, 0);        // the whole panel is ONE block (base.py:534-570)
  BnwPlan pl;
  const size_t all_floats = (size_t)a.m.set_floats, eff_floats = (size_t)nd * mf.set_floats;
  rc = bnw_plan(h, s, a.m, (long long)((all_floats + eff_floats) / std::max<long long>(1, a.m.set_floats) + 2), bnw_tiles(r.bs), pl, stream);
  if (rc) return rc;
  if ((rc = bnw_pack(pl.b, a.m, 0, stream)) || (rc = bnw_pack(pl.b, mf, ((size_t)a.m.set_floats + 63) & ~(size_t)63, stream))) return rc;
  bnw_noise(a.m, pl.b->dw, r, 1, c.seed, c.stream_id, stream);
  bnw_rows_args(a, pl, r, 1, c.seed);
  a.x = c.x; a.y = c.y; a.v = c.v; a.z = c.z; a.stream0 = c.stream_id;
  BnwBatch bt;                          // "batch": the whole panel is the batch of every call
  rc = bnw_batch(s, pl.b, 1, bt, stream);
  if (rc) return rc;
  if (c.encode) {
    if (bt.on) {
      hipLaunchKernelGGL(bnw_colstats_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 256), (unsigned)std::min(s->p, 1024)), dim3(256), 0, stream,
                         c.v, n, s->p, bt.vstats);
      a.vstats = bt.vstats;
    }
    a.mode = 3;
    bnw_launch_rows(pl, a, stream);
    a.vstats = nullptr;
  }
  if (bt.on && (c.sums || nd)) {          // statistics of z (slot 1) and of x
    BnwStatArgs sa = bnw_stat_args(bt, r, s->q, c.seed);
    sa.z = c.z; sa.x = c.x; sa.xstats = c.x ? bt.xstats : nullptr;
    bnw_stats(sa, stream);
    a.stats = bt.parity(0); a.xstats = bt.xstats;
  }
  if (c.sums) {
    BGM_HIP_CHECK(hipMemsetAsync(c.sums, 0, 3 * sizeof(double), stream));
    a.mode = 2; a.sums = c.sums;
    bnw_launch_rows(pl, a, stream);
  }
  if (nd) {
    if (c.dose_sums) BGM_HIP_CHECK(hipMemsetAsync(c.dose_sums, 0, sizeof(double) * nd, stream));
    BnwEffects eff = bnw_effects_begin(mf, pl, pl.b->dw + ((all_floats + 63) & ~(size_t)63), r, c.seed, 0);
    const BnnEffectSlot sl{nd, c.dose_sums ? c.x_values : s->pair_dev, c.stream_id + 1u, c.dose_sums, c.dose_sums ? nullptr : c.ite, 1};
    if ((rc = bnw_effects_of(eff, sl, c.z, bt.parity(0), 0u, stream))) return rc;
  }
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
