// bnn_sample_api.hip -- C ABI of the Bayesian-network CausalBGM path: posterior sampling, effects, evaluation.  An entry point checks its
// arguments and hands the call to the family the session's route names (bnn_sample_host.h); bns (bnn_sample_kernels.h) has its host side here.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bgm_host.h"
#include "bnn_sample_kernels.h"
#include "bnn_state.h"

struct BnsPlan {
  BnsNet net[4];
  long long frag_total = 0;      // packed loc / sigma floats (all four nets)
  long long set_ghf = 0;         // floats of one perturbation set [g | h | f]
  long long set_f = 0;           // ... of the outcome net alone
  long long set_all = 0;         // ... [e | g | h | f] (evaluation)
  int lds_bytes = 0;
  int eff_lds_bytes = 0;       // effects kernel: + the second perturbation buffer of its pipelined dose loop
};

// fragment plan of the session's nets; false when a shape is outside the kernels' limits (hidden widths <= 64, inputs <= 208)
static bool bns_plan(const BnnState *s, BnsPlan &pl) {
  long long fb = 0;
  for (int k = 0; k < 4; ++k) {
    BnsNet &n = pl.net[k];
    std::memset(&n, 0, sizeof(n));
    bns_from(s->net[k], n);
    if (n.n_layers < 2 || n.swords > BNS_SW || n.K[0] > BNS_MAXK) return false;
    for (int l = 0; l < n.n_layers - 1; ++l)
      if (n.K[l + 1] > 16 * BNS_MAXT) return false;
    { int bsum = 0; for (int l = 0; l < n.n_layers; ++l) bsum += 16 * n.MT[l]; if (bsum > BNS_MAXB) return false; }
    n.fbase = (int)fb;
    fb += n.foff[n.n_layers];
  }
  pl.frag_total = fb;
  pl.net[BNN_G].dbase = 0;
  pl.net[BNN_H].dbase = pl.net[BNN_G].foff[pl.net[BNN_G].n_layers];
  pl.net[BNN_F].dbase = pl.net[BNN_H].dbase + pl.net[BNN_H].foff[pl.net[BNN_H].n_layers];
  pl.set_ghf = pl.net[BNN_F].dbase + pl.net[BNN_F].foff[pl.net[BNN_F].n_layers];
  pl.net[BNN_E].dbase = (int)pl.set_ghf;     // evaluation sets: [g | h | f | e]
  pl.set_all = pl.set_ghf + pl.net[BNN_E].foff[pl.net[BNN_E].n_layers];
  pl.set_f = pl.net[BNN_F].foff[pl.net[BNN_F].n_layers];
  pl.lds_bytes = (int)sizeof(float) * (2 * BNS_MAXK + BNS_MAXB + BNS_WAVES * BNS_R * 16 * BNS_SW + 2 * BNS_CHUNK * 256);
  pl.eff_lds_bytes = pl.lds_bytes + (int)sizeof(float) * BNS_CHUNK * 256;
  return true;
}

// ---- the route (bnn_sample_host.h)
bool bns_accepts(const BnnState *s) { BnsPlan pl; return bns_plan(s, pl); }
static BnsPlan bns_plan_of(const BnnState *s) { BnsPlan pl; bns_plan(s, pl); return pl; }      // (a bns call: the route has said that the plan exists)
const BnnRoute &bnn_route(BnnState *s) {
  BnnRoute &r = s->route;
  if (r.known) return r;
  r.second = bns_accepts(s) ? BNS : BNW;
  r.primary = bnf_accepts(s) ? BNF : r.second;
  r.known = true;
  return r;
}
int bnn_pair(BnnState *s) {
  const float host[2] = {1.0f, 0.0f};
  if (s->pair_dev) return BGM_OK;
  BGM_HIP_CHECK(hipMalloc((void **)&s->pair_dev, sizeof(host)));
  BGM_HIP_CHECK(hipMemcpy(s->pair_dev, host, sizeof(host), hipMemcpyHostToDevice));
  return BGM_OK;
}

// ---- bns
// effects kernel: the pipelined dose loop when the outcome net's shape allows it (bns_eff_fast_ok), else the generic routine
static auto bns_eff_kernel(const BnsEffArgs &ea) -> void (*)(BnsEffArgs) {
  return bns_eff_default_ok(ea.f) ? bns_effects_kernel<2> : bns_eff_fast_ok(ea.f) ? bns_effects_kernel<1> : bns_effects_kernel<0>;
}
static int bns_set_lds_eff(const BnsPlan &pl) {
  int rc = bgm_set_lds(bns_effects_kernel<2>, pl.eff_lds_bytes);
  if (!rc) rc = bgm_set_lds(bns_effects_kernel<1>, pl.eff_lds_bytes);
  return rc ? rc : bgm_set_lds(bns_effects_kernel<0>, pl.eff_lds_bytes);
}

// Device scratch of the sampling side: [lf | sf | zprop | dw sets | stats (doubles) | xstats (doubles)], grown on demand.
struct BnsBuf { float *lf, *sf, *zprop, *dw; double *stats, *xstats, *vstats; };
static int bns_buffers(BnnState *s, const BnsPlan &pl, const BnnRows &r, long long dw_floats, BnsBuf &b, hipStream_t stream) {
  const long long fr = (pl.frag_total + 63) & ~63LL;
  const long long zp = (r.n * s->q + 63) & ~63LL;
  const long long dwf = (dw_floats + 63) & ~63LL;
  const long long st_d = 2LL * r.n_blocks * 256 + 2LL * r.n_blocks + 2 * BNS_MAXK + 64;      // doubles
  const size_t need = (size_t)(2 * fr + zp + dwf + 2 * st_d + 128);
  if (need > s->samp_cap) s->packed_valid = false;
  int rc = bnn_reserve(s->samp_dev, s->samp_cap, need, stream);
  if (rc || (rc = bnn_pair(s))) return rc;
  b.lf = s->samp_dev; b.sf = b.lf + fr; b.zprop = b.sf + fr; b.dw = b.zprop + zp;
  b.stats = (double *)(b.dw + dwf);
  b.xstats = b.stats + 2LL * r.n_blocks * 256;
  b.vstats = b.xstats + 2LL * r.n_blocks;
  if (!s->packed_valid) {
    BGM_HIP_CHECK(hipMemsetAsync(b.lf, 0, sizeof(float) * 2 * fr, stream));
    BnsPackArgs pa{};
    for (int k = 0; k < 4; ++k) pa.net[k] = pl.net[k];
    pa.theta = s->theta_dev; pa.lf = b.lf; pa.sf = b.sf; pa.n_nets = 4;
    hipLaunchKernelGGL(bns_pack_kernel, dim3(32, 4), dim3(256), 0, stream, pa);
    BGM_HIP_CHECK(hipGetLastError());
    s->packed_valid = true;
  }
  // padding positions of the perturbation sets must be zero: the noise kernel only writes real elements
  BGM_HIP_CHECK(hipMemsetAsync(b.dw, 0, sizeof(float) * dwf, stream));
  BGM_HIP_CHECK(hipMemsetAsync(b.stats, 0, sizeof(double) * st_d, stream));
  return BGM_OK;
}

// the fields a call fixes of its log-posterior / MH launches, statistics passes and effects launches
static BnsMhArgs bns_mh_args(const BnnState *s, const BnsPlan &pl, const BnsBuf &b, const BnnRows &r, uint64_t seed) {
  BnsMhArgs a{};
  for (int k = 0; k < 4; ++k) a.net[k] = pl.net[k];
  a.theta = s->theta_dev; a.q = s->q; a.p = s->p; a.set_floats = pl.set_ghf;
  a.z0 = s->cfg.z_dims[0]; a.z1 = s->cfg.z_dims[1]; a.z2 = s->cfg.z_dims[2]; a.binary = s->cfg.binary_treatment;
  const BnnSig2 sig2 = bnn_sig2(s->cfg);
  a.sig2[0] = sig2.v; a.sig2[1] = sig2.x; a.sig2[2] = sig2.y;
  a.lf = b.lf; a.dw = b.dw; a.xstats = b.xstats; a.zprop = b.zprop;
  a.n = r.n; a.row_base = r.row_base; a.bs = r.bs; a.wg_per_block = (r.bs + BNS_ROWS - 1) / BNS_ROWS; a.block0 = r.block0;
  a.n_items = r.n_blocks * a.wg_per_block;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  return a;
}
static void bns_launch_mh(const BnsPlan &pl, const BnsMhArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(bns_mh_kernel, dim3((a.n_items + 7) & ~7), dim3(BNS_THREADS), pl.lds_bytes, stream, a);
}
static BnsPropArgs bns_prop_args(const BnnState *s, const BnsBuf &b, const BnnRows &r, uint64_t seed) {
  BnsPropArgs pa{};
  pa.zprop = b.zprop; pa.n = r.n; pa.row_base = r.row_base; pa.q = s->q; pa.bs = r.bs; pa.wg_per_block = (r.bs + 255) / 256;
  pa.k0 = (uint32_t)seed; pa.k1 = (uint32_t)(seed >> 32); pa.stats = b.stats; pa.n_blocks = r.n_blocks;
  return pa;
}
static void bns_propose(const BnsPropArgs &pa, hipStream_t stream) {
  hipLaunchKernelGGL(bns_propose_kernel, dim3(pa.n_blocks * pa.wg_per_block), dim3(256), 0, stream, pa);
}
// dw: where the outcome net's sets (one per block and dose) go
static BnsEffArgs bns_eff_args(const BnnState *s, const BnsPlan &pl, const BnsBuf &b, float *dw, const BnnRows &r, uint64_t seed) {
  BnsEffArgs ea{};
  ea.f = pl.net[BNN_F]; ea.f.dbase = 0; ea.sig2_y = bnn_sig2(s->cfg).y;
  ea.theta = s->theta_dev; ea.lf = b.lf; ea.dw = dw; ea.set_floats = pl.set_f;
  ea.n = r.n; ea.row_base = r.row_base; ea.q = s->q; ea.z0 = s->cfg.z_dims[0]; ea.z1 = s->cfg.z_dims[1];
  ea.bs = r.bs; ea.wg_per_block = (r.bs + BNS_ROWS - 1) / BNS_ROWS; ea.block0 = r.block0; ea.n_items = r.n_blocks * ea.wg_per_block;
  ea.k0 = (uint32_t)seed; ea.k1 = (uint32_t)(seed >> 32);
  return ea;
}

// perturbation sets of [g | h | f], with_e: [g | h | f | e], one per block and call; call c draws from stream stream0 + c
static void bns_noise(const BnsPlan &pl, const BnsBuf &b, bool with_e, const BnnRows &r, int n_calls, uint64_t seed, uint32_t stream0,
                      hipStream_t stream) {
  const int ids[4] = {BNN_G, BNN_H, BNN_F, BNN_E};
  BnsNoiseArgs na{};
  na.n_nets = with_e ? 4 : 3;
  for (int i = 0; i < na.n_nets; ++i) na.net[i] = pl.net[ids[i]];
  na.n_calls = n_calls; na.sf = b.sf; na.dw = b.dw; na.set_floats = with_e ? pl.set_all : pl.set_ghf;
  na.k0 = (uint32_t)(seed & 0xFFFFFFFFull); na.k1 = (uint32_t)(seed >> 32); na.stream0 = stream0; na.stream_stride = 1u;
  na.block0 = r.block0;
  hipLaunchKernelGGL(bns_noise_kernel, dim3(8, r.n_blocks * n_calls), dim3(256), 0, stream, na);
}

// effects of ONE draw (states z, their statistics `stats`): the outcome net's sets of the slot's doses, then the effects kernel
static void bns_effects_of(const BnsPlan &pl, const BnsBuf &b, BnsEffArgs &ea, const BnnEffectSlot &sl, const float *z, const double *stats,
                           uint32_t it_noise, hipStream_t stream) {
  BnsNoiseArgs na{};
  na.net[0] = ea.f; na.n_nets = 1; na.n_calls = sl.n_doses; na.sf = b.sf; na.dw = const_cast<float *>(ea.dw); na.set_floats = pl.set_f;
  na.k0 = ea.k0; na.k1 = ea.k1; na.stream0 = sl.stream0; na.stream_stride = 1u; na.block0 = ea.block0;
  hipLaunchKernelGGL(bns_noise_kernel, dim3(2, ea.n_items / ea.wg_per_block * sl.n_doses), dim3(256), 0, stream, na);
  ea.z = z; ea.stats = stats; ea.n_doses = sl.n_doses; ea.xvals = sl.xvals; ea.stream0 = sl.stream0; ea.it_noise = it_noise;
  ea.sum_out = sl.sum_out; ea.sum_stride = sl.stride; ea.ite_out = sl.ite_out; ea.ite_stride = sl.stride;
  hipLaunchKernelGGL(bns_eff_kernel(ea), dim3((ea.n_items + 7) & ~7), dim3(BNS_THREADS), pl.eff_lds_bytes, stream, ea);
}

static int bns_logpost(bgm_handle *h, BnnState *s, const BnnLogpostCall &c, hipStream_t stream) {
  const BnsPlan pl = bns_plan_of(s);
  const BnnRows r = bnn_rows(c.n, c.block_rows, c.block0, 0);
  BnsBuf b;
  int rc = bns_buffers(s, pl, r, (long long)r.n_blocks * pl.set_ghf, b, stream);
  if (rc) return rc;
  bns_noise(pl, b, false, r, 1, c.seed, c.stream_id, stream);
  BnsPropArgs pa = bns_prop_args(s, b, r, c.seed);
  pa.z = c.z; pa.x = c.x; pa.xstats = b.xstats;
  bns_propose(pa, stream);
  BnsMhArgs a = bns_mh_args(s, pl, b, r, c.seed);
  a.stats = b.stats; a.x = c.x; a.y = c.y; a.v = c.v; a.z = const_cast<float *>(c.z); a.mode = 0; a.stream0 = c.stream_id; a.out = c.out;
  if (s->bp_on) {      // conditional prior under batch statistics: one noisy call of the prior net for this evaluation (bprior_api.hip)
    if ((rc = bprior_rows(h, s, c.n, c.block_rows, c.block0, c.seed, c.stream_id, 1, stream))) return rc;
    a.prior = s->bp_rows; a.prior_stride = 0;
  }
  rc = bgm_set_lds(bns_mh_kernel, pl.lds_bytes);
  if (rc) return rc;
  bns_launch_mh(pl, a, stream);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

static int bns_mh_run(bgm_handle *h, BnnState *s, const bgm_bnn_mh_args &g, hipStream_t stream) {
  const BnsPlan pl = bns_plan_of(s);
  const BnnRows r = bnn_rows(g);
  const int n_blocks = r.n_blocks, q = s->q, n_doses = bnn_effect_doses(g.effect, g.n_doses);
  BnsBuf b;
  int rc = bns_buffers(s, pl, r, 2LL * n_blocks * pl.set_ghf + (long long)n_blocks * n_doses * pl.set_f, b, stream);
  if (rc) return rc;
  rc = bgm_set_lds(bns_mh_kernel, pl.lds_bytes);
  if (rc) return rc;
  rc = bns_set_lds_eff(pl);
  if (rc) return rc;
  BnsEffArgs ea = bns_eff_args(s, pl, b, b.dw + 2LL * n_blocks * pl.set_ghf, r, g.seed);
  ea.sample_y = g.sample_y;
  // effects of the draw kept by iteration `it_kept`, whose state statistics sit in slot 1 of parity `par`
  auto effects = [&](int it_kept, int par) {
    bns_effects_of(pl, b, ea, bnn_effect_slot(g, s->pair_dev, it_kept - g.burn_in), g.state_dev, b.stats + (long long)par * n_blocks * 256,
                   (uint32_t)it_kept, stream);
  };
  BnsPropArgs pa = bns_prop_args(s, b, r, g.seed);
  pa.z = g.state_dev; pa.q_sd = g.q_sd; pa.q_sd_blocks = g.q_sd_blocks_dev; pa.x = g.x_dev; pa.z_init = g.state_dev;
  BnsMhArgs a = bns_mh_args(s, pl, b, r, g.seed);
  a.x = g.x_dev; a.y = g.y_dev; a.v = g.v_dev; a.z = g.state_dev; a.mode = 1; a.acc_count = g.acc_count_dev;
#ifdef BNS_PROF
  static unsigned long long *prof_dev = nullptr;
  if (!prof_dev) hipMalloc((void **)&prof_dev, 128);
  hipMemsetAsync(prof_dev, 0, 128, stream);
  a.prof = prof_dev;
  ea.prof = prof_dev + 8;
#endif
  for (int i = 0; i < g.n_iters; ++i) {
    const int it = g.it_begin + i;
    bns_noise(pl, b, false, r, 2, g.seed, 2u * (uint32_t)it, stream);
    pa.it = it; pa.par = i & 1; pa.init = (i == 0 && g.init) ? 1 : 0; pa.xstats = (i == 0) ? b.xstats : nullptr;
    bns_propose(pa, stream);
    if (i > 0 && bnn_kept_effect(g, it - 1)) effects(it - 1, i & 1);
    if (s->bp_on) {      // the two evaluations' own calls of the prior net (streams 2 it, 2 it + 1)
      if ((rc = bprior_rows(h, s, r.n, r.bs, g.block0, g.seed, 2u * (uint32_t)it, 2, stream))) return rc;
      a.prior = s->bp_rows; a.prior_stride = r.n * (long long)(q + 2);
    }
    a.it = it; a.stats = b.stats + (long long)(i & 1) * n_blocks * 256;
    a.acc_blocks = g.acc_blocks_dev ? g.acc_blocks_dev + (long long)i * n_blocks : nullptr;
    bns_launch_mh(pl, a, stream);
    if ((rc = bnn_keep_draw(g, bnn_kept(g, it), q, stream))) return rc;
  }
#ifdef BNS_PROF
  {
    unsigned long long hp[6];
    hipStreamSynchronize(stream);
    hipMemcpy(hp, prof_dev, sizeof(hp), hipMemcpyDeviceToHost);
    const double wgs = (double)n_blocks * a.wg_per_block * std::max(1, g.n_iters);
    int occ = -1;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, bns_mh_kernel, BNS_THREADS, pl.lds_bytes);
    fprintf(stderr, "[BNS_PROF] occupancy %d workgroups / CU (lds %d B)\n", occ, pl.lds_bytes);
    unsigned long long he[6];
    hipMemcpy(he, prof_dev + 8, sizeof(he), hipMemcpyDeviceToHost);
    if (g.effect) fprintf(stderr, "[BNS_PROF] effects, cycles per workgroup-launch: prologue %.0f staging %.0f first %.0f middle %.0f last %.0f outside %.0f\n",
            he[0] / wgs, he[1] / wgs, he[2] / wgs, he[3] / wgs, he[4] / wgs, he[5] / wgs);
    fprintf(stderr, "[BNS_PROF] cycles per workgroup-iteration (wave 0): prologue %.0f staging %.0f first %.0f middle %.0f last %.0f outside %.0f\n",
            hp[0] / wgs, hp[1] / wgs, hp[2] / wgs, hp[3] / wgs, hp[4] / wgs, hp[5] / wgs);
  }
#endif
  if (g.n_iters > 0 && bnn_kept_effect(g, g.it_begin + g.n_iters - 1)) {
    // statistics of the final state: one more statistics pass (its proposal is not used)
    const int i = g.n_iters;
    pa.it = g.it_begin + i; pa.par = i & 1; pa.init = 0; pa.xstats = nullptr;
    bns_propose(pa, stream);
    effects(g.it_begin + i - 1, i & 1);
  }
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

static int bns_evaluate(bgm_handle *, BnnState *s, const BnnEvalCall &c, hipStream_t stream) {
  const BnsPlan pl = bns_plan_of(s);
  const long long n = c.n;
  const int nd = c.dose_sums ? c.n_doses : (c.ite ? 2 : 0);
  const BnnRows r = bnn_rows(n, (int)n, 0, 0);      // the whole panel is ONE block
  BnsBuf b;
  int rc = bns_buffers(s, pl, r, pl.set_all + (long long)nd * pl.set_f, b, stream);
  if (rc) return rc;
  rc = bgm_set_lds(bns_eval_kernel, pl.lds_bytes);
  if (rc) return rc;
  rc = bns_set_lds_eff(pl);
  if (rc) return rc;
  bns_noise(pl, b, true, r, 1, c.seed, c.stream_id, stream);
  BnsEvalArgs ev{};
  for (int k = 0; k < 4; ++k) ev.net[k] = pl.net[k];
  ev.theta = s->theta_dev; ev.lf = b.lf; ev.dw = b.dw; ev.stats = b.stats; ev.xstats = b.xstats; ev.vstats = b.vstats;
  ev.x = c.x; ev.y = c.y; ev.v = c.v; ev.z = c.z; ev.n = n; ev.q = s->q; ev.p = s->p;
  ev.z0 = s->cfg.z_dims[0]; ev.z1 = s->cfg.z_dims[1]; ev.z2 = s->cfg.z_dims[2]; ev.binary = s->cfg.binary_treatment;
  ev.k0 = (uint32_t)c.seed; ev.k1 = (uint32_t)(c.seed >> 32); ev.stream = c.stream_id; ev.sums = c.sums;
  const int wgs = (int)((n + BNS_ROWS - 1) / BNS_ROWS);
  if (c.encode) {
    hipLaunchKernelGGL(bns_colstats_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 256), s->p), dim3(256), 0, stream, c.v, n,
                       s->p, b.vstats);
    ev.mode = 0;
    hipLaunchKernelGGL(bns_eval_kernel, dim3(wgs), dim3(BNS_THREADS), pl.lds_bytes, stream, ev);
  }
  if (c.sums || nd) {
    // statistics of z (slot 1) and of x
    BnsPropArgs pa = bns_prop_args(s, b, r, c.seed);
    pa.z = c.z; pa.x = c.x; pa.xstats = c.x ? b.xstats : nullptr;
    bns_propose(pa, stream);
  }
  if (c.sums) {
    BGM_HIP_CHECK(hipMemsetAsync(c.sums, 0, 3 * sizeof(double), stream));
    ev.mode = 1;
    hipLaunchKernelGGL(bns_eval_kernel, dim3(wgs), dim3(BNS_THREADS), pl.lds_bytes, stream, ev);
  }
  if (nd) {
    if (c.dose_sums) BGM_HIP_CHECK(hipMemsetAsync(c.dose_sums, 0, sizeof(double) * nd, stream));
    BnsEffArgs ea = bns_eff_args(s, pl, b, b.dw + pl.set_all, r, c.seed);
    const BnnEffectSlot sl{nd, c.dose_sums ? c.x_values : s->pair_dev, c.stream_id + 1u, c.dose_sums, c.dose_sums ? nullptr : c.ite, 1};
    bns_effects_of(pl, b, ea, sl, c.z, b.stats, 0u, stream);
  }
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

static int bns_effects(bgm_handle *, BnnState *s, const BnnEffectsCall &c, hipStream_t stream) {
  const BnsPlan pl = bns_plan_of(s);
  const BnnRows r = bnn_rows(c);
  BnsBuf b;
  int rc = bns_buffers(s, pl, r, (long long)r.n_blocks * bnn_effect_doses(c.effect, c.n_doses) * pl.set_f, b, stream);
  if (rc) return rc;
  rc = bns_set_lds_eff(pl);
  if (rc) return rc;
  BnsEffArgs ea = bns_eff_args(s, pl, b, b.dw, r, c.seed);
  ea.sample_y = c.sample_y;
  BnsPropArgs pa = bns_prop_args(s, b, r, c.seed);
  for (int d = 0; d < c.n_keep; ++d) {
    const float *z = c.draws + (long long)d * c.n * s->q;
    pa.z = z; pa.it = d; pa.par = d & 1;                      // statistics of this draw (slot 1 of parity d & 1)
    bns_propose(pa, stream);
    bns_effects_of(pl, b, ea, bnn_effect_slot(c, s->pair_dev, d), z, b.stats + (long long)(d & 1) * r.n_blocks * 256, (uint32_t)(c.it0 + d), stream);
  }
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

// ---- the entry points: argument checks, the family of the call, done
static int bnn_enter(bgm_handle *h, const char *who, BnnState *&s) {
  if (!h || !h->bnn_state) { bgm_set_error(std::string(who) + ": no session (bgm_bnn_begin)"); return BGM_E_STATE; }
  s = static_cast<BnnState *>(h->bnn_state);
  return BGM_OK;
}

extern "C" int bgm_bnn_sampling_family(bgm_handle *h, int32_t *family) {
  BnnState *s;
  int rc = bnn_enter(h, "bgm_bnn_sampling_family", s);
  if (rc) return rc;
  if (!family) { bgm_set_error("bgm_bnn_sampling_family: bad argument"); return BGM_E_INVALID; }
  *family = (int32_t)bnn_route(s).primary;
  return BGM_OK;
}

extern "C" int bgm_bnn_logpost(bgm_handle *h, const float *x, const float *y, const float *v, const float *z, int64_t n,
                               int32_t block_rows, int32_t block0, uint64_t seed, uint32_t stream_id, float *out, void *stream_) {
  BnnState *s;
  int rc = bnn_enter(h, "bgm_bnn_logpost", s);
  if (rc) return rc;
  if (!x || !y || !v || !z || !out || n < 1 || block_rows < 2) { bgm_set_error("bgm_bnn_logpost: bad argument"); return BGM_E_INVALID; }
  const BnnLogpostCall c{x, y, v, z, n, block_rows, block0, seed, stream_id, out};
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  const BnnFamily family = bnn_family_for(s, c);
  return family == BNF ? bnf_logpost(h, s, c, stream) : family == BNS ? bns_logpost(h, s, c, stream) : bnw_logpost(h, s, c, stream);
}

extern "C" int bgm_bnn_mh_run(bgm_handle *h, const bgm_bnn_mh_args *g, void *stream_) {
  BnnState *s;
  if (h && h->ra_scale) { bgm_set_error("bgm_bnn_mh_run: the per-chain proposal scale (bgm_causal_set_row_scale) does not exist for the Bayesian networks"); return BGM_E_UNSUPPORTED; }
  int rc = bnn_enter(h, "bgm_bnn_mh_run", s);
  if (rc) return rc;
  if (!g || !g->x_dev || !g->y_dev || !g->v_dev || !g->state_dev || g->n < 1 || g->block_rows < 2 || g->n_iters < 0) {
    bgm_set_error("bgm_bnn_mh_run: bad argument"); return BGM_E_INVALID;
  }
  if (g->effect == 1 && (!g->x_values_dev || g->n_doses < 1 || !g->adrf_sum_dev)) { bgm_set_error("bgm_bnn_mh_run: ADRF needs x_values_dev and adrf_sum_dev"); return BGM_E_INVALID; }
  if (g->effect == 2 && !g->ite_dev) { bgm_set_error("bgm_bnn_mh_run: ITE needs ite_dev"); return BGM_E_INVALID; }
  if (g->effect < 0 || g->effect > 2) { bgm_set_error("bgm_bnn_mh_run: bad effect"); return BGM_E_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  const BnnFamily family = bnn_family_for(s, *g);
  if (family == BNF) return bnf_mh_run(h, s, *g, stream);      // (checks that block_row0 lies inside the block)
  if (g->block_row0 != 0) { bgm_set_error("bgm_bnn_mh_run: a share of one block (block_row0 > 0) is served by the default-shape sampling kernels with inference-mode normalisation only"); return BGM_E_UNSUPPORTED; }
  return family == BNS ? bns_mh_run(h, s, *g, stream) : bnw_mh_run(h, s, *g, stream);
}

extern "C" int bgm_bnn_evaluate(bgm_handle *h, const float *x, const float *y, const float *v, float *z, int32_t encode, int64_t n,
                                const float *x_values, int32_t n_doses, uint64_t seed, uint32_t stream_id, double *sums,
                                double *dose_sums, float *ite, void *stream_) {
  BnnState *s;
  int rc = bnn_enter(h, "bgm_bnn_evaluate", s);
  if (rc) return rc;
  if (!v || !z || n < 2 || n > 0x7FFFFFFFLL) { bgm_set_error("bgm_bnn_evaluate: bad argument"); return BGM_E_INVALID; }
  if (sums && (!x || !y)) { bgm_set_error("bgm_bnn_evaluate: x_dev, y_dev required"); return BGM_E_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  if (dose_sums && (!x_values || n_doses < 1)) { bgm_set_error("bgm_bnn_evaluate: dose grid missing"); return BGM_E_INVALID; }
  const BnnEvalCall c{x, y, v, z, encode, n, x_values, n_doses, seed, stream_id, sums, dose_sums, ite};
  return bnn_family_for(s, c) == BNS ? bns_evaluate(h, s, c, stream) : bnw_evaluate(h, s, c, stream);
}

extern "C" int bgm_bnn_effects(bgm_handle *h, const float *draws, int64_t n, int32_t block_rows, int32_t block0, int64_t row_base,
                               int32_t n_keep, int32_t it0, uint64_t seed, int32_t effect, int32_t sample_y, const float *x_values,
                               int32_t n_doses, double *adrf_sum, float *ite, void *stream_) {
  BnnState *s;
  int rc = bnn_enter(h, "bgm_bnn_effects", s);
  if (rc) return rc;
  if (!draws || n < 1 || block_rows < 2 || n_keep < 1 || (effect != 1 && effect != 2)) { bgm_set_error("bgm_bnn_effects: bad argument"); return BGM_E_INVALID; }
  if (effect == 1 && (!x_values || n_doses < 1 || !adrf_sum)) { bgm_set_error("bgm_bnn_effects: ADRF needs x_values_dev and adrf_sum_dev"); return BGM_E_INVALID; }
  if (effect == 2 && !ite) { bgm_set_error("bgm_bnn_effects: ITE needs ite_dev"); return BGM_E_INVALID; }
  const BnnEffectsCall c{draws, n, block_rows, block0, row_base, n_keep, it0, seed, effect, sample_y, x_values, n_doses, adrf_sum, ite};
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  const BnnFamily family = bnn_family_for(s, c);
  return family == BNF ? bnf_effects(h, s, c, stream) : family == BNS ? bns_effects(h, s, c, stream) : bnw_effects(h, s, c, stream);
}
