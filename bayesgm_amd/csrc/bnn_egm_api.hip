// bnn_egm_api.hip -- C ABI of the EGM warm start with Bayesian networks (a sub-session of bgm_bnn_begin).
#include <algorithm>
#include <cstring>
#include <vector>

#include "bgm_host.h"
#include "bnn_egm_kernels.h"
#include "bnn_state.h"
#include "egm_host.h"

static BnnState *bst(bgm_handle *h) { return static_cast<BnnState *>(h->bnn_state); }

struct BnnEgmState {
  bgm_egm_config cfg{};
  BnnEgmArgs base{};
  EgmCore core;              // side 0: the Bayesian nets' parameters (the sub-session's own Adam slots), side 1: the discriminator
  BnnEgmPlan plan{};         // which kernels the two steps run, decided by bgm_bnn_egm_begin (egm_plan.h)
  size_t n_dz = 0, ws_floats = 0;
  float *dev = nullptr;      // m | v (EGM Adam slots of the Bayesian nets) | theta_d | m_d | v_d | grad_d | ws
  int n_tiles = 0;           // gradient tiles of the generator chain (egm_chain_bnn.h)
  EcbCall disc_call{};       // noise of the discriminator step's encoder call (workspace offsets)
  EcbTab *tab_dev = nullptr;
  int *tiles_dev = nullptr;
  float *thetaT_dev = nullptr;
};

void bgm_bnn_egm_free(void *p) {
  BnnEgmState *e = static_cast<BnnEgmState *>(p);
  if (!e) return;
  if (e->dev) hipFree(e->dev);
  if (e->tab_dev) hipFree(e->tab_dev);
  if (e->tiles_dev) hipFree(e->tiles_dev);
  if (e->thetaT_dev) hipFree(e->thetaT_dev);
  delete e;
}

extern "C" int bgm_bnn_egm_begin(bgm_handle *h, const bgm_egm_config *cfg, const float *theta_dz_host, int64_t count, void *stream_) {
  (void)stream_;
  if (!h || !h->bnn_state) { bgm_set_error("bgm_bnn_egm_begin: no session (bgm_bnn_begin)"); return BGM_E_STATE; }
  if (!cfg || !theta_dz_host) { bgm_set_error("bgm_bnn_egm_begin: NULL argument"); return BGM_E_INVALID; }
  BnnState *s = bst(h);
  if (cfg->batch_size < 2 || cfg->batch_size > s->cfg.max_batch) { bgm_set_error("bgm_bnn_egm_begin: batch_size outside [2, max_batch]"); return BGM_E_INVALID; }
  if (cfg->n_hidden_dz < 1 || cfg->n_hidden_dz + 1 > EGM_MAX_LAYERS) { bgm_set_error("bgm_bnn_egm_begin: bad dz_units"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  bgm_bnn_egm_free(s->egm); s->egm = nullptr;
  BnnEgmState *e = new BnnEgmState();
  s->egm = e;
  e->cfg = *cfg;
  BnnEgmArgs &a = e->base;
  for (int k = 0; k < 4; ++k) a.net[k] = s->net[k];
  EgmDisc &d = a.dz;
  const int L = cfg->n_hidden_dz, o = egm_fill_disc(d, s->q, L, cfg->dz_units);
  d.fixed_norm = h->disc_norm;
  e->n_dz = (size_t)o;
  if ((int64_t)o != count) {
    bgm_bnn_egm_free(e); s->egm = nullptr;
    bgm_set_error("bgm_bnn_egm_begin: expected " + std::to_string(o) + " discriminator parameters, got " + std::to_string(count));
    return BGM_E_INVALID;
  }
  const int B = cfg->batch_size;
  int wmax = s->wmax;
  for (int l = 0; l <= L; ++l) wmax = std::max(wmax, d.dims[l]);
  a.wmax = wmax;
  const bool t2 = chain_extent(s->q, s->p).t0 == 2;
  e->plan = bnn_egm_plan({s->q, s->p, B, d.fixed_norm != 0, L, d.dims, ecb_dims(s->net[BNN_G]), ecb_dims(s->net[BNN_E]), ecb_dims(s->net[BNN_F]),
                          ecb_dims(s->net[BNN_H])}, egm_switches_now(), bnn_step_one_launch(),
                         sizeof(float) * (size_t)(t2 ? ech_disc_lds_floats<4, 2, 1, 2>(d, B) : ech_disc_lds_floats<4, 2, 1>(d, B)),
                         sizeof(float) * (size_t)(t2 ? ecb_lds_floats<4, 2, 1, 2>(d, B) : ecb_lds_floats<4, 2, 1>(d, B)));
  const EgmArena &arena = e->plan.arena;
  a.dmax = arena.dmax;
  a.disc_lds = arena.in_lds ? 1 : 0;
  a.n_gen = s->n_params; a.B = B; a.q = s->q; a.p = s->p;
  a.z0 = s->cfg.z_dims[0]; a.z1 = s->cfg.z_dims[1]; a.z2 = s->cfg.z_dims[2];
  a.binary = s->cfg.binary_treatment; a.use_z_rec = cfg->use_z_rec;
  // workspace: nine Flipout call caches (g x 3, e x 2, f x 2, h x 2) + discriminator caches + scratch rows
  auto cache_floats = [&](const BnnNet &n) {
    return (size_t)B * n.dims[0] + n.dims[0] + 2 * (size_t)B * n.hoff[n.n_layers + 1] + 2 * (size_t)n.eoff[n.n_layers] + (size_t)B * n.swords + 64;
  };
  size_t gen_ws = 0;
  EcbTab tab{};
  std::vector<int> tiles;
  if (e->plan.chain_gen_lds > 0) {      // the generator step as row-tile chains: its nine calls' stashes and the gradient tiles
    const int call_net[ECB_CALLS] = {BNN_G, BNN_G, BNN_E, BNN_E, BNN_G, BNN_F, BNN_F, BNN_H, BNN_H};
    const int call_soff[ECB_CALLS] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    const int all_nets[4] = {BNN_G, BNN_E, BNN_F, BNN_H};
    gen_ws = ecb_build_tab(s->net, call_net, call_soff, ECB_CALLS, B, e->plan.ext.ntl, tab, tiles, all_nets, 4);
    tab.n_warm = s->n_params;
    e->n_tiles = tab.n_tiles;
  }
  {   // noise block of the discriminator step's encoder call, behind the generator chain's region
    const BnnNet &E = s->net[BNN_E];
    size_t off = (gen_ws + 3) / 4 * 4;
    e->disc_call.net = BNN_E;
    e->disc_call.dW = (int)off; off += ((size_t)E.eoff[E.n_layers] + 16 + 3) / 4 * 4;
    e->disc_call.sg = (int)off; off += ((size_t)B * E.swords + 3) / 4 * 4;
    e->disc_call.xh = (int)off; off += (size_t)B * EchDims<4, 2, 1, 2>::SW;      // two latent tiles: the tail's fourth stash (EchDiscIo::gstash)
    gen_ws = off;
  }
  size_t keep = 0;      // the kept upstream gradients of the nine calls (wide generator step: G / GS of bnn_bwd)
  for (int k : {BNN_G, BNN_G, BNN_G, BNN_E, BNN_E, BNN_F, BNN_F, BNN_H, BNN_H}) keep += 2 * ((size_t)B * s->net[k].hoff[s->net[k].n_layers + 1] + 4);
  e->ws_floats = keep + gen_ws + 3 * cache_floats(s->net[BNN_G]) + 2 * cache_floats(s->net[BNN_E]) + 2 * cache_floats(s->net[BNN_F]) +
                 2 * cache_floats(s->net[BNN_H]) + (size_t)B * (4 * (size_t)s->p + 32 * (size_t)wmax + 256) + 4 * arena.cache + e->n_dz + arena.floats + 8192;
  const size_t np = ((size_t)s->n_params + 63) & ~(size_t)63, nd = (e->n_dz + 63) & ~(size_t)63;
  const size_t total = 2 * np + 4 * nd + e->ws_floats + 64;
  BGM_HIP_CHECK(hipMalloc((void **)&e->dev, total * sizeof(float)));
  BGM_HIP_CHECK(hipMemset(e->dev, 0, total * sizeof(float)));
  a.theta = s->theta_dev; a.grad = s->grad_dev;
  BGM_HIP_CHECK(hipMemset(s->grad_dev, 0, sizeof(float) * (size_t)s->n_params));   // entries no step writes stay zero (bgm_bnn_egm_apply runs Adam over all of them)
  a.m = e->dev; a.v = e->dev + np;
  a.theta_d = e->dev + 2 * np; a.m_d = a.theta_d + nd; a.v_d = a.m_d + nd; a.grad_d = a.v_d + nd;
  a.ws = a.grad_d + nd;
  e->core.set_adam(cfg->lr, BNN_ADAM_B1, BNN_ADAM_B2, BNN_ADAM_EPS);
  e->core.set_side(0, a.theta, a.m, a.v, a.grad, (size_t)s->n_params);
  e->core.set_side(1, a.theta_d, a.m_d, a.v_d, a.grad_d, e->n_dz);
  BGM_HIP_CHECK(hipMemcpy(a.theta_d, theta_dz_host, e->n_dz * sizeof(float), hipMemcpyHostToDevice));
  if (e->plan.chain_gen_lds > 0) {
    // (no transposed mirror: the backward products read the canonical arrays K-contiguously, egm_chain_gen.h)
    BGM_HIP_CHECK(hipMalloc((void **)&e->tab_dev, sizeof(EcbTab)));
    BGM_HIP_CHECK(hipMemcpy(e->tab_dev, &tab, sizeof(EcbTab), hipMemcpyHostToDevice));
    BGM_HIP_CHECK(hipMalloc((void **)&e->tiles_dev, sizeof(int) * tiles.size()));
    BGM_HIP_CHECK(hipMemcpy(e->tiles_dev, tiles.data(), sizeof(int) * tiles.size(), hipMemcpyHostToDevice));
  }
  return BGM_OK;
}

static int bnn_egm_need(bgm_handle *h, const char *who, BnnState *&s, BnnEgmState *&e) {
  if (!h || !h->bnn_state || !bst(h)->egm) { bgm_set_error(std::string(who) + ": call bgm_bnn_egm_begin first"); return BGM_E_STATE; }
  s = bst(h);
  e = static_cast<BnnEgmState *>(s->egm);
  return BGM_OK;
}

// ---- the kernels of the discriminator routes (egm_plan.h), rows in the order of the enum -- the order this unit has always
// instantiated them in (it moves the register allocation of some: scripts/compare_code_objects.py after any change here)
using BnnEgmDiscFn = void (*)(BnnEgmArgs, EcbCall);
static BnnEgmDiscFn bnn_egm_disc_chain_kernel_of(BnnEgmDiscRoute r) {
  static const BnnEgmDiscFn k[] = {bnn_egm_disc_chain_kernel<13, 4, 2, 1, 2, 2>, bnn_egm_disc_chain_kernel<0, 4, 2, 1, 2, 2>,                                   // T2
                                   bnn_egm_disc_chain_kernel<13, 4, 2, 1, 2>, bnn_egm_disc_chain_kernel<7, 4, 2, 1, 2>, bnn_egm_disc_chain_kernel<0, 4, 2, 1, 2>,     // B32
                                   bnn_egm_disc_chain_kernel<13, 4, 2, 1, 1>, bnn_egm_disc_chain_kernel<7, 4, 2, 1, 1>, bnn_egm_disc_chain_kernel<0, 4, 2, 1, 1>};    // B16
  return k[(int)r];
}

extern "C" int bgm_bnn_egm_disc_step(bgm_handle *h, const float *z_dev, const int32_t *idx_dev, const float *v_dev, float eps,
                                     uint64_t seed, uint32_t stream_id, int32_t apply, float *out_dev, void *stream_) {
  BnnState *s; BnnEgmState *e;
  int rc = bnn_egm_need(h, "bgm_bnn_egm_disc_step", s, e);
  if (rc) return rc;
  if (!z_dev || !idx_dev || !v_dev) { bgm_set_error("bgm_bnn_egm_disc_step: NULL pointer"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  const hipStream_t stream = (hipStream_t)stream_;
  BnnEgmArgs a = e->base;
  a.z = z_dev; a.idx = idx_dev; a.v_ = v_dev; a.eps = eps; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.stream = stream_id;
  a.adam = e->core.adam(1, apply != 0);
  const BnnEgmPlan &pl = e->plan;
  const bool wg = pl.disc == BnnEgmDiscRoute::WG;
  // the encoder call's noise: in front of an encoder chain its own launch; the general encoder's eps / dW over the chip
  if (bnn_egm_disc_has_enc_chain(pl.disc)) {
    hipLaunchKernelGGL(bnn_egm_disc_noise_kernel, dim3(ECB_NOISE_PARTS), dim3(EGM_THREADS), 0, stream, a, e->disc_call);
    BGM_HIP_CHECK(hipGetLastError());
  } else if (pl.wide) {
    a.wide = 1;
    hipLaunchKernelGGL(bnn_egm_disc_noise_wide_kernel, dim3(16), dim3(EGM_THREADS), 0, stream, a, wg ? 1 : 0);
  }
  if (wg) return bgm_launch(bnn_egm_disc_step_kernel, 1, EGM_WAVES, pl.arena.lds_bytes, stream, a);
  return bgm_launch(bnn_egm_disc_chain_kernel_of(pl.disc), 1, EGM_WAVES, pl.chain_disc_lds, stream, a, e->disc_call);
}

// the generator chain's instantiations live in bnn_egm_gen_chain_{a,b,c,d}.hip (compile time); rows in the order of BnnEgmGenRoute
using BnnEgmGenChainLaunch = int(const BnnEgmArgs &a, int nb, int lds, const EcbTab *tab, float *thetaT, hipStream_t stream);
BnnEgmGenChainLaunch bnn_egm_gen_chain_launch_a, bnn_egm_gen_chain_launch_b, bnn_egm_gen_chain_launch_c, bnn_egm_gen_chain_launch_d;
static BnnEgmGenChainLaunch *const bnn_egm_gen_chain_launch[] = {bnn_egm_gen_chain_launch_d, bnn_egm_gen_chain_launch_c,      // CHAIN_T2, CHAIN_PAD
                                                                bnn_egm_gen_chain_launch_a, bnn_egm_gen_chain_launch_b};     // CHAIN_N13, CHAIN_N7

extern "C" int bgm_bnn_egm_gen_step(bgm_handle *h, const float *z_dev, const int32_t *idx_dev, const float *v_dev, const float *x_dev,
                                    const float *y_dev, uint64_t seed, uint32_t stream_id, int32_t apply, float *out_dev, void *stream_) {
  BnnState *s; BnnEgmState *e;
  int rc = bnn_egm_need(h, "bgm_bnn_egm_gen_step", s, e);
  if (rc) return rc;
  if (!z_dev || !idx_dev || !v_dev || !x_dev || !y_dev) { bgm_set_error("bgm_bnn_egm_gen_step: NULL pointer"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  const hipStream_t stream = (hipStream_t)stream_;
  BnnEgmArgs a = e->base;
  a.z = z_dev; a.idx = idx_dev; a.v_ = v_dev; a.x_ = x_dev; a.y_ = y_dev; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.stream = stream_id;
  a.adam = e->core.adam(0, apply != 0);
  if (apply) { s->packed_valid = false; s->bnf_valid = false; }
  const BnnEgmPlan &pl = e->plan;
  if (pl.gen != BnnEgmGenRoute::STEP) {      // the nine calls' noise, the chains, the gradient tiles (and Adam)
    hipLaunchKernelGGL(bnn_egm_gen_noise_kernel, dim3(ECB_CALLS * ECB_NOISE_PARTS), dim3(EGM_THREADS), 0, stream, a, e->tab_dev);
    BGM_HIP_CHECK(hipGetLastError());
    if ((rc = bnn_egm_gen_chain_launch[(int)pl.gen](a, a.B / 16, pl.chain_gen_lds, e->tab_dev, e->thetaT_dev, stream))) return rc;
    hipLaunchKernelGGL(a.B == 32 ? bnn_egm_gen_dw_kernel<2> : bnn_egm_gen_dw_kernel<1>, dim3((e->n_tiles + ECH_WAVES - 1) / ECH_WAVES + 1), dim3(EGM_THREADS), 0,
                       stream, a, e->tab_dev, e->tiles_dev, e->thetaT_dev);
    BGM_HIP_CHECK(hipGetLastError());
    return BGM_OK;
  }
  // general widths: one workgroup walks the nine calls and their backward passes; the calls' eps / dW and the Adam step (elementwise over
  // all parameters of g, e, f, h) run as launches over the chip around it.  BGM_BNN_STEP_ONE_LAUNCH: everything inside the one workgroup.
  a.wide = pl.wide ? 1 : 0;
  if (a.wide) hipLaunchKernelGGL(bnn_egm_gen_noise_wide_kernel, dim3(16, 9), dim3(EGM_THREADS), 0, stream, a);
  hipLaunchKernelGGL(bnn_egm_gen_step_kernel, dim3(1), dim3(EGM_THREADS), 64 * (int)sizeof(float), stream, a);
  if (a.wide) hipLaunchKernelGGL(bnn_egm_gen_dw_wide_kernel, dim3(16, 4), dim3(EGM_THREADS), 0, stream, a);      // the gradient tiles of all layers
  if (a.wide && a.apply)
    hipLaunchKernelGGL(egm_dp_adam_kernel, dim3((unsigned)((a.n_gen + 255) / 256)), dim3(256), 0, stream, a.theta, a.m, a.v, a.grad, a.n_gen, a.adam,
                       (float *)nullptr, (const int *)nullptr);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

extern "C" int bgm_bnn_egm_set_share(bgm_handle *h, int32_t row0) {
  BnnState *s; BnnEgmState *e;
  int rc = bnn_egm_need(h, "bgm_bnn_egm_set_share", s, e);
  if (rc) return rc;
  if (row0 < 0) { bgm_set_error("bgm_bnn_egm_set_share: row0 < 0"); return BGM_E_INVALID; }
  e->base.row0 = (uint32_t)row0;
  return BGM_OK;
}

extern "C" int bgm_bnn_egm_grad(bgm_handle *h, int32_t which, float scale, float *grad_dev, int64_t count, void *stream_) {
  BnnState *s; BnnEgmState *e;
  int rc = bnn_egm_need(h, "bgm_bnn_egm_grad", s, e);
  if (rc) return rc;
  return egm_grad(e->core, h->device, "bgm_bnn_egm_grad", which, scale, grad_dev, count, (hipStream_t)stream_);
}

extern "C" int bgm_bnn_egm_apply(bgm_handle *h, int32_t which, const float *grad_dev, int64_t count, void *stream_) {
  BnnState *s; BnnEgmState *e;
  int rc = bnn_egm_need(h, "bgm_bnn_egm_apply", s, e);
  if (rc) return rc;
  rc = egm_apply(e->core, h->device, "bgm_bnn_egm_apply", which, grad_dev, count, (hipStream_t)stream_);
  if (which == 0 && rc != BGM_E_INVALID) { s->packed_valid = false; s->bnf_valid = false; }      // the nets moved: their packed copies are stale
  return rc;
}

extern "C" int bgm_bnn_egm_read(bgm_handle *h, int32_t what, float *host, int64_t count, void *stream_) {
  BnnState *s; BnnEgmState *e;
  int rc = bnn_egm_need(h, "bgm_bnn_egm_read", s, e);
  if (rc) return rc;
  if ((what != 1 && what != 3) || !host || (size_t)count != e->n_dz) { bgm_set_error("bgm_bnn_egm_read: what must be 1 (parameters) or 3 (gradient) of the discriminator"); return BGM_E_INVALID; }
  return egm_read(e->core, h->device, "bgm_bnn_egm_read", "bgm_bnn_egm_read", what, host, count, (hipStream_t)stream_);
}

extern "C" int bgm_bnn_egm_end(bgm_handle *h, void *stream_) {
  if (!h || !h->bnn_state) return BGM_OK;
  BnnState *s = bst(h);
  if (!s->egm) return BGM_OK;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BGM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
  bgm_bnn_egm_free(s->egm);
  s->egm = nullptr;
  return BGM_OK;
}
