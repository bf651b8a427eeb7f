// egm_api.hip -- C-ABI entry points of the CausalBGM EGM warm start (include/bgm_hip.h, EGM section).
#include <algorithm>
#include <cstring>
#include <vector>

#include "bgm_host.h"
#include "egm_kernels.h"
#include "egm_chain.h"
#include "egm_chain_gen.h"
#include "egm_host.h"

static constexpr float EGM_B1 = 0.9f, EGM_B2 = 0.99f, EGM_ADAM_EPS = 1e-7f;   // causalbgm/base.py:86-87, Keras epsilon

struct EgmState {
  bgm_egm_config cfg{};
  EgmArgs base{};              // network descriptions + device pointers shared by both kernels
  EgmCore core;
  EgmPlan plan{};              // which kernel each step runs, decided by bgm_causal_egm_begin (egm_plan.h)
  size_t n_gen = 0, n_dz = 0, ws_floats = 0;
  EcgTab gen_tab{};            // the generator chain's stashes and gradient tiles
  float *thetaT_dev = nullptr;
  int *tiles_dev = nullptr;
  int *mirror_dev = nullptr;   // [n_gen] index of a parameter's copy in thetaT_dev, -1 for biases (data-parallel Adam, bgm_causal_egm_apply)
  float *dev = nullptr;        // one allocation: theta_g|m_g|v_g|grad_g|theta_d|m_d|v_d|grad_d|ws
};

static EgmState *est(bgm_handle *h) { return static_cast<EgmState *>(h->egm_state); }

void bgm_egm_free_state(bgm_handle *h) {
  if (!h->egm_state) return;
  EgmState *s = est(h);
  if (s->dev) hipFree(s->dev);
  if (s->thetaT_dev) hipFree(s->thetaT_dev);
  if (s->tiles_dev) hipFree(s->tiles_dev);
  if (s->mirror_dev) hipFree(s->mirror_dev);
  delete s;
  h->egm_state = nullptr;
}

static bool fill_mlp(const HostNet &n, EgmMlp &m, int off) {
  const int L = (int)n.dims.size() - 1;
  if (L < 1 || L > EGM_MAX_LAYERS) return false;
  m.n_layers = L;
  for (int i = 0; i <= L; ++i) m.dims[i] = n.dims[i];
  m.off = off;
  egm_finish_mlp(m);
  return true;
}

extern "C" int bgm_causal_egm_begin(bgm_handle *h, const bgm_egm_config *cfg, const float *theta_dz_host, int64_t count,
                                    void *stream_) {
  (void)stream_;
  if (!h || !h->configured) { bgm_set_error("bgm_causal_egm_begin: handle not configured"); return BGM_E_STATE; }
  if (!cfg || !theta_dz_host) { bgm_set_error("bgm_causal_egm_begin: NULL argument"); return BGM_E_INVALID; }
  for (int k = 0; k < 4; ++k)
    if (!h->nets[k].set) { bgm_set_error("bgm_causal_egm_begin: install g, f, h and e with bgm_causal_set_weights first"); return BGM_E_STATE; }
  if (cfg->batch_size < 2 || cfg->batch_size > 4096) { bgm_set_error("bgm_causal_egm_begin: batch_size must be in [2, 4096]"); return BGM_E_INVALID; }
  if (cfg->n_hidden_dz < 1 || cfg->n_hidden_dz + 1 > EGM_MAX_LAYERS) { bgm_set_error("bgm_causal_egm_begin: bad dz_units"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  bgm_egm_free_state(h);
  EgmState *s = new EgmState();
  h->egm_state = s;
  s->cfg = *cfg;
  EgmArgs &a = s->base;
  const HostNet &G = h->nets[BGM_NET_G], &E = h->nets[BGM_NET_E], &F = h->nets[BGM_NET_F], &H = h->nets[BGM_NET_H];
  int off = 0;
  bool ok = fill_mlp(G, a.g, off); off += (int)G.count();
  ok = ok && fill_mlp(E, a.e, off); off += (int)E.count();
  ok = ok && fill_mlp(F, a.f, off); off += (int)F.count();
  ok = ok && fill_mlp(H, a.h, off); off += (int)H.count();
  if (!ok) { bgm_egm_free_state(h); bgm_set_error("bgm_causal_egm_begin: too many layers"); return BGM_E_UNSUPPORTED; }
  s->n_gen = (size_t)off;
  EgmDisc &d = a.dz;
  const int L = cfg->n_hidden_dz, o = egm_fill_disc(d, h->q, L, cfg->dz_units);
  d.fixed_norm = h->disc_norm;
  s->n_dz = (size_t)o;
  if ((int64_t)o != count) {
    bgm_egm_free_state(h);
    bgm_set_error("bgm_causal_egm_begin: expected " + std::to_string(o) + " discriminator parameters, got " + std::to_string(count));
    return BGM_E_INVALID;
  }
  int wmax = std::max(h->q, h->p + 1);      // widest layer
  auto scan = [&](const int *dims, int n_layers) { for (int l = 0; l <= n_layers; ++l) wmax = std::max(wmax, dims[l]); };
  scan(a.g.dims, a.g.n_layers); scan(a.e.dims, a.e.n_layers); scan(a.f.dims, a.f.n_layers); scan(a.h.dims, a.h.n_layers);
  scan(d.dims, L + 1);
  const int B = cfg->batch_size;
  const bool t2 = chain_extent(h->q, h->p).t0 == 2;
  s->plan = egm_plan({h->q, h->p, B, d.fixed_norm != 0, L, d.dims, egm_dims(a.g), egm_dims(a.e), egm_dims(a.f), egm_dims(a.h)}, egm_switches_now(),
                     sizeof(float) * (size_t)(t2 ? ech_disc_lds_floats<4, 2, 1, 2>(d, B) : ech_disc_lds_floats<4, 2, 1>(d, B)),
                     sizeof(float) * (size_t)(t2 ? ecg_lds_floats<4, 2, 1, 2>(d, B) : ecg_lds_floats<4, 2, 1>(d, B)));
  const EgmArena &arena = s->plan.arena;
  a.dmax = arena.dmax;
  a.disc_lds = arena.in_lds ? 1 : 0;
  size_t gen_stash = 0;
  std::vector<int> gen_tiles;
  if (s->plan.chain_gen_lds > 0) {      // the generator chain's stashes: every layer's input and upstream gradient of the six passes
    const int ntl = s->plan.ext.ntl;
    EcgTab &T = s->gen_tab;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t r = off; off += (n + 3) / 4 * 4; return (int)r; };
    const EgmMlp *nets[6] = {&a.g, &a.e, &a.e, &a.g, &a.f, &a.h};
    int xw[6][EGM_MAX_LAYERS], dw[6][EGM_MAX_LAYERS];
    for (int ps = 0; ps < 6; ++ps) {
      const EgmMlp &m = *nets[ps];
      for (int l = 0; l < m.n_layers; ++l) {
        xw[ps][l] = 16 * chain_tiles(m.dims[l]);
        dw[ps][l] = 16 * chain_tiles(m.dims[l + 1]);
      }
      if (nets[ps] == &a.e) xw[ps][0] = 16 * ntl;                   // the encoder's input tiles are the generator's output tiles
      if (nets[ps] == &a.g) dw[ps][m.n_layers - 1] = 16 * ntl;
      for (int l = 0; l < m.n_layers; ++l) { T.x[ps][l] = take((size_t)B * xw[ps][l]); T.d[ps][l] = take((size_t)B * dw[ps][l]); }
    }
    gen_stash = off;
    // weight-gradient tiles, with the passes that feed each net
    auto add = [&](const EgmMlp &m, int p0, int p1) {
      egm_tiles_add(m, T.x[p0], p1 >= 0 ? T.x[p1] : nullptr, T.d[p0], p1 >= 0 ? T.d[p1] : nullptr, xw[p0], dw[p0], gen_tiles);
    };
    add(a.g, ECG_PASS_G1, ECG_PASS_G2); add(a.e, ECG_PASS_E2, ECG_PASS_E1); add(a.f, ECG_PASS_F, -1); add(a.h, ECG_PASS_H, -1);
    T.n_tiles = (int)(gen_tiles.size() / ECG_TILE_INTS);
    T.n_warm = (int)s->n_gen;
  }
  a.n_gen = (int)s->n_gen; a.B = B; a.q = h->q; a.p = h->p; a.wmax = wmax;
  a.z0 = h->cfg.z_dims[0]; a.z1 = h->cfg.z_dims[1]; a.z2 = h->cfg.z_dims[2];
  a.binary = h->cfg.binary_treatment; a.use_z_rec = cfg->use_z_rec;
  // workspace bound: every buffer of either kernel is [B x width <= wmax]; count them generously
  size_t acts = 0;
  auto widths = [&](const int *dims, int n_layers) { size_t t = 0; for (int l = 0; l <= n_layers; ++l) t += dims[l] + 4; return t; };
  acts += 2 * widths(a.g.dims, a.g.n_layers) + 2 * widths(a.e.dims, a.e.n_layers) + widths(a.f.dims, a.f.n_layers) +
          widths(a.h.dims, a.h.n_layers) + 3 * 3 * widths(d.dims, L + 1) + 12 * widths(d.dims, L + 1);
  s->ws_floats = std::max((size_t)B * (acts + 16 * (size_t)wmax + 4 * (size_t)h->p + 64) + s->n_dz + arena.floats + 4096, gen_stash + 64);
  const size_t total = 4 * s->n_gen + 4 * s->n_dz + s->ws_floats + 64;
  BGM_HIP_CHECK(hipMalloc(&s->dev, total * sizeof(float)));
  BGM_HIP_CHECK(hipMemset(s->dev, 0, total * sizeof(float)));
  float *p = s->dev;
  auto take = [&](size_t n) { float *r = p; p += (n + 3) / 4 * 4; return r; };
  a.theta_g = take(s->n_gen); a.m_g = take(s->n_gen); a.v_g = take(s->n_gen); a.grad_g = take(s->n_gen);
  a.theta_d = take(s->n_dz); a.m_d = take(s->n_dz); a.v_d = take(s->n_dz); a.grad_d = take(s->n_dz);
  a.ws = take(s->ws_floats);
  s->core.set_adam(cfg->lr, EGM_B1, EGM_B2, EGM_ADAM_EPS);
  s->core.set_side(0, a.theta_g, a.m_g, a.v_g, a.grad_g, s->n_gen);
  s->core.set_side(1, a.theta_d, a.m_d, a.v_d, a.grad_d, s->n_dz);
  std::vector<float> tg;
  tg.reserve(s->n_gen);
  for (const HostNet *n : {&G, &E, &F, &H}) tg.insert(tg.end(), n->theta.begin(), n->theta.end());
  BGM_HIP_CHECK(hipMemcpy(a.theta_g, tg.data(), tg.size() * sizeof(float), hipMemcpyHostToDevice));
  BGM_HIP_CHECK(hipMemcpy(a.theta_d, theta_dz_host, s->n_dz * sizeof(float), hipMemcpyHostToDevice));
  if (s->plan.chain_gen_lds > 0) {
    // transposed mirror of the weight matrices, kept current by the kernel's Adam
    std::vector<float> tT(s->n_gen, 0.0f);
    std::vector<int> mdst(s->n_gen, -1);
    for (const EgmMlp *m : {&a.g, &a.e, &a.f, &a.h}) egm_mirror_add(*m, tg.data(), tT, mdst);
    BGM_HIP_CHECK(hipMalloc(&s->mirror_dev, sizeof(int) * s->n_gen));
    BGM_HIP_CHECK(hipMemcpy(s->mirror_dev, mdst.data(), sizeof(int) * s->n_gen, hipMemcpyHostToDevice));
    BGM_HIP_CHECK(hipMalloc(&s->thetaT_dev, sizeof(float) * (s->n_gen + 64)));     // K-contiguous tile loads read up to 15 floats past a row
    BGM_HIP_CHECK(hipMemset(s->thetaT_dev, 0, sizeof(float) * (s->n_gen + 64)));
    BGM_HIP_CHECK(hipMemcpy(s->thetaT_dev, tT.data(), sizeof(float) * s->n_gen, hipMemcpyHostToDevice));
    BGM_HIP_CHECK(hipMalloc(&s->tiles_dev, sizeof(int) * gen_tiles.size()));
    BGM_HIP_CHECK(hipMemcpy(s->tiles_dev, gen_tiles.data(), sizeof(int) * gen_tiles.size(), hipMemcpyHostToDevice));
    s->gen_tab.thetaT = s->thetaT_dev;
    s->gen_tab.tiles = s->tiles_dev;
  }
  return BGM_OK;
}

// ---- the kernels of the routes (egm_plan.h), rows in the order of the enums -- which is the order this unit has always instantiated
// them in: the order of the kernels in a module moves the register allocation of some of them (see fit_chain_kernels in fit_api.hip;
// scripts/compare_code_objects.py after any change here)
using EgmDiscFn = void (*)(EgmArgs);
using EgmGenFn = void (*)(EgmArgs, EcgTab);
static EgmDiscFn egm_disc_kernel(EgmDiscRoute r) {
  static const EgmDiscFn k[] = {egm_disc_chain_kernel<4, 0, 4, 2, 1, 2, 2>,                                                // chain-t2
                                egm_disc_chain_kernel<4, 13, 4, 2, 1, 2>, egm_disc_chain_kernel<4, 7, 4, 2, 1, 2>,        // chain-32-k13, -k7
                                egm_disc_chain_kernel<4, 0, 4, 2, 1, 2>, egm_disc_chain_kernel<4, 0, 4, 2, 1, 1>,         // chain-32-stream, chain-16
                                egm_disc_step_kernel, egm_disc_step_kernel};                                              // lds, global
  return k[(int)r];
}
static EgmGenFn egm_gen_chain_kernel_of(EgmGenRoute r) {
  static const EgmGenFn k[] = {egm_gen_chain_kernel<4, 13, 4, 2, 1, 2, true, 2>, egm_gen_chain_kernel<4, 13, 4, 2, 1, 2, true>,      // chain-t2, chain-pad
                               egm_gen_chain_kernel<4, 13, 4, 2, 1, 2>, egm_gen_chain_kernel<4, 7, 4, 2, 1, 2>,                      // chain-32-n13, -n7
                               egm_gen_chain_kernel<4, 13, 4, 2, 1, 1>, egm_gen_chain_kernel<4, 7, 4, 2, 1, 1>};                     // chain-16-n13, -n7
  return k[(int)r];
}

extern "C" int bgm_causal_egm_disc_step(bgm_handle *h, const float *z_dev, const int32_t *idx_dev, const float *v_dev, float eps,
                                        int32_t apply, float *out_dev, void *stream_) {
  if (!h || !h->egm_state) { bgm_set_error("bgm_causal_egm_disc_step: call bgm_causal_egm_begin first"); return BGM_E_STATE; }
  if (!z_dev || !idx_dev || !v_dev) { bgm_set_error("bgm_causal_egm_disc_step: NULL pointer"); return BGM_E_INVALID; }
  EgmState *s = est(h);
  BGM_HIP_CHECK(hipSetDevice(h->device));
  EgmArgs a = s->base;
  a.z = z_dev; a.idx = idx_dev; a.v = v_dev; a.x = nullptr; a.y = nullptr; a.eps = eps; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.adam = s->core.adam(1, apply != 0);
  const bool chain = s->plan.chain_disc_lds > 0;
  EgmPhaseClock::begin(a, (hipStream_t)stream_);
  if (int rc = bgm_launch(egm_disc_kernel(s->plan.disc), 1, EGM_WAVES, chain ? s->plan.chain_disc_lds : s->plan.arena.lds_bytes, (hipStream_t)stream_, a)) return rc;
  EgmPhaseClock::report("disc", chain);
  return BGM_OK;
}

extern "C" int bgm_causal_egm_gen_step(bgm_handle *h, const float *z_dev, const int32_t *idx_dev, const float *v_dev,
                                       const float *x_dev, const float *y_dev, int32_t apply, float *out_dev, void *stream_) {
  if (!h || !h->egm_state) { bgm_set_error("bgm_causal_egm_gen_step: call bgm_causal_egm_begin first"); return BGM_E_STATE; }
  if (!z_dev || !idx_dev || !v_dev || !x_dev || !y_dev) { bgm_set_error("bgm_causal_egm_gen_step: NULL pointer"); return BGM_E_INVALID; }
  EgmState *s = est(h);
  BGM_HIP_CHECK(hipSetDevice(h->device));
  EgmArgs a = s->base;
  a.z = z_dev; a.idx = idx_dev; a.v = v_dev; a.x = x_dev; a.y = y_dev; a.eps = 0.0f; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.adam = s->core.adam(0, apply != 0);
  const bool chain = s->plan.chain_gen_lds > 0;
  EgmPhaseClock::begin(a, (hipStream_t)stream_);
  if (!chain) {
    if (int rc = bgm_launch(egm_gen_step_kernel, 1, EGM_WAVES, s->plan.arena.lds_bytes, (hipStream_t)stream_, a)) return rc;
  } else {      // the chains, then the weight-gradient tiles (and Adam) over the chip
    if (int rc = bgm_launch(egm_gen_chain_kernel_of(s->plan.gen), 1, ECH_WAVES, s->plan.chain_gen_lds, (hipStream_t)stream_, a, s->gen_tab)) return rc;
    hipLaunchKernelGGL(a.B == 32 ? egm_gen_dw_kernel<2> : egm_gen_dw_kernel<1>, dim3((s->gen_tab.n_tiles + ECH_WAVES - 1) / ECH_WAVES), dim3(ECH_THREADS), 0,
                       (hipStream_t)stream_, a, s->gen_tab);
    BGM_HIP_CHECK(hipGetLastError());
  }
  EgmPhaseClock::report("gen", chain);
  return BGM_OK;
}

extern "C" int bgm_causal_egm_grad(bgm_handle *h, int32_t which, float scale, float *grad_dev, int64_t count, void *stream_) {
  if (!h || !h->egm_state) { bgm_set_error("bgm_causal_egm_grad: call bgm_causal_egm_begin first"); return BGM_E_STATE; }
  return egm_grad(est(h)->core, h->device, "bgm_causal_egm_grad", which, scale, grad_dev, count, (hipStream_t)stream_);
}

extern "C" int bgm_causal_egm_apply(bgm_handle *h, int32_t which, const float *grad_dev, int64_t count, void *stream_) {
  if (!h || !h->egm_state) { bgm_set_error("bgm_causal_egm_apply: call bgm_causal_egm_begin first"); return BGM_E_STATE; }
  EgmState *s = est(h);
  return egm_apply(s->core, h->device, "bgm_causal_egm_apply", which, grad_dev, count, (hipStream_t)stream_, s->thetaT_dev, s->mirror_dev);
}

extern "C" int bgm_causal_egm_read(bgm_handle *h, int32_t what, float *host, int64_t count, void *stream_) {
  if (!h || !h->egm_state || !host) { bgm_set_error("bgm_causal_egm_read: no session / NULL"); return BGM_E_STATE; }
  return egm_read(est(h)->core, h->device, "bgm_causal_egm_read", "bgm_causal_egm_read", what, host, count, (hipStream_t)stream_);
}

extern "C" int bgm_causal_egm_sync(bgm_handle *h, void *stream_) {
  if (!h || !h->egm_state) { bgm_set_error("bgm_causal_egm_sync: no session"); return BGM_E_STATE; }
  EgmState *s = est(h);
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BGM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
  std::vector<float> tg(s->n_gen);
  BGM_HIP_CHECK(hipMemcpy(tg.data(), s->base.theta_g, s->n_gen * sizeof(float), hipMemcpyDeviceToHost));
  size_t off = 0;
  for (int id : {BGM_NET_G, BGM_NET_E, BGM_NET_F, BGM_NET_H}) {
    HostNet &n = h->nets[id];
    std::memcpy(n.theta.data(), tg.data() + off, n.count() * sizeof(float));
    off += n.count();
  }
  h->blob_valid = false; h->bx_valid = false; h->eblob_valid = false;
  h->det_valid = false;   // the general sampling path's packed copy follows the refreshed networks as well
  h->gx_valid = false;
  return BGM_OK;
}

extern "C" int bgm_causal_egm_end(bgm_handle *h, void *stream_) {
  if (!h) return BGM_E_INVALID;
  if (!h->egm_state) return BGM_OK;
  int rc = bgm_causal_egm_sync(h, stream_);
  bgm_egm_free_state(h);
  return rc;
}
