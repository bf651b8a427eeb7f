// bgm_egm_api.hip -- C-ABI entry points of the BGM EGM warm start (include/bgm_hip.h, BGM EGM section).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bgm_host.h"
#include "bgm_state.h"
#include "bgm_egm_kernels.h"
#include "egm_host.h"

static constexpr float BEGM_B1 = 0.5f, BEGM_B2 = 0.9f, BEGM_ADAM_EPS = 1e-7f;   // bgm/base.py:82-85, Keras epsilon

using BgmEgmState = BgmEgmSession<BgmEgmArgs>;
static BgmEgmState *best(bgm_handle *h) { return static_cast<BgmEgmState *>(h->bgm_egm_state); }

void bgm_bgm_egm_free_state(bgm_handle *h) {
  delete best(h);
  h->bgm_egm_state = nullptr;
}

extern "C" int bgm_bgm_egm_begin(bgm_handle *h, const bgm_bgm_egm_config *cfg, const float *theta_e_host, int64_t count_e,
                                 const float *theta_dz_host, int64_t count_dz, const float *theta_dx_host, int64_t count_dx,
                                 void *stream_) {
  (void)stream_;
  if (!h || !h->bgm_state || !bst(h)->configured || !bst(h)->set) { bgm_set_error("bgm_bgm_egm_begin: configure the BGM model and set its weights first"); return BGM_E_STATE; }
  if (!cfg || !theta_e_host || !theta_dz_host || !theta_dx_host) { bgm_set_error("bgm_bgm_egm_begin: NULL argument"); return BGM_E_INVALID; }
  if (cfg->batch_size < 2 || cfg->batch_size > 4096) { bgm_set_error("bgm_bgm_egm_begin: batch_size must be in [2, 4096]"); return BGM_E_INVALID; }
  if (cfg->n_hidden_e < 1 || cfg->n_hidden_e + 1 > EGM_MAX_LAYERS || cfg->n_hidden_dz < 1 || cfg->n_hidden_dz + 1 > EGM_MAX_LAYERS ||
      cfg->n_hidden_dx < 1 || cfg->n_hidden_dx + 1 > EGM_MAX_LAYERS) { bgm_set_error("bgm_bgm_egm_begin: bad layer counts"); return BGM_E_INVALID; }
  BgmState *bs = bst(h);
  const int q = bs->cfg.z_dim, p = bs->cfg.x_dim, NH = bs->cfg.n_hidden_g;
  if (NH + 1 > EGM_MAX_LAYERS) { bgm_set_error("bgm_bgm_egm_begin: too many generator layers"); return BGM_E_UNSUPPORTED; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  if (bs->fit_active) { bgm_set_error("bgm_bgm_egm_begin: a fit session is active"); return BGM_E_STATE; }
  bgm_bgm_egm_free_state(h);
  BgmEgmState *s = new BgmEgmState();
  h->bgm_egm_state = s;
  s->cfg = *cfg;
  BgmEgmArgs &a = s->base;
  // generator
  EgmVarNet &g = a.g;
  g.q = q; g.p = p; g.hlast = bs->cfg.g_units[NH - 1];
  g.mlp.n_layers = NH + 1;
  g.mlp.dims[0] = q;
  for (int i = 0; i < NH; ++i) g.mlp.dims[i + 1] = bs->cfg.g_units[i];
  g.mlp.dims[NH + 1] = p;
  g.mlp.off = 4 * q;
  egm_finish_mlp(g.mlp);
  int o = 4 * q;
  for (int l = 0; l <= NH; ++l) o += g.mlp.dims[l] * g.mlp.dims[l + 1] + g.mlp.dims[l + 1];
  g.wvar = o; o += g.hlast * p;
  g.bvar = o; o += p;
  s->n_g = (size_t)o;
  if (s->n_g != bs->theta.size()) { bgm_bgm_egm_free_state(h); bgm_set_error("bgm_bgm_egm_begin: internal parameter count mismatch"); return BGM_E_INVALID; }
  if (int rc = bgm_egm_describe(*s, "bgm_bgm_egm_begin", q, p, h->disc_norm, count_e, count_dz, count_dx)) { bgm_bgm_egm_free_state(h); return rc; }
  const EgmMlp &e = a.e;
  int wmax = std::max(q, p);
  size_t widths = 0;
  auto scan = [&](const int *dims, int n_layers) { size_t t = 0; for (int l = 0; l <= n_layers; ++l) { wmax = std::max(wmax, dims[l]); t += dims[l] + 4; } return t; };
  const size_t wg = scan(g.mlp.dims, g.mlp.n_layers), we = scan(e.dims, e.n_layers);
  const size_t wdz = scan(a.dz.dims, a.dz.n_hidden + 1), wdx = scan(a.dx.dims, a.dx.n_hidden + 1);
  const int B = cfg->batch_size;
  a.B = B; a.wmax = wmax; a.n_gen = (int)s->n_gen; a.n_disc = (int)s->n_disc;
  a.gamma = cfg->gamma; a.alpha = cfg->alpha;
  // workspace bound (floats per row): generator caches x2 (+ zhat, zn, s_raw), encoder caches x2, data-sized temporaries,
  // one discriminator cache, the gradient-penalty scratch of the wider discriminator, scratch rows
  widths = 2 * (wg + 3 * (size_t)q + p) + 2 * we + 10 * (size_t)p + 3 * std::max(wdz, wdx) + 8 * std::max(wdz, wdx) + 12 * (size_t)wmax + 64;
  s->ws_floats = (size_t)B * widths + s->n_disc + 8192;
  if (int rc = bgm_egm_allocate(*s, 64, we, h->n_cus, theta_e_host, theta_dz_host, theta_dx_host)) return rc;
  BGM_HIP_CHECK(hipMemcpy(a.theta_g, bs->theta.data(), s->n_g * sizeof(float), hipMemcpyHostToDevice));
  s->core.set_adam(cfg->lr, BEGM_B1, BEGM_B2, BEGM_ADAM_EPS);
  return BGM_OK;
}

extern "C" int bgm_bgm_egm_disc_step(bgm_handle *h, const float *z_dev, const float *x_dev, const float *noise_dev, float eps_z,
                                     float eps_x, int32_t apply, float *out_dev, void *stream_) {
  if (!h || !h->bgm_egm_state) { bgm_set_error("bgm_bgm_egm_disc_step: call bgm_bgm_egm_begin first"); return BGM_E_STATE; }
  if (!z_dev || !x_dev || !noise_dev) { bgm_set_error("bgm_bgm_egm_disc_step: NULL pointer"); return BGM_E_INVALID; }
  BgmEgmState *s = best(h);
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BgmEgmArgs a = s->base;
  a.z = z_dev; a.x = x_dev; a.n1 = noise_dev; a.n2 = nullptr; a.eps_z = eps_z; a.eps_x = eps_x; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.adam = s->core.adam(1, apply != 0);
  hipLaunchKernelGGL(bgm_egm_disc_step_kernel, dim3(1), dim3(EGM_THREADS), BGM_EGM_LDS, (hipStream_t)stream_, a);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

extern "C" int bgm_bgm_egm_gen_step(bgm_handle *h, const float *z_dev, const float *x_dev, const float *noise1_dev,
                                    const float *noise2_dev, int32_t apply, float *out_dev, void *stream_) {
  if (!h || !h->bgm_egm_state) { bgm_set_error("bgm_bgm_egm_gen_step: call bgm_bgm_egm_begin first"); return BGM_E_STATE; }
  if (!z_dev || !x_dev || !noise1_dev || !noise2_dev) { bgm_set_error("bgm_bgm_egm_gen_step: NULL pointer"); return BGM_E_INVALID; }
  BgmEgmState *s = best(h);
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BgmEgmArgs a = s->base;
  a.z = z_dev; a.x = x_dev; a.n1 = noise1_dev; a.n2 = noise2_dev; a.eps_z = a.eps_x = 0.0f; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.adam = s->core.adam(0, apply != 0);
  hipLaunchKernelGGL(bgm_egm_gen_step_kernel, dim3(1), dim3(EGM_THREADS), BGM_EGM_LDS, (hipStream_t)stream_, a);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

extern "C" int bgm_bgm_egm_read(bgm_handle *h, int32_t what, float *host, int64_t count, void *stream_) {
  if (!h || !h->bgm_egm_state || !host) { bgm_set_error("bgm_bgm_egm_read: no session / NULL"); return BGM_E_STATE; }
  return egm_read(best(h)->core, h->device, "bgm_bgm_egm_read", "bgm_bgm_egm_read/write", what, host, count, (hipStream_t)stream_);
}

extern "C" int bgm_bgm_egm_write(bgm_handle *h, int32_t what, const float *host, int64_t count, void *stream_) {
  if (!h || !h->bgm_egm_state || !host) { bgm_set_error("bgm_bgm_egm_write: no session / NULL"); return BGM_E_STATE; }
  return egm_write(best(h)->core, h->device, "bgm_bgm_egm_write", "bgm_bgm_egm_read/write", what, host, count, (hipStream_t)stream_);
}

extern "C" int bgm_bgm_egm_encode(bgm_handle *h, const float *x_dev, int64_t n, float *z_dev, void *stream_) {
  if (!h || !h->bgm_egm_state) { bgm_set_error("bgm_bgm_egm_encode: no session"); return BGM_E_STATE; }
  return bgm_egm_encode(*best(h), bgm_egm_encode_kernel, h->device, "bgm_bgm_egm_encode", x_dev, n, z_dev, (hipStream_t)stream_);
}

extern "C" int bgm_bgm_egm_sync(bgm_handle *h, void *stream_) {
  if (!h || !h->bgm_egm_state) { bgm_set_error("bgm_bgm_egm_sync: no session"); return BGM_E_STATE; }
  BgmEgmState *s = best(h);
  BgmState *bs = bst(h);
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BGM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
  BGM_HIP_CHECK(hipMemcpy(bs->theta.data(), s->base.theta_g, s->n_g * sizeof(float), hipMemcpyDeviceToHost));
  bs->set = true; bs->blob_valid = false; bs->gx_valid = false;
  return BGM_OK;
}

extern "C" int bgm_bgm_egm_end(bgm_handle *h, void *stream_) {
  if (!h) return BGM_E_INVALID;
  if (!h->bgm_egm_state) return BGM_OK;
  int rc = bgm_bgm_egm_sync(h, stream_);
  bgm_bgm_egm_free_state(h);
  return rc;
}
