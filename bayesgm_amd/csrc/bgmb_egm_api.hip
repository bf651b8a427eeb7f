// bgmb_egm_api.hip -- C-ABI entry points of the EGM warm start of BGM with the Bayesian generator (bgm_bvn_egm_*).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "bgm_host.h"
#include "bgmb_state.h"
#include "bgmb_egm_kernels.h"
#include "egm_host.h"

static constexpr float VEGM_B1 = 0.5f, VEGM_B2 = 0.9f, VEGM_ADAM_EPS = 1e-7f;   // bgm/base.py:82-85, Keras epsilon

using BgmbEgmState = BgmEgmSession<BgmbEgmArgs>;

void bgm_bvn_egm_free(void *p) { delete static_cast<BgmbEgmState *>(p); }

static BgmbState *vst(bgm_handle *h) { return static_cast<BgmbState *>(h->bvn_state); }
static BgmbEgmState *vest(bgm_handle *h) { return (h && h->bvn_state) ? static_cast<BgmbEgmState *>(vst(h)->egm) : nullptr; }

extern "C" int bgm_bvn_egm_begin(bgm_handle *h, const bgm_bgm_egm_config *cfg, const float *theta_e_host, int64_t count_e,
                                 const float *theta_dz_host, int64_t count_dz, const float *theta_dx_host, int64_t count_dx,
                                 void *stream_) {
  if (!h || !h->bvn_state) { bgm_set_error("bgm_bvn_egm_begin: no session (bgm_bvn_begin)"); return BGM_E_STATE; }
  if (!cfg || !theta_e_host || !theta_dz_host || !theta_dx_host) { bgm_set_error("bgm_bvn_egm_begin: NULL argument"); return BGM_E_INVALID; }
  if (cfg->batch_size < 2 || cfg->batch_size > 4096) { bgm_set_error("bgm_bvn_egm_begin: batch_size must be in [2, 4096]"); return BGM_E_INVALID; }
  if (cfg->n_hidden_e < 1 || cfg->n_hidden_e + 1 > EGM_MAX_LAYERS || cfg->n_hidden_dz < 1 || cfg->n_hidden_dz + 1 > EGM_MAX_LAYERS ||
      cfg->n_hidden_dx < 1 || cfg->n_hidden_dx + 1 > EGM_MAX_LAYERS) { bgm_set_error("bgm_bvn_egm_begin: bad layer counts"); return BGM_E_INVALID; }
  BgmbState *bs = vst(h);
  const int q = bs->q, p = bs->p;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BGM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
  bgm_bvn_egm_free(bs->egm);
  bs->egm = nullptr;
  BgmbEgmState *s = new BgmbEgmState();
  bs->egm = s;
  s->cfg = *cfg;
  BgmbEgmArgs &a = s->base;
  a.g = bs->net;
  a.q = q; a.p = p;
  s->n_g = (size_t)bs->n_params;
  if (int rc = bgm_egm_describe(*s, "bgm_bvn_egm_begin", q, p, h->disc_norm, count_e, count_dz, count_dx)) {
    bgm_bvn_egm_free(bs->egm); bs->egm = nullptr;
    return rc;
  }
  const EgmMlp &e = a.e;
  int wmax = std::max(bs->wmax, std::max(q, 2 * p));
  auto scan = [&](const int *dims, int n_layers) { size_t t = 0; for (int l = 0; l <= n_layers; ++l) { wmax = std::max(wmax, dims[l]); t += dims[l] + 4; } return t; };
  const size_t we = scan(e.dims, e.n_layers);
  const size_t wdz = scan(a.dz.dims, a.dz.n_hidden + 1), wdx = scan(a.dx.dims, a.dx.n_hidden + 1);
  const int B = cfg->batch_size;
  a.B = B; a.wmax = wmax; a.n_gen = (int)s->n_gen; a.n_disc = (int)s->n_disc;
  a.gamma = cfg->gamma; a.alpha = cfg->alpha;
  // workspace: two Flipout call caches, two encoder caches, data-sized temporaries, one discriminator cache, the
  // gradient-penalty scratch of the wider discriminator, scratch rows
  const size_t widths = 2 * we + 10 * (size_t)p + 2 * (size_t)q + 11 * std::max(wdz, wdx) + 12 * (size_t)wmax + 64;
  s->ws_floats = 2 * bnn_cache_floats(a.g, B) + (size_t)B * widths + s->n_disc + 8192;
  if (int rc = bgm_egm_allocate(*s, 256, we, h->n_cus, theta_e_host, theta_dz_host, theta_dx_host)) return rc;
  BGM_HIP_CHECK(hipMemcpy(a.theta_g, bs->theta_dev, s->n_g * sizeof(float), hipMemcpyDeviceToDevice));
  s->core.set_adam(cfg->lr, VEGM_B1, VEGM_B2, VEGM_ADAM_EPS);
  return BGM_OK;
}

extern "C" int bgm_bvn_egm_disc_step(bgm_handle *h, const float *z_dev, const float *x_dev, const float *noise_dev, float eps_z,
                                     float eps_x, uint64_t seed, uint32_t stream_id, int32_t apply, float *out_dev, void *stream_) {
  BgmbEgmState *s = vest(h);
  if (!s) { bgm_set_error("bgm_bvn_egm_disc_step: call bgm_bvn_egm_begin first"); return BGM_E_STATE; }
  if (!z_dev || !x_dev || !noise_dev) { bgm_set_error("bgm_bvn_egm_disc_step: NULL pointer"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BgmbEgmArgs a = s->base;
  a.z = z_dev; a.x = x_dev; a.n1 = noise_dev; a.n2 = nullptr; a.eps_z = eps_z; a.eps_x = eps_x; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream_id;
  a.adam = s->core.adam(1, apply != 0);
  hipLaunchKernelGGL(bgmb_egm_disc_step_kernel, dim3(1), dim3(EGM_THREADS), BGM_EGM_LDS, (hipStream_t)stream_, a);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

extern "C" int bgm_bvn_egm_gen_step(bgm_handle *h, const float *z_dev, const float *x_dev, const float *noise1_dev,
                                    const float *noise2_dev, uint64_t seed, uint32_t stream_id, int32_t apply, float *out_dev,
                                    void *stream_) {
  BgmbEgmState *s = vest(h);
  if (!s) { bgm_set_error("bgm_bvn_egm_gen_step: call bgm_bvn_egm_begin first"); return BGM_E_STATE; }
  if (!z_dev || !x_dev || !noise1_dev || !noise2_dev) { bgm_set_error("bgm_bvn_egm_gen_step: NULL pointer"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BgmbEgmArgs a = s->base;
  a.z = z_dev; a.x = x_dev; a.n1 = noise1_dev; a.n2 = noise2_dev; a.eps_z = a.eps_x = 0.0f; a.out = out_dev; a.apply = apply ? 1 : 0;
  a.k0 = (uint32_t)(seed & 0xFFFFFFFFull); a.k1 = (uint32_t)(seed >> 32); a.stream = stream_id;
  a.adam = s->core.adam(0, apply != 0);
  hipLaunchKernelGGL(bgmb_egm_gen_step_kernel, dim3(1), dim3(EGM_THREADS), BGM_EGM_LDS, (hipStream_t)stream_, a);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

extern "C" int bgm_bvn_egm_read(bgm_handle *h, int32_t what, float *host, int64_t count, void *stream_) {
  BgmbEgmState *s = vest(h);
  if (!s || !host) { bgm_set_error("bgm_bvn_egm_read: no session / NULL"); return BGM_E_STATE; }
  return egm_read(s->core, h->device, "bgm_bvn_egm_read", "bgm_bvn_egm_read/write", what, host, count, (hipStream_t)stream_);
}

extern "C" int bgm_bvn_egm_write(bgm_handle *h, int32_t what, const float *host, int64_t count, void *stream_) {
  BgmbEgmState *s = vest(h);
  if (!s || !host) { bgm_set_error("bgm_bvn_egm_write: no session / NULL"); return BGM_E_STATE; }
  return egm_write(s->core, h->device, "bgm_bvn_egm_write", "bgm_bvn_egm_read/write", what, host, count, (hipStream_t)stream_);
}

extern "C" int bgm_bvn_egm_encode(bgm_handle *h, const float *x_dev, int64_t n, float *z_dev, void *stream_) {
  BgmbEgmState *s = vest(h);
  if (!s) { bgm_set_error("bgm_bvn_egm_encode: no session"); return BGM_E_STATE; }
  return bgm_egm_encode(*s, bgm_egm_encode_kernel, h->device, "bgm_bvn_egm_encode", x_dev, n, z_dev, (hipStream_t)stream_);
}

// copy the session's generator into the bvn session (its Adam slots are untouched)
extern "C" int bgm_bvn_egm_sync(bgm_handle *h, void *stream_) {
  BgmbEgmState *s = vest(h);
  if (!s) { bgm_set_error("bgm_bvn_egm_sync: no session"); return BGM_E_STATE; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  BGM_HIP_CHECK(hipMemcpyAsync(vst(h)->theta_dev, s->base.theta_g, s->n_g * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream_));
  return BGM_OK;
}

extern "C" int bgm_bvn_egm_end(bgm_handle *h, void *stream_) {
  if (!h) return BGM_E_INVALID;
  BgmbEgmState *s = vest(h);
  if (!s) return BGM_OK;
  int rc = bgm_bvn_egm_sync(h, stream_);
  BGM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
  bgm_bvn_egm_free(vst(h)->egm);
  vst(h)->egm = nullptr;
  return rc;
}
