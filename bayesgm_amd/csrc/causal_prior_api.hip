// causal_prior_api.hip -- the CausalBGM sampling kernels with a per-row conditional latent prior (IdentifiableCausalBGM,
// models/causalbgm/identifiable.py:195-211 update_latent_variable_sgd, :521-555 get_log_posterior, :557-614
// metropolis_hastings_sampler): the PRIOR = 1 instantiations of causal_kernels.h, kept in their own translation unit.
// Selected by bgm_causal_set_prior (include/bgm_hip.h); the default path (causal_api.hip) is untouched.
#include <algorithm>
#include <cmath>
#include <string>

#include "causal_launch.h"
#include "prior_kernels.h"

extern "C" int bgm_causal_set_prior(bgm_handle *h, const int32_t *seg_dev, const float *tab_dev, int32_t n_segments) {
  if (!h || !h->configured) { bgm_set_error("bgm_causal_set_prior: handle not configured"); return BGM_E_STATE; }
  if ((seg_dev == nullptr) != (tab_dev == nullptr) || (seg_dev && n_segments <= 0)) { bgm_set_error("bgm_causal_set_prior: seg_dev and tab_dev go together"); return BGM_E_INVALID; }
  h->prior_seg = seg_dev; h->prior_tab = tab_dev; h->prior_segments = seg_dev ? n_segments : 0;
  return BGM_OK;
}

int bgm_causal_prior_logpost(bgm_handle *h, const float *x, const float *y, const float *v, const float *z, int64_t n, float *out,
                             int grid, hipStream_t stream) {
  return bgm_causal_dispatch(h, "conditional prior: kernel", [&](auto s) {
    using S = decltype(s);
    return bgm_launch(causal_logpost_kernel<S::KT1, S::KSL1, S::NTL, MH_R, MH_WAVES, 1>, grid, MH_WAVES, h->meta.total * 4, stream,
                      h->sblob_dev, h->meta, x, y, v, z, n, out, h->prior_seg, h->prior_tab);
  });
}

int bgm_causal_prior_mh_launch(bgm_handle *h, const CausalMhKArgs &a, int effect, int grid, int lds, hipStream_t stream) {
  CausalMhKArgs ka = a;
  ka.seg = (const int *)h->prior_seg;
  ka.prior_tab = h->prior_tab;
  return bgm_causal_with_effect(effect, [&](auto e) {
    return bgm_causal_dispatch(h, "conditional prior: MH kernel", [&](auto s) {
      using S = decltype(s);
      constexpr int EFFECT = decltype(e)::value;
      return bgm_launch(ka.uc ? causal_mh_kernel<S::KT1, S::KSL1, S::NTL, MH_R, MH_WAVES, EFFECT, 1, (S::NTL > 2)>
                              : causal_mh_kernel<S::KT1, S::KSL1, S::NTL, MH_R, MH_WAVES, EFFECT, 1>,
                        grid, MH_WAVES, lds, stream, ka);
    });
  });
}


// ---- the prior network itself (prior_kernels.h)
static int prior_net_of(const bgm_prior_config *cfg, int rows, PriorNet &n, int &lds_floats, const char *who) {
  if (!cfg || cfg->n_layers < 1 || cfg->n_layers > PRIOR_MAX_LAYERS) { bgm_set_error(std::string(who) + ": prior net needs 1.." + std::to_string(PRIOR_MAX_LAYERS) + " dense layers"); return BGM_E_INVALID; }
  n = PriorNet{};
  n.n_layers = cfg->n_layers;
  int off = 0, a = 0, wmax = 0;
  for (int l = 0; l <= cfg->n_layers; ++l) {
    if (cfg->dims[l] < 1) { bgm_set_error(std::string(who) + ": bad layer width"); return BGM_E_INVALID; }
    n.dims[l] = cfg->dims[l];
    if (l) wmax = std::max(wmax, cfg->dims[l]);
  }
  for (int l = 0; l < cfg->n_layers; ++l) {
    n.w_off[l] = off; off += n.dims[l] * n.dims[l + 1];
    n.b_off[l] = off; off += n.dims[l + 1];
    n.a_off[l] = a; a += rows * n.dims[l + 1];
  }
  n.a_off[cfg->n_layers] = a;
  n.n_params = off; n.wmax = wmax;
  lds_floats = a;
  return BGM_OK;
}

extern "C" int bgm_prior_n_params(const bgm_prior_config *cfg, int64_t *count) {
  PriorNet n; int lf;
  int rc = prior_net_of(cfg, 1, n, lf, "bgm_prior_n_params");
  if (rc) return rc;
  if (!count) { bgm_set_error("bgm_prior_n_params: NULL count"); return BGM_E_INVALID; }
  *count = n.n_params;
  return BGM_OK;
}

extern "C" int bgm_prior_table(bgm_handle *h, const bgm_prior_config *cfg, const float *theta_dev, float *table_dev, void *stream_) {
  if (!h || !h->configured || !theta_dev || !table_dev) { bgm_set_error("bgm_prior_table: bad argument"); return BGM_E_INVALID; }
  PriorNet n; int lf;
  int rc = prior_net_of(cfg, cfg ? cfg->dims[0] : 0, n, lf, "bgm_prior_table");
  if (rc) return rc;
  if (n.dims[n.n_layers] != h->q + 1) { bgm_set_error("bgm_prior_table: the prior net must end in q + 1 outputs"); return BGM_E_INVALID; }
  if ((size_t)lf * 4 > 150 * 1024) { bgm_set_error("bgm_prior_table: prior net too wide for one workgroup's LDS"); return BGM_E_UNSUPPORTED; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  return bgm_launch(prior_table_kernel, 1, PRIOR_THREADS / 64, lf * 4, (hipStream_t)stream_, n, theta_dev, table_dev, h->q);
}

static int prior_step_impl(bgm_handle *h, const bgm_prior_config *cfg, float *theta_dev, float *m_dev, float *v_dev, const int32_t *seg_dev,
                           float *data_z_dev, const int32_t *idx_dev, int32_t batch, int32_t batch_global, const float *dz_dev, float lr_z,
                           float lr_prior, int64_t t_z, int64_t t_prior, float *grad_dev, int apply, float *out_dev, void *stream_, const char *who) {
  if (!h || !h->configured || !theta_dev || (apply && (!m_dev || !v_dev)) || !seg_dev || !data_z_dev || !idx_dev || !dz_dev || batch < 1 ||
      batch_global < batch || t_z < 1 || (apply && t_prior < 1) || (!apply && !grad_dev)) {
    bgm_set_error(std::string(who) + ": bad argument"); return BGM_E_INVALID;
  }
  PriorNet n; int lf;
  int rc = prior_net_of(cfg, batch, n, lf, who);
  if (rc) return rc;
  const int q = h->q;
  if (n.dims[n.n_layers] != q + 1) { bgm_set_error(std::string(who) + ": the prior net must end in q + 1 outputs"); return BGM_E_INVALID; }
  const size_t bytes = ((size_t)lf + (size_t)batch * q + 2 * (size_t)batch * n.wmax + 3 * (size_t)batch) * 4;
  if (bytes > 150 * 1024) { bgm_set_error(std::string(who) + ": minibatch x prior-net widths exceed one workgroup's LDS"); return BGM_E_UNSUPPORTED; }
  auto lr_t = [](double lr, double t) { return (float)(lr * std::sqrt(1.0 - std::pow(0.99, t)) / (1.0 - std::pow(0.9, t))); };
  PriorStepArgs a{};
  a.net = n; a.theta = theta_dev; a.m = m_dev; a.v = v_dev; a.seg = seg_dev; a.data_z = data_z_dev; a.idx = idx_dev; a.dz = dz_dev;
  a.B = batch; a.q = q; a.lr_t_z = lr_t(lr_z, (double)t_z); a.lr_t_p = apply ? lr_t(lr_prior, (double)t_prior) : 0.0f;
  a.b1 = 0.9f; a.b2 = 0.99f; a.eps = 1e-7f;        // tf.keras.optimizers.Adam(lr, beta_1=0.9, beta_2=0.99), identifiable.py:88-95
  a.out = out_dev; a.inv_B = 1.0f / (float)batch_global; a.grad = grad_dev; a.apply = apply;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  return bgm_launch(prior_step_kernel, 1, PRIOR_THREADS / 64, (int)bytes, (hipStream_t)stream_, a);
}

extern "C" int bgm_prior_step(bgm_handle *h, const bgm_prior_config *cfg, float *theta_dev, float *m_dev, float *v_dev, const int32_t *seg_dev,
                              float *data_z_dev, const int32_t *idx_dev, int32_t batch, const float *dz_dev, float lr_z, float lr_prior,
                              int64_t t_z, int64_t t_prior, float *out_dev, void *stream_) {
  return prior_step_impl(h, cfg, theta_dev, m_dev, v_dev, seg_dev, data_z_dev, idx_dev, batch, batch, dz_dev, lr_z, lr_prior, t_z, t_prior, nullptr, 1,
                         out_dev, stream_, "bgm_prior_step");
}

extern "C" int bgm_prior_grad(bgm_handle *h, const bgm_prior_config *cfg, const float *theta_dev, const int32_t *seg_dev, float *data_z_dev,
                              const int32_t *idx_dev, int32_t batch, int32_t batch_global, const float *dz_dev, float lr_z, int64_t t_z,
                              float *grad_dev, float *out_dev, void *stream_) {
  return prior_step_impl(h, cfg, const_cast<float *>(theta_dev), nullptr, nullptr, seg_dev, data_z_dev, idx_dev, batch, batch_global, dz_dev, lr_z, 0.0f,
                         t_z, 0, grad_dev, 0, out_dev, stream_, "bgm_prior_grad");
}

extern "C" int bgm_prior_apply(bgm_handle *h, const bgm_prior_config *cfg, float *theta_dev, float *m_dev, float *v_dev, const float *grad_dev,
                               float lr_prior, int64_t t_prior, void *stream_) {
  if (!h || !theta_dev || !m_dev || !v_dev || !grad_dev || t_prior < 1) { bgm_set_error("bgm_prior_apply: bad argument"); return BGM_E_INVALID; }
  int64_t count = 0;
  int rc = bgm_prior_n_params(cfg, &count);
  if (rc) return rc;
  const float lr_t = (float)((double)lr_prior * std::sqrt(1.0 - std::pow(0.99, (double)t_prior)) / (1.0 - std::pow(0.9, (double)t_prior)));
  BGM_HIP_CHECK(hipSetDevice(h->device));
  hipLaunchKernelGGL(prior_adam_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, theta_dev, m_dev, v_dev, grad_dev, (int)count,
                     lr_t, 0.9f, 0.99f, 1e-7f);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
