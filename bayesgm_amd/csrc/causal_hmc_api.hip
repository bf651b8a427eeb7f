// causal_hmc_api.hip -- C-ABI entry points of the CausalBGM log posterior with its gradient and of the HMC latent sampler with a step
// size per chain (bgm_causal_logpost_grad, bgm_causal_hmc_run; include/bgm_hip.h), and the host-side packing of their weights: the
// Gram copy of the sampling blob (causal_api.hip) re-laid in the dual-access layout of bgm_kernels.h.  Kernels: causal_hmc_kernels.h;
// the transition behind causal_hmc_kernel is chmc_run (causal_hmc_fx_kernels.h), shared with the metric and the effect kernels.
// Of the shape table (causal_launch.h) only KT1 matters to these kernels: the Gram form takes g's output layer, and with it NTL, out
// of them, and the dual-access first layers always run all 4 KT1 K-steps, so KSL1 has no meaning either.  They are instantiated per
// KT1 and dispatched through bgm_causal_dispatch on the handle's shape like every other family.
#include <string>
#include <vector>

#include "causal_launch.h"
#include "causal_hmc_host.h"
#include "causal_hmc_obs_host.h"
#include "bnf_det_host.h"
#include "gx_host.h"

namespace {

// element (input row rho, output column o) of a layer packed by pack_layer (bgm_host.h) with K_ROWS input rows and NT output tiles
float packed_at(const std::vector<float> &b, int off, int K_ROWS, int NT, int rho, int o) {
  const int t = o >> 4;
  int T0 = 0, GS = group_size(NT);
  while (t >= T0 + GS) { T0 += GS; GS = group_size(NT - T0); }
  return b[(size_t)off + (size_t)K_ROWS * 16 * T0 + ((size_t)rho * 16 + (o & 15)) * GS + (t - T0)];
}

// [NT][K_ROWS][17] from a pack_layer block
void to_dual(const std::vector<float> &src, int s_off, std::vector<float> &dst, int d_off, int K_ROWS, int NT) {
  for (int to = 0; to < NT; ++to)
    for (int rho = 0; rho < K_ROWS; ++rho)
      for (int c = 0; c < 16; ++c) dst[(size_t)d_off + ((size_t)to * K_ROWS + rho) * 17 + c] = packed_at(src, s_off, K_ROWS, NT, rho, 16 * to + c);
}

const char *refused_path(const bgm_handle *h) {
  return h->bnn_state ? "the Bayesian networks (a bgm_bnn_begin session is open on this handle)"
         : gx_wanted(h) ? "the general-width engine (hidden widths outside the compiled families)"
         : bnf_det_wanted(h) ? "the streamed-fragment kernels (no LDS-resident compiled shape holds the model)"
         : h->precision != 0 ? "the split-precision kernels (bgm_causal_set_precision)"
         : h->prior_seg ? "the conditional latent prior (bgm_causal_set_prior)" : nullptr;
}

// the Gram blob of the handle and this panel's 2 u, c; then the dual-access copy, rebuilt whenever the Gram copy was
int hmc_prepare(bgm_handle *h, const float *v, int64_t n, hipStream_t stream, HmcState *&st) {
  if (int rc = bgm_causal_gram_prepare(h, v, n, stream)) return rc;
  st = bgm_causal_hmc_state(h);
  if (h->hmc_valid) return BGM_OK;
  const CausalMeta &gm = h->gmeta;
  const int KT1 = h->KT1, KR1 = 16 * KT1;
  std::vector<float> gb((size_t)gm.total);
  BGM_HIP_CHECK(hipMemcpyAsync(gb.data(), h->gblob_dev, gb.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
  BGM_HIP_CHECK(hipStreamSynchronize(stream));
  CausalHmcMeta &m = st->m;
  m = CausalHmcMeta{};
  m.q = gm.q; m.p = gm.p; m.binary = gm.binary; m.n_gh = gm.n_gh;
  m.sig2_v = gm.sig2_v; m.sig2_x = gm.sig2_x; m.sig2_y = gm.sig2_y;
  if (m.n_gh > CHMC_MAX_GH) { bgm_set_error("bgm_causal_hmc: more hidden layers in g than the kernel unrolls"); return BGM_E_UNSUPPORTED; }
  int off = 0;
  auto take = [&](int count) { int o = off; off += (count + 3) / 4 * 4; return o; };
  m.w1g = take(4 * KR1 * 17); m.w1f = take(4 * KR1 * 17); m.w1h = take(4 * KR1 * 17);
  m.b1g = take(64); m.b1f = take(64); m.b1h = take(64);
  m.wg = take(m.n_gh * CHMC_W64); m.bg = take(m.n_gh * 64);
  m.gram = take(CHMC_W64); m.ga = take(132);
  m.wf2 = take(2 * 64 * 17); m.bf2 = take(32); m.wf3 = take(32 * 17); m.bf3 = take(16); m.wf4 = take(16 * 17); m.bf4 = take(16);
  m.wh2 = take(2 * 64 * 17); m.bh2 = take(32); m.wh3 = take(32 * 17); m.bh3 = take(16); m.wh4 = take(16 * 17); m.bh4 = take(16);
  m.total = off;
  if (m.total != bgm_causal_hmc_blob_floats(KT1, m.n_gh)) { bgm_set_error("bgm_causal_hmc: blob layout and bgm_causal_hmc_blob_floats disagree"); return BGM_E_STATE; }
  if ((size_t)m.total * 4 > 160 * 1024) { bgm_set_error("bgm_causal_hmc: the weights do not fit the 160 KiB LDS (" + std::to_string(m.total * 4) + " B)"); return BGM_E_UNSUPPORTED; }
  std::vector<float> hb((size_t)m.total, 0.0f);
  auto copy = [&](int s_off, int d_off, int count) { std::copy(gb.begin() + s_off, gb.begin() + s_off + count, hb.begin() + d_off); };
  to_dual(gb, gm.w1g, hb, m.w1g, KR1, 4); to_dual(gb, gm.w1f, hb, m.w1f, KR1, 4); to_dual(gb, gm.w1h, hb, m.w1h, KR1, 4);
  copy(gm.b1g, m.b1g, 64); copy(gm.b1f, m.b1f, 64); copy(gm.b1h, m.b1h, 64);
  for (int l = 0; l < m.n_gh; ++l) to_dual(gb, gm.wg + l * 4096, hb, m.wg + l * CHMC_W64, 64, 4);
  copy(gm.bg, m.bg, m.n_gh * 64);
  to_dual(gb, gm.wgl, hb, m.gram, 64, 4);
  copy(gm.bgl, m.ga, 132);
  to_dual(gb, gm.wf2, hb, m.wf2, 64, 2); copy(gm.bf2, m.bf2, 32);
  to_dual(gb, gm.wf3, hb, m.wf3, 32, 1); copy(gm.bf3, m.bf3, 16);
  to_dual(gb, gm.wf4, hb, m.wf4, 16, 1); copy(gm.bf4, m.bf4, 16);
  to_dual(gb, gm.wh2, hb, m.wh2, 64, 2); copy(gm.bh2, m.bh2, 32);
  to_dual(gb, gm.wh3, hb, m.wh3, 32, 1); copy(gm.bh3, m.bh3, 16);
  to_dual(gb, gm.wh4, hb, m.wh4, 16, 1); copy(gm.bh4, m.bh4, 16);
  if (int rc = bgm_reserve(st->blob_dev, st->blob_cap, hb.size())) return rc;
  BGM_HIP_CHECK(hipMemcpyAsync(st->blob_dev, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice, stream));
  BGM_HIP_CHECK(hipStreamSynchronize(stream));      // stack-local staging buffer
  h->hmc_valid = true;
  return BGM_OK;
}

}  // namespace

int bgm_causal_hmc_check(bgm_handle *h, const char *who) {
  if (!h || !h->configured) { bgm_set_error(std::string(who) + ": handle not configured"); return BGM_E_STATE; }
  if (const char *path = refused_path(h)) { bgm_set_error(std::string(who) + ": the gradient / HMC kernels do not exist for " + path); return BGM_E_UNSUPPORTED; }
  return BGM_OK;
}

void bgm_causal_hmc_free(bgm_handle *h) {
  HmcState *st = static_cast<HmcState *>(h->hmc_state);
  if (!st) return;
  if (st->blob_dev) hipFree(st->blob_dev);
  delete st;
  h->hmc_state = nullptr;
  h->hmc_valid = false;
}

extern "C" int bgm_causal_logpost_grad(bgm_handle *h, const float *x, const float *y, const float *v, const float *z, int64_t n,
                                       float *out_logp, float *out_grad, void *stream_) {
  if (int rc = bgm_causal_hmc_check(h, "bgm_causal_logpost_grad")) return rc;
  if (n <= 0) return BGM_OK;
  if (!x || !y || !v || !z || !out_logp || !out_grad) { bgm_set_error("bgm_causal_logpost_grad: NULL pointer"); return BGM_E_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  HmcState *st = nullptr;
  if (int rc = hmc_prepare(h, v, n, stream, st)) return rc;
  const int grid = bgm_causal_grid(h, n, 1);
  if (h->hmc_partial) return bgm_causal_hmc_obs_logpost(h, st, x, y, z, n, out_logp, out_grad, grid, stream);      // bgm_causal_hmc_set_partial
  return bgm_causal_dispatch(h, "log-posterior gradient kernel", [&](auto s) {
    using S = decltype(s);
    return bgm_launch(causal_hmc_logpost_kernel<S::KT1, MH_WAVES>, grid, MH_WAVES, st->m.total * 4, stream, st->blob_dev, st->m, x, y,
                      h->uc_dev, z, (long long)n, out_logp, out_grad);
  });
}

int bgm_causal_hmc_args(bgm_handle *h, const char *who_, const CausalHmcCall &c, CausalHmcLaunch &l) {
  const std::string who(who_);
  if (!c.x || !c.y || !c.v || !c.state || !c.logp || !c.grad || !c.step) { bgm_set_error(who + ": NULL data pointer"); return BGM_E_INVALID; }
  if (c.n_leapfrog < 1) { bgm_set_error(who + ": n_leapfrog must be >= 1"); return BGM_E_INVALID; }
  if (c.it_begin < 0 || c.burn_in < 0) { bgm_set_error(who + ": it_begin / burn_in must be >= 0"); return BGM_E_INVALID; }
  if (c.row_base < 0 || c.row_base + c.n > 0xFFFFFFFFll) { bgm_set_error(who + ": row index exceeds the 32-bit RNG counter"); return BGM_E_INVALID; }
  if (c.up || c.dn) {
    if (!c.up || !c.dn || c.n_table < 0) { bgm_set_error(who + ": up_dev / dn_dev must both hold n_table >= 0 factors"); return BGM_E_INVALID; }
    if (!(c.s_min > 0.0f) || !(c.s_max >= c.s_min) || !(c.s_max < INFINITY)) { bgm_set_error(who + ": the clamp needs 0 < s_min <= s_max < inf"); return BGM_E_INVALID; }
  }
  if (c.draws && (long long)c.it_begin + c.n_iters - c.burn_in > c.n_keep) { bgm_set_error(who + ": iterations beyond burn_in + n_keep"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  HmcState *st = nullptr;
  if (int rc = hmc_prepare(h, c.v, c.n, c.stream, st)) return rc;
  const CausalHmcMassArgs &ma = st->mass;      // bgm_causal_hmc_set_mass
  if (ma.scale && ma.accumulate && (!ma.ref || !ma.s1 || !ma.s2)) { bgm_set_error("HMC metric: launched without its buffers"); return BGM_E_STATE; }
  CausalHmcKArgs &ka = l.ka;
  ka = CausalHmcKArgs{};
  ka.blob = st->blob_dev; ka.x = c.x; ka.y = c.y; ka.uc = h->uc_dev; ka.n = c.n; ka.row_base = c.row_base;
  ka.state = c.state; ka.logp = c.logp; ka.grad = c.grad; ka.step = c.step;
  ka.up = c.up; ka.dn = c.dn; ka.n_table = c.up ? c.n_table : 0; ka.s_min = c.s_min; ka.s_max = c.s_max;
  ka.init = c.init ? 1 : 0; ka.it_begin = c.it_begin; ka.n_iters = c.n_iters; ka.burn_in = c.burn_in; ka.n_leapfrog = c.n_leapfrog;
  ka.k0 = (unsigned)(c.seed & 0xFFFFFFFFull); ka.k1 = (unsigned)(c.seed >> 32);
  ka.acc_count = c.acc_count; ka.draws = c.draws; ka.m = st->m;
  l.st = st;
  l.grid = bgm_causal_grid(h, c.n, 1);
  l.lds = st->m.total * 4;
  l.stream = c.stream;
  return BGM_OK;
}

extern "C" int bgm_causal_hmc_run(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base, float *state,
                                  float *logp, float *grad, float *step, const float *up, const float *dn, int32_t n_table, float s_min,
                                  float s_max, int32_t init, int32_t it_begin, int32_t n_iters, int32_t burn_in, int32_t n_leapfrog,
                                  uint64_t seed, uint32_t *acc_count, float *draws, int32_t n_keep, void *stream_) {
  if (int rc = bgm_causal_hmc_check(h, "bgm_causal_hmc_run")) return rc;
  if (n <= 0 || n_iters <= 0) return BGM_OK;
  CausalHmcLaunch l{};
  if (int rc = bgm_causal_hmc_args(h, "bgm_causal_hmc_run", BGM_CAUSAL_HMC_CALL, l)) return rc;
  if (l.st->traj_set()) return bgm_causal_hmc_traj_launch(h, l);      // bgm_causal_hmc_set_trajectory
  if (h->hmc_partial) return bgm_causal_hmc_obs_launch(h, l);      // bgm_causal_hmc_set_partial
  if (l.st->mass.scale) return bgm_causal_hmc_mass_launch(h, l);      // bgm_causal_hmc_set_mass
  return bgm_causal_dispatch(h, "HMC kernel", [&](auto s) {
    using S = decltype(s);
    return bgm_launch(causal_hmc_kernel<S::KT1, MH_WAVES>, l.grid, MH_WAVES, l.lds, l.stream, l.ka);
  });
}
