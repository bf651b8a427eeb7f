// causal_hmc_fx_api.hip -- bgm_causal_hmc_run_effects (include/bgm_hip.h): the CausalBGM HMC latent sampler with the effect pass
// fused into the retained iterations (causal_hmc_fx_kernels.h), in a translation unit of its own.  The paths without effects
// (causal_hmc_api.hip, causal_hmc_mass_api.hip) are untouched: bgm_causal_hmc_run never comes here.
// replaces: nothing in causalbgm/base.py; infer_from_latent_posterior (:671-763) runs there on stored MH draws.
#include <string>

#include "causal_launch.h"
#include "causal_hmc_host.h"
#include "causal_hmc_fx_kernels.h"

namespace {

const char *WHO = "bgm_causal_hmc_run_effects";

// f's part of the sampling blob behind the HMC blob: where the pieces come from (h->meta), where they go and the rebased meta
void fx_layout(const bgm_handle *h, CausalHmcFxArgs &fx) {
  const CausalMeta &sm = h->meta;
  const int tail = sm.bf4 + 16 - sm.wf2;      // wf2, bf2, wf3, bf3, wf4, bf4 are consecutive in the sampling blob
  const int src[CHMC_FX_PIECES] = {sm.w1f, sm.b1f, sm.wf2, sm.wxf}, cnt[CHMC_FX_PIECES] = {16 * h->KT1 * 64, 64, tail, 64};
  int off = 0;
  for (int p = 0; p < CHMC_FX_PIECES; ++p) {
    fx.src[p] = src[p]; fx.dst[p] = off; fx.cnt[p] = cnt[p];
    off += cnt[p];
  }
  CausalMeta &mf = fx.mf;
  mf = CausalMeta{};
  mf.q = sm.q; mf.p = sm.p; mf.binary = sm.binary; mf.sig2_y = sm.sig2_y; mf.l1b = sm.l1b;
  mf.w1f = fx.dst[0]; mf.b1f = fx.dst[1];
  const int shift = fx.dst[2] - sm.wf2;
  mf.wf2 = sm.wf2 + shift; mf.bf2 = sm.bf2 + shift; mf.wf3 = sm.wf3 + shift; mf.bf3 = sm.bf3 + shift; mf.wf4 = sm.wf4 + shift; mf.bf4 = sm.bf4 + shift;
  mf.wxf = fx.dst[3];
  mf.total = off;
}

template <int EFFECT>
int launch_fx(bgm_handle *h, const CausalHmcKArgs &ka, const CausalHmcMassArgs &ma, const CausalHmcFxArgs &fx, int grid, int lds, hipStream_t stream) {
  if (ma.scale)
    return bgm_causal_dispatch(h, "HMC kernel with a diagonal metric and fused effects", [&](auto s) {
      using S = decltype(s);
      return bgm_launch(causal_hmc_mass_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT>, grid, MH_WAVES, lds, stream, ka, ma, fx);
    });
  return bgm_causal_dispatch(h, "HMC kernel with fused effects", [&](auto s) {
    using S = decltype(s);
    return bgm_launch(causal_hmc_fx_kernel<S::KT1, S::KSL1, MH_WAVES, EFFECT>, grid, MH_WAVES, lds, stream, ka, fx);
  });
}

}  // namespace

extern "C" int bgm_causal_hmc_run_effects(bgm_handle *h, const float *x, const float *y, const float *v, int64_t n, int64_t row_base,
                                          float *state, float *logp, float *grad, float *step, const float *up, const float *dn,
                                          int32_t n_table, float s_min, float s_max, int32_t init, int32_t it_begin, int32_t n_iters,
                                          int32_t burn_in, int32_t n_leapfrog, uint64_t seed, uint32_t *acc_count, float *draws,
                                          int32_t n_keep, int32_t sample_y, const float *x_values, int32_t n_doses, float *adrf_partial,
                                          float *ite, void *stream_) {
  if (int rc = bgm_causal_hmc_check(h, WHO)) return rc;
  if (n <= 0 || n_iters <= 0) return BGM_OK;
  const std::string who(WHO);
  const bool binary = h->cfg.binary_treatment != 0;
  if (binary && !ite) { bgm_set_error(who + ": ite_dev required for binary treatment"); return BGM_E_INVALID; }
  if (!binary && (!x_values || n_doses <= 0 || !adrf_partial)) { bgm_set_error(who + ": x_values / adrf_partial required"); return BGM_E_INVALID; }
  if (n_keep <= 0 || (long long)it_begin + n_iters - burn_in > n_keep) { bgm_set_error(who + ": iterations beyond burn_in + n_keep"); return BGM_E_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  if (int rc = bgm_causal_sampling_blob(h, stream)) return rc;
  // the LDS budget is known from the shape: refuse before the panel's pre-pass or any kernel of the sampler is launched
  const size_t lds = ((size_t)bgm_causal_hmc_blob_floats(h->KT1, h->meta.n_gh) + chmc_fx_floats(h->KT1)) * 4;
  if (lds > 160 * 1024) {
    bgm_set_error(who + ": the HMC weights with f's part of the sampling blob do not fit the 160 KiB LDS (" + std::to_string(lds) +
                  " B); use the draws route: bgm_causal_hmc_run with draws_dev, then bgm_causal_effects");
    return BGM_E_UNSUPPORTED;
  }
  CausalHmcKArgs ka{};
  HmcState *st = nullptr;
  int grid = 0;
  if (int rc = bgm_causal_hmc_args(h, WHO, x, y, v, n, row_base, state, logp, grad, step, up, dn, n_table, s_min, s_max, init, it_begin, n_iters,
                                   burn_in, n_leapfrog, seed, acc_count, draws, n_keep, stream, ka, st, grid))
    return rc;
  const CausalHmcMassArgs &ma = st->mass;      // bgm_causal_hmc_set_mass
  if (ma.scale && ma.accumulate && (!ma.ref || !ma.s1 || !ma.s2)) { bgm_set_error("HMC metric: launched without its buffers"); return BGM_E_STATE; }
  CausalHmcFxArgs fx{};
  fx_layout(h, fx);
  if (fx.mf.total != chmc_fx_floats(h->KT1) || (size_t)(st->m.total + fx.mf.total) * 4 != lds) { bgm_set_error(who + ": LDS layout disagrees with its byte count"); return BGM_E_STATE; }
  fx.sblob = h->sblob_dev;
  fx.n_keep = n_keep; fx.sample_y = sample_y; fx.n_doses = binary ? 2 : n_doses;
  fx.x_values = x_values; fx.adrf_partial = adrf_partial; fx.ite = ite;
  return binary ? launch_fx<2>(h, ka, ma, fx, grid, (int)lds, stream) : launch_fx<1>(h, ka, ma, fx, grid, (int)lds, stream);
}
