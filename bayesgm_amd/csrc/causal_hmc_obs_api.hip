// causal_hmc_obs_api.hip -- bgm_causal_hmc_set_partial (include/bgm_hip.h) and the launches of the CausalBGM gradient / HMC kernels for
// partially observed rows (causal_hmc_obs_kernels.h: the OBS instantiations of chmc_logpost_run and chmc_run), in a translation
// unit of their own, compiled beside those of the other HMC entry points: bgm_causal_logpost_grad, bgm_causal_hmc_run,
// bgm_causal_hmc_run_effects and bgm_causal_hmc_run_row_effects come here only while the option is on.
// Each launch is bgm_causal_hmc_launch_pair (causal_hmc_host.h) with the two kernels of this unit that it names.
// replaces: nothing in causalbgm/base.py; the reference's predict needs the outcome of every row.
#include <string>

#include "causal_launch.h"
#include "causal_hmc_obs_host.h"
#include "causal_hmc_obs_kernels.h"

extern "C" int bgm_causal_hmc_set_partial(bgm_handle *h, int32_t on) {
  if (!h) { bgm_set_error("bgm_causal_hmc_set_partial: NULL handle"); return BGM_E_INVALID; }
  if (!on) { h->hmc_partial = false; return BGM_OK; }
  if (int rc = bgm_causal_hmc_check(h, "bgm_causal_hmc_set_partial")) return rc;
  h->hmc_partial = true;
  return BGM_OK;
}

int bgm_causal_hmc_obs_logpost(bgm_handle *h, const HmcState *st, const float *x, const float *y, const float *z, int64_t n, float *out_logp,
                               float *out_grad, int grid, hipStream_t stream) {
  return bgm_causal_dispatch(h, "log-posterior gradient kernel for partially observed rows", [&](auto s) {
    using S = decltype(s);
    return bgm_launch(causal_hmc_obs_logpost_kernel<S::KT1, MH_WAVES>, grid, MH_WAVES, st->m.total * 4, stream, st->blob_dev, st->m, x, y,
                      h->uc_dev, z, (long long)n, out_logp, out_grad);
  });
}

int bgm_causal_hmc_obs_launch(bgm_handle *h, const CausalHmcLaunch &l) {
  return bgm_causal_hmc_launch_pair(h, l, "HMC kernel for partially observed rows",
                                    [](auto s) { return causal_hmc_obs_kernel<decltype(s)::KT1, MH_WAVES>; },
                                    [](auto s) { return causal_hmc_obs_mass_kernel<decltype(s)::KT1, MH_WAVES>; });
}

int bgm_causal_hmc_obs_ite_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx) {
  return bgm_causal_hmc_launch_pair(
      h, l, "HMC kernel with fused effects for partially observed rows",
      [](auto s) { using S = decltype(s); return causal_hmc_obs_ite_kernel<S::KT1, S::KSL1, MH_WAVES>; },
      [](auto s) { using S = decltype(s); return causal_hmc_obs_mass_ite_kernel<S::KT1, S::KSL1, MH_WAVES>; }, fx);
}

int bgm_causal_hmc_obs_rowfx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx, const CausalHmcRowFxArgs &rf) {
  return bgm_causal_hmc_launch_pair(
      h, l, "HMC kernel with per-row effects for partially observed rows",
      [](auto s) { using S = decltype(s); return causal_hmc_obs_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES>; },
      [](auto s) { using S = decltype(s); return causal_hmc_obs_mass_rowfx_kernel<S::KT1, S::KSL1, MH_WAVES>; }, fx, rf);
}
