// causal_hmc_fx_host.h -- what the entry points of the HMC kernels with the effect pass inside share on the host:
// bgm_causal_hmc_run_effects (causal_hmc_fx_api.hip) and bgm_causal_hmc_run_row_effects (causal_hmc_rowfx_api.hip).  Host only.
#pragma once
#include <string>

#include "causal_hmc_host.h"
#include "causal_hmc_fx_kernels.h"

// f's part of the sampling blob behind the HMC blob: where the pieces come from (h->meta), where they go and the rebased meta
static inline void bgm_causal_hmc_fx_layout(const bgm_handle *h, CausalHmcFxArgs &fx) {
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

// After bgm_causal_hmc_check and the entry point's own argument checks: n_keep / it_begin / burn_in, the sampling blob, the LDS
// budget refusal (naming the bytes, before the panel's pre-pass or any kernel of the sampler is launched), bgm_causal_hmc_args,
// then fx.sblob / src / dst / cnt / mf / n_keep and the LDS bytes of the launch.  The caller fills in the rest of fx.
static inline int bgm_causal_hmc_fx_prepare(bgm_handle *h, const char *who_, const CausalHmcCall &c, CausalHmcLaunch &l, CausalHmcFxArgs &fx) {
  const std::string who(who_);
  if (c.n_keep <= 0 || (long long)c.it_begin + c.n_iters - c.burn_in > c.n_keep) { bgm_set_error(who + ": iterations beyond burn_in + n_keep"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(h->device));
  if (int rc = bgm_causal_sampling_blob(h, c.stream)) return rc;
  // the LDS budget is known from the shape: refuse before the panel's pre-pass or any kernel of the sampler is launched
  const size_t lds = ((size_t)bgm_causal_hmc_blob_floats(h->KT1, h->meta.n_gh) + chmc_fx_floats(h->KT1)) * 4;
  if (lds > 160 * 1024) {
    bgm_set_error(who + ": the HMC weights with f's part of the sampling blob do not fit the 160 KiB LDS (" + std::to_string(lds) +
                  " B); use the draws route: bgm_causal_hmc_run with draws_dev, then bgm_causal_effects");
    return BGM_E_UNSUPPORTED;
  }
  if (int rc = bgm_causal_hmc_args(h, who_, c, l)) return rc;
  bgm_causal_hmc_fx_layout(h, fx);
  if (fx.mf.total != chmc_fx_floats(h->KT1) || (size_t)(l.st->m.total + fx.mf.total) * 4 != lds) { bgm_set_error(who + ": LDS layout disagrees with its byte count"); return BGM_E_STATE; }
  l.lds = (int)lds;
  fx.sblob = h->sblob_dev;
  fx.n_keep = c.n_keep;
  return BGM_OK;
}
