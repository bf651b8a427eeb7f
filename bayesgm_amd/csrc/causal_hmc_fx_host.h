// causal_hmc_fx_host.h -- what the entry points of the HMC kernels with the effect pass inside share on the host: the prologue of
// bgm_causal_hmc_run_effects, _run_group_effects (bgm_causal_hmc_begin) and of the four per-row ones, _run_row_effects, _row_tails,
// _row_contrasts and _row_choice (bgm_causal_hmc_rows_begin), and the preparation of their launch (bgm_causal_hmc_fx_prepare).  An
// entry point is: begin, its own argument checks, prepare, its own kernel arguments, launch (bgm_causal_hmc_launch_pair,
// causal_hmc_host.h) -- in that order, which is the order in which a call with several mistakes reports them.  Host only.
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

// What every entry point with an effect pass does first: the handle / path check, the empty call (go = false with BGM_OK: done,
// return), and -- `traj_kernels` names the kernels of an entry point that has no TRAJ twins, NULL for one that has -- the refusal
// of a trajectory option.  go = true with BGM_OK: go on.
static inline int bgm_causal_hmc_begin(bgm_handle *h, const char *who, int64_t n, int32_t n_iters, const char *traj_kernels, bool &go) {
  go = false;
  if (int rc = bgm_causal_hmc_check(h, who)) return rc;
  if (n <= 0 || n_iters <= 0) return BGM_OK;
  if (traj_kernels)
    if (int rc = bgm_causal_hmc_traj_refuse(h, who, traj_kernels)) return rc;
  go = true;
  return BGM_OK;
}

// ... and the four per-row entry points after it: a continuous treatment, the dose grid and the moments of the curve
static inline int bgm_causal_hmc_rows_begin(bgm_handle *h, const char *who_, int64_t n, int32_t n_iters, const char *traj_kernels,
                                            const float *x_values, int32_t n_doses, const float *row_moments, bool &go) {
  if (int rc = bgm_causal_hmc_begin(h, who_, n, n_iters, traj_kernels, go); rc || !go) return rc;
  go = false;
  const std::string who(who_);
  if (h->cfg.binary_treatment != 0) {
    bgm_set_error(who + ": a binary treatment has its per-row effect already: bgm_causal_hmc_run_effects (BGM_EFFECT_ITE)");
    return BGM_E_INVALID;
  }
  if (!x_values || n_doses <= 0 || !row_moments) { bgm_set_error(who + ": x_values / row_moments required"); return BGM_E_INVALID; }
  go = true;
  return BGM_OK;
}

// After begin and the entry point's own argument checks: n_keep / it_begin / burn_in, the sampling blob, the LDS budget refusal
// (naming the bytes, before the panel's pre-pass or any kernel of the sampler is launched), bgm_causal_hmc_args, then fx.sblob /
// src / dst / cnt / mf / n_keep, the three fields every effect pass reads (sample_y, n_doses: the stride of a slot, x_values) and
// the LDS bytes of the launch.  The caller fills in the rest of fx.
static inline int bgm_causal_hmc_fx_prepare(bgm_handle *h, const char *who_, const CausalHmcCall &c, int32_t sample_y, int32_t n_doses,
                                            const float *x_values, CausalHmcLaunch &l, CausalHmcFxArgs &fx) {
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
  fx.sample_y = sample_y; fx.n_doses = n_doses; fx.x_values = x_values;
  return BGM_OK;
}
