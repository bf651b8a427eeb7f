// causal_hmc_obs_host.h -- what the HMC entry points call while bgm_causal_hmc_set_partial is on (bgm_handle::hmc_partial): the
// launches of the OBS kernels (causal_hmc_obs_kernels.h), all of which live in causal_hmc_obs_api.hip.  The entry points check their
// arguments and build the kernel arguments as always; only the kernel differs.  Host only.
#pragma once
#include "causal_hmc_host.h"
#include "causal_hmc_rowfx_kernels.h"

int bgm_causal_hmc_obs_logpost(bgm_handle *h, const HmcState *st, const float *x, const float *y, const float *z, int64_t n, float *out_logp,
                               float *out_grad, int grid, hipStream_t stream);                                 // bgm_causal_logpost_grad
int bgm_causal_hmc_obs_launch(bgm_handle *h, const CausalHmcLaunch &l);                                       // bgm_causal_hmc_run
int bgm_causal_hmc_obs_ite_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx);        // bgm_causal_hmc_run_effects, binary
int bgm_causal_hmc_obs_rowfx_launch(bgm_handle *h, const CausalHmcLaunch &l, const CausalHmcFxArgs &fx,
                                    const CausalHmcRowFxArgs &rf);                                            // bgm_causal_hmc_run_row_effects
