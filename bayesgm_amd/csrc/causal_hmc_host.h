// causal_hmc_host.h -- host state of the CausalBGM HMC latent sampler, shared by causal_hmc_api.hip (identity mass) and
// causal_hmc_mass_api.hip (the diagonal metric per chain).  Host only.
#pragma once
#include "bgm_host.h"
#include "causal_hmc_mass_kernels.h"

// bgm_handle::hmc_state
struct HmcState {
  float *blob_dev = nullptr;       // the dual-access copy of the Gram blob
  size_t blob_cap = 0;
  CausalHmcMeta m{};
  CausalHmcMassArgs mass{};        // bgm_causal_hmc_set_mass; scale = NULL: identity mass
};

static inline HmcState *bgm_causal_hmc_state(bgm_handle *h) {
  if (!h->hmc_state) h->hmc_state = new HmcState();
  return static_cast<HmcState *>(h->hmc_state);
}

// BGM_E_STATE for an unconfigured handle, BGM_E_UNSUPPORTED (naming the path) where the gradient / HMC kernels do not exist
int bgm_causal_hmc_check(bgm_handle *h, const char *who);                                                     // causal_hmc_api.hip
int bgm_causal_hmc_mass_launch(bgm_handle *h, const CausalHmcKArgs &ka, const CausalHmcMassArgs &ma, int grid, int lds,
                               hipStream_t stream);                                                           // causal_hmc_mass_api.hip
