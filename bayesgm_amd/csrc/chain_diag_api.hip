// chain_diag_api.hip -- MCMC chain diagnostics (split R-hat, effective sample size) of sampled draws.
//
// New ground: the reference prints an acceptance rate and has no per-chain diagnostic.  The formulas are the Stan / ArviZ "mean"
// forms without rank normalisation (include/bgm_hip.h) -> chain_diag_means_kernel + chain_diag_acov_kernel.
#include <algorithm>
#include <string>

#include "bgm_host.h"
#include "chain_diag_kernels.h"

namespace {

struct ChainDiagPlan {
  ChainDiagShape s;
  int threads;
  size_t lds_bytes;
  long long ws_bytes;
};

int chain_diag_plan(int32_t n_chains, int32_t n_draws, int64_t n_series, int32_t max_lag, ChainDiagPlan &pl) {
  if (n_series < 0) { bgm_set_error("bgm_chain_diagnostics: n_series < 0"); return BGM_E_INVALID; }
  if (n_draws < 8) {
    bgm_set_error("bgm_chain_diagnostics: n_draws = " + std::to_string(n_draws) + ", at least 8 draws per chain are needed");
    return BGM_E_INVALID;
  }
  if (n_chains < 1 || n_chains > CD_MAX_CHAINS) {
    bgm_set_error("bgm_chain_diagnostics: n_chains = " + std::to_string(n_chains) + " outside the supported 1 .. " + std::to_string(CD_MAX_CHAINS));
    return n_chains < 1 ? BGM_E_INVALID : BGM_E_UNSUPPORTED;
  }
  if (max_lag < 1 || max_lag > CD_MAX_LAG) {
    bgm_set_error("bgm_chain_diagnostics: max_lag = " + std::to_string(max_lag) + " outside the supported 1 .. " + std::to_string(CD_MAX_LAG));
    return max_lag < 1 ? BGM_E_INVALID : BGM_E_UNSUPPORTED;
  }
  if (n_series > (int64_t)CD_TILE * 0x7fffffff) { bgm_set_error("bgm_chain_diagnostics: too many series"); return BGM_E_UNSUPPORTED; }
  ChainDiagShape &s = pl.s;
  s.n_series = n_series; s.n_chains = n_chains; s.n_draws = n_draws;
  s.h = n_draws / 2; s.m = 2 * n_chains;
  s.max_lag = std::min(max_lag, n_draws / 2 - 1);
  s.n_lags = 2 * ((s.max_lag + 1) / 2);                 // the pairs (2j, 2j + 1) with 2j + 1 <= max_lag
  s.groups = (s.n_lags + CD_LG - 1) / CD_LG;
  s.look = CD_LG * s.groups + CD_LT;
  // rows of the LDS image: lookahead + chunk.  Up to 16 lag groups (256 threads) three workgroups share a CU; beyond, one does.
  const int chunk = s.groups <= 16 ? 128 : 96;
  s.chunk = std::min(chunk, (s.h + CD_LT - 1) / CD_LT * CD_LT);
  pl.threads = CD_TILE * s.groups;
  pl.lds_bytes = ((size_t)(s.look + s.chunk) * CD_PITCH + CD_TILE) * sizeof(double);
  pl.ws_bytes = (long long)(s.m + 1) * n_series * (long long)sizeof(double);
  return BGM_OK;
}

}  // namespace

extern "C" int bgm_chain_diagnostics_workspace(bgm_handle *h, int32_t n_chains, int32_t n_draws, int64_t n_series, int32_t max_lag,
                                               int64_t *bytes) {
  if (!h || !bytes) { bgm_set_error("bgm_chain_diagnostics_workspace: bad argument"); return BGM_E_INVALID; }
  ChainDiagPlan pl;
  const int rc = chain_diag_plan(n_chains, n_draws, n_series, max_lag, pl);
  if (rc != BGM_OK) return rc;
  *bytes = pl.ws_bytes;
  return BGM_OK;
}

extern "C" int bgm_chain_diagnostics(bgm_handle *h, const float *draws_dev, int32_t n_chains, int32_t n_draws, int64_t n_series,
                                     int32_t max_lag, double *out_dev, int32_t *flags_dev, void *workspace_dev, int64_t workspace_bytes,
                                     void *stream_) {
  if (!h) { bgm_set_error("bgm_chain_diagnostics: bad argument"); return BGM_E_INVALID; }
  ChainDiagPlan pl;
  const int rc = chain_diag_plan(n_chains, n_draws, n_series, max_lag, pl);
  if (rc != BGM_OK) return rc;
  if (n_series == 0) return BGM_OK;
  if (!draws_dev || !out_dev || !flags_dev) { bgm_set_error("bgm_chain_diagnostics: bad argument"); return BGM_E_INVALID; }
  if (!workspace_dev || workspace_bytes < pl.ws_bytes) {
    bgm_set_error("bgm_chain_diagnostics: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(pl.ws_bytes) +
                  " needed (bgm_chain_diagnostics_workspace)");
    return BGM_E_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  double *ws = static_cast<double *>(workspace_dev);
  hipLaunchKernelGGL(chain_diag_means_kernel, dim3((unsigned)((n_series + 255) / 256)), dim3(256), 0, stream, draws_dev, pl.s, out_dev,
                     flags_dev, ws);
  BGM_HIP_CHECK(hipGetLastError());
  const unsigned tiles = (unsigned)((n_series + CD_TILE - 1) / CD_TILE);
  BGM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(chain_diag_acov_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)pl.lds_bytes));
  hipLaunchKernelGGL(chain_diag_acov_kernel, dim3(tiles), dim3(pl.threads), pl.lds_bytes, stream, draws_dev, pl.s, out_dev, flags_dev, ws);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
