// sdr_api.hip -- moments of a covariate panel for the latent-dimension estimate (SIR + PCA).
//
// replaces (src/bayesgm/utils/helpers.py): the two economic QRs of get_SDR_dim (:140-179) and the PCA of
// estimate_latent_dims (:181-222) are restated on the centred Gram, the column sums and the per-slice column sums of V
// (bayesgm_amd/latent_dims.py); this unit computes those in one read of V -> sdr_moments_kernel + sdr_reduce_kernel.
#include <algorithm>
#include <string>

#include "bgm_host.h"
#include "sdr_kernels.h"

namespace {

constexpr int SDR_MAX_P = 2048;
constexpr int SDR_MAX_SLICES = 1024;

struct SdrPlan {
  SdrShape s;
  int n_wg;            // workgroups over the rows (gridDim.x)
  int n_groups;        // workgroups over the output tiles (gridDim.y)
  size_t lds_bytes;
  long long ws_bytes;
};

int sdr_plan(const bgm_handle *h, int64_t n, int32_t p, int32_t s0, int32_t s1, SdrPlan &pl) {
  if (n < 0 || p <= 0 || s0 < 0 || s1 < 0) { bgm_set_error("bgm_sdr_moments: bad shape"); return BGM_E_INVALID; }
  if (p > SDR_MAX_P) {
    bgm_set_error("bgm_sdr_moments: p = " + std::to_string(p) + " exceeds the limit p <= " + std::to_string(SDR_MAX_P));
    return BGM_E_UNSUPPORTED;
  }
  if (s0 > SDR_MAX_SLICES || s1 > SDR_MAX_SLICES) {
    bgm_set_error("bgm_sdr_moments: " + std::to_string(std::max(s0, s1)) + " slices exceed the limit of " + std::to_string(SDR_MAX_SLICES) +
                  " slices per labeling");
    return BGM_E_UNSUPPORTED;
  }
  SdrShape &s = pl.s;
  s.n = n; s.p = p; s.pb = (p + 15) / 16; s.s0 = s0; s.s1 = s1;
  s.eb = (1 + s0 + s1 + 15) / 16;
  s.n_tasks = sdr_n_tasks(s.pb, s.eb);
  const int P = 16 * s.pb;
  s.kr = std::min(SDR_MAX_KR, SDR_ROWS_BYTES / (8 * (P + 1)) / 8 * 8);   // >= 8 for P <= 2048
  pl.n_groups = (s.n_tasks + SDR_WAVES - 1) / SDR_WAVES;
  // one 8-wave workgroup per CU (up to ~150 KiB of LDS): split the rows so that groups x row ranges ~ one workgroup per CU
  const long long chunks = std::max<long long>(1, (n + s.kr - 1) / s.kr);
  long long want = std::max<long long>(1, (long long)std::max(h->n_cus, 1) / pl.n_groups);
  want = std::min(want, chunks);
  s.rows_per_wg = (chunks + want - 1) / want * s.kr;
  pl.n_wg = (int)std::max<long long>(1, (n + s.rows_per_wg - 1) / s.rows_per_wg);
  s.ldv = p;
  pl.lds_bytes = (size_t)s.kr * (P + 1) * 8 + (size_t)P * 8 + (size_t)2 * s.kr * 4;
  pl.ws_bytes = (long long)pl.n_wg * s.n_tasks * SDR_TPW * 256 * 8;
  return BGM_OK;
}

}  // namespace

extern "C" int bgm_sdr_moments_workspace(bgm_handle *h, int64_t n, int32_t p, int32_t n_slices0, int32_t n_slices1, int64_t *bytes) {
  if (!h || !bytes) { bgm_set_error("bgm_sdr_moments_workspace: bad argument"); return BGM_E_INVALID; }
  SdrPlan pl;
  const int rc = sdr_plan(h, n, p, n_slices0, n_slices1, pl);
  if (rc != BGM_OK) return rc;
  *bytes = pl.ws_bytes;
  return BGM_OK;
}

extern "C" int bgm_sdr_moments(bgm_handle *h, const void *v_dev, int32_t v_is_f64, int64_t n, int32_t p, int64_t ldv,
                               const double *shift_dev, const int32_t *labels0_dev, int32_t n_slices0, const int32_t *labels1_dev,
                               int32_t n_slices1, double *out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream_) {
  if (!h || !out_dev || (n > 0 && !v_dev) || ldv < p || (n_slices0 > 0 && n > 0 && !labels0_dev) ||
      (n_slices1 > 0 && n > 0 && !labels1_dev)) {
    bgm_set_error("bgm_sdr_moments: bad argument");
    return BGM_E_INVALID;
  }
  SdrPlan pl;
  const int rc = sdr_plan(h, n, p, n_slices0, n_slices1, pl);
  if (rc != BGM_OK) return rc;
  pl.s.ldv = ldv;
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  const size_t out_count = (size_t)(1 + n_slices0 + n_slices1) * p + (size_t)p * p;
  if (n == 0) {
    BGM_HIP_CHECK(hipMemsetAsync(out_dev, 0, out_count * 8, stream));
    return BGM_OK;
  }
  if (!workspace_dev || workspace_bytes < pl.ws_bytes) {
    bgm_set_error("bgm_sdr_moments: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(pl.ws_bytes) +
                  " needed (bgm_sdr_moments_workspace)");
    return BGM_E_INVALID;
  }
  const int *l0 = n_slices0 > 0 ? labels0_dev : nullptr, *l1 = n_slices1 > 0 ? labels1_dev : nullptr;
  double *ws = static_cast<double *>(workspace_dev);
  if (v_is_f64) {
    BGM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(sdr_moments_kernel<double>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
    hipLaunchKernelGGL(sdr_moments_kernel<double>, dim3(pl.n_wg, pl.n_groups), dim3(64 * SDR_WAVES), pl.lds_bytes, stream,
                       static_cast<const double *>(v_dev), shift_dev, l0, l1, pl.s, ws);
  } else {
    BGM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(sdr_moments_kernel<float>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
    hipLaunchKernelGGL(sdr_moments_kernel<float>, dim3(pl.n_wg, pl.n_groups), dim3(64 * SDR_WAVES), pl.lds_bytes, stream,
                       static_cast<const float *>(v_dev), shift_dev, l0, l1, pl.s, ws);
  }
  BGM_HIP_CHECK(hipGetLastError());
  const long long total = (long long)pl.s.n_tasks * SDR_TPW * 256;
  hipLaunchKernelGGL(sdr_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ws, pl.s, pl.n_wg, out_dev);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
