// bgm_impute_tails_api.hip -- BGM imputation inside the per-chain HMC sampler with the two TAILS of every missing cell kept beside its
// moments (bgm_bgm_hmc_run_rows_impute_tails, include/bgm_hip.h): the instantiations of bgm_hmc_rows_impute_tails_kernel
// (bgm_rowstep_kernels.h, STEP 4) for the six fp32 variants of bgm_launch.h at the wave counts of their bgm_hmc_rows_impute_kernel twins -- in
// a translation unit of their own, so that the kernels of bgm_impute_api.hip stay the code objects they were.  Opt-in: nothing else
// launches these kernels.
// replaces: np.quantile over the predictive draws of every missing cell in BGM.predict (bgm/base.py:527-663), without the draws: the
// buffers hold what bgm_row_tail_quantiles (aux_kernels.hip) reads.
#include <string>

#include "bgm_rowstep_host.h"
#include "bgm_launch.h"

extern "C" int bgm_bgm_hmc_run_rows_impute_tails(bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                                                 float s_min, float s_max, float max_trajectory, int32_t jitter, int32_t *n_steps_dev,
                                                 float *moments_dev, float *cells_dev, const int32_t *slot_dev, int32_t k_slots,
                                                 int32_t n_keep, int32_t add_noise, float *tails_dev, int32_t k_tail, void *stream_) {
  const std::string fn = "bgm_bgm_hmc_run_rows_impute_tails: ";
  const BgmTrajOpts traj{max_trajectory, jitter, n_steps_dev};
  const BgmImputeOpts opts{moments_dev, cells_dev, slot_dev, k_slots, n_keep, add_noise};
  bool go;
  int rc = bgm_hmc_impute_check(fn, h, a, up_dev, dn_dev, n_table, s_min, s_max, &traj, opts, &go);
  if (rc || !go) return rc;
  if (!tails_dev) { bgm_set_error(fn + "NULL pointer tails_dev"); return BGM_E_INVALID; }
  if (!slot_dev) { bgm_set_error(fn + "tails_dev needs slot_dev (the slot map gives every missing cell its series)"); return BGM_E_INVALID; }
  if (k_slots < 1) { bgm_set_error(fn + "tails_dev needs k_slots >= 1"); return BGM_E_INVALID; }
  if (k_tail < 1 || k_tail > n_keep) {
    bgm_set_error(fn + "k_tail must be in [1, n_keep = " + std::to_string(n_keep) + "]; got " + std::to_string(k_tail));
    return BGM_E_INVALID;
  }
  BgmState *s = bst(h);
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  rc = bgm_bgm_build_blob(h, stream);
  if (rc) return rc;
  BgmImputeTailsHmcKArgs ka{};
  bgm_hmc_impute_fill(ka, s, a, up_dev, dn_dev, n_table, s_min, s_max, &traj, opts);
  ka.tails = tails_dev; ka.k_tail = k_tail;
  const long long tiles = (a->n + 15) / 16;
  return bgm_bgm_dispatch(s, "BGM HMC with per-chain steps, fused imputation and tails", [&](auto v) {
    using V = decltype(v);
    constexpr int W = V::NTX == 0 ? BGM_WAVES_WIDE_HMC : BGM_WAVES;
    return bgm_launch(bgm_hmc_rows_impute_tails_kernel<V::KTQ, V::NTX, V::NH, W>, bgm_tile_grid(h, tiles, W), W, s->lds_bytes, stream, ka);
  });
}
