// bgm_impute_api.hip -- BGM imputation inside the per-chain HMC sampler (bgm_bgm_hmc_run_rows_impute, include/bgm_hip.h): the
// instantiations of bgm_hmc_rows_impute_kernel (bgm_rowstep_kernels.h, STEP 3) for the six fp32 variants of bgm_launch.h at the wave
// counts of their bgm_hmc_rows_traj_kernel twins -- in a translation unit of their own, so that the kernels of bgm_rowstep_api.hip stay
// the code objects they were.  Opt-in: nothing else launches these kernels.
// replaces: predict_on_posteriors over stored latent draws and the per-cell mean in BGM.predict (bgm/base.py:511-525, 527-663), for
// the missing cells only and as moments, not draws.
#include <string>

#include "bgm_rowstep_host.h"
#include "bgm_launch.h"
#include "gx_bgm_host.h"

extern "C" int bgm_bgm_hmc_run_rows_impute(bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                                           float s_min, float s_max, float max_trajectory, int32_t jitter, int32_t *n_steps_dev,
                                           float *moments_dev, float *cells_dev, const int32_t *slot_dev, int32_t k_slots, int32_t n_keep,
                                           int32_t add_noise, void *stream_) {
  const std::string fn = "bgm_bgm_hmc_run_rows_impute: ";
  const BgmTrajOpts traj{max_trajectory, jitter, n_steps_dev};
  const BgmImputeOpts opts{moments_dev, cells_dev, slot_dev, k_slots, n_keep, add_noise};
  bool go;
  int rc = bgm_hmc_impute_check(fn, h, a, up_dev, dn_dev, n_table, s_min, s_max, &traj, opts, &go);
  if (rc || !go) return rc;
  BgmState *s = bst(h);
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  rc = bgm_bgm_build_blob(h, stream);
  if (rc) return rc;
  BgmImputeHmcKArgs ka{};
  bgm_hmc_impute_fill(ka, s, a, up_dev, dn_dev, n_table, s_min, s_max, &traj, opts);
  const long long tiles = (a->n + 15) / 16;
  return bgm_bgm_dispatch(s, "BGM HMC with per-chain steps and fused imputation", [&](auto v) {
    using V = decltype(v);
    constexpr int W = V::NTX == 0 ? BGM_WAVES_WIDE_HMC : BGM_WAVES;
    return bgm_launch(bgm_hmc_rows_impute_kernel<V::KTQ, V::NTX, V::NH, W>, bgm_tile_grid(h, tiles, W), W, s->lds_bytes, stream, ka);
  });
}
