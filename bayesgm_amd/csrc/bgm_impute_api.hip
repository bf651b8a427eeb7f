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
  bool go;
  int rc = bgm_hmc_rows_check(fn, h, a, up_dev, dn_dev, n_table, s_min, s_max, &traj, &go);
  if (rc || !go) return rc;
  if (!moments_dev) { bgm_set_error(fn + "NULL pointer moments_dev"); return BGM_E_INVALID; }
  if (cells_dev && !slot_dev) { bgm_set_error(fn + "cells_dev needs slot_dev"); return BGM_E_INVALID; }
  if (cells_dev && k_slots < 1) { bgm_set_error(fn + "cells_dev needs k_slots >= 1"); return BGM_E_INVALID; }
  if (n_keep < 1) { bgm_set_error(fn + "n_keep must be >= 1"); return BGM_E_INVALID; }
  if (add_noise != 0 && add_noise != 1) { bgm_set_error(fn + "add_noise must be 0 or 1"); return BGM_E_INVALID; }
  if (a->burn_in < 0 || (long long)a->it_begin + a->n_iters > (long long)a->burn_in + n_keep) {
    bgm_set_error(fn + "it_begin + n_iters = " + std::to_string((long long)a->it_begin + a->n_iters) + " lies beyond burn_in + n_keep = " +
                  std::to_string((long long)a->burn_in + n_keep));
    return BGM_E_INVALID;
  }
  BgmState *s = bst(h);
  if (gxb_wanted(s)) {
    bgm_set_error(fn + "the fused imputation (predictive moments inside the per-chain HMC kernel) exists for trunks [64] x 3 / [64] x 5 "
                  "with z_dim <= 16; this shape runs on the general-width engine, which has the shared step and stored draws only");
    return BGM_E_UNSUPPORTED;
  }
  if (s->precision != 0) {
    bgm_set_error(fn + "the fused imputation (predictive moments inside the per-chain HMC kernel) is built for fp32 only, not for split "
                  "precision (f16x3): sample with bgm_bgm_hmc_run_rows and decode with bgm_bgm_predict_draws");
    return BGM_E_UNSUPPORTED;
  }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  rc = bgm_bgm_build_blob(h, stream);
  if (rc) return rc;
  BgmImputeHmcKArgs ka{};
  bgm_hmc_rows_fill(ka, s, a, up_dev, dn_dev, n_table, s_min, s_max, &traj, true);
  ka.moments = moments_dev; ka.cells = cells_dev; ka.slot = slot_dev; ka.k_slots = k_slots; ka.n_keep = n_keep; ka.add_noise = add_noise;
  const long long tiles = (a->n + 15) / 16;
  return bgm_bgm_dispatch(s, "BGM HMC with per-chain steps and fused imputation", [&](auto v) {
    using V = decltype(v);
    constexpr int W = V::NTX == 0 ? BGM_WAVES_WIDE_HMC : BGM_WAVES;
    return bgm_launch(bgm_hmc_rows_impute_kernel<V::KTQ, V::NTX, V::NH, W>, bgm_tile_grid(h, tiles, W), W, s->lds_bytes, stream, ka);
  });
}
