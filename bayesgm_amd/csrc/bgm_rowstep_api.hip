// bgm_rowstep_api.hip -- BGM HMC with a step size per chain, adapted by that chain alone during burn-in (bgm_bgm_hmc_run_rows,
// include/bgm_hip.h): the instantiations of bgm_hmc_rows_kernel (bgm_rowstep_kernels.h) for every variant of bgm_launch.h, fp32 and
// split precision, at the wave counts of their scalar-step twins -- kept in their own translation unit.  bgm_bgm_hmc_run_rows_traj
// adds the number of leapfrog steps per chain: bgm_hmc_rows_traj_kernel for every variant, launched only when a cap, the jitter
// or the step count is asked for, so the plain per-chain step runs the kernels it ran before.  The default path
// (bgm_api.hip, bgm_bgm_hmc_run + bgm_bgm_hmc_adapt) is untouched.
// replaces: the shared step of tfp.mcmc.SimpleStepSizeAdaptation in tfp_mcmc_sampler (bgm/base.py:798-821), opt-in.
#include <string>

#include "bgm_rowstep_host.h"
#include "bgm_launch.h"
#include "gx_bgm_host.h"

// the kernel with a number of steps per chain when something of it is asked for, else the plain per-chain step, which takes ka's base
template <int KTQ, int NTX, int NH, int W, int PREC = 0, bool X4 = false>
static int bgm_hmc_rows_launch(bool want_traj, int grid, int lds, hipStream_t stream, const BgmTrajHmcKArgs &ka) {
  return want_traj ? bgm_launch(bgm_hmc_rows_traj_kernel<KTQ, NTX, NH, W, PREC, X4>, grid, W, lds, stream, ka)
                   : bgm_launch(bgm_hmc_rows_kernel<KTQ, NTX, NH, W, PREC, X4>, grid, W, lds, stream, ka);
}

// the two entries' common body; traj = nullptr: bgm_bgm_hmc_run_rows
static int bgm_hmc_rows_run(const char *fn_, bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                            float s_min, float s_max, const BgmTrajOpts *traj, void *stream_) {
  const std::string fn = std::string(fn_) + ": ";
  bool go;
  int rc = bgm_hmc_rows_check(fn, h, a, up_dev, dn_dev, n_table, s_min, s_max, traj, &go);
  if (rc || !go) return rc;
  BgmState *s = bst(h);
  if (gxb_wanted(s)) {
    bgm_set_error(fn + "the per-chain step exists for trunks [64] x 3 / [64] x 5 with z_dim <= 16; this shape runs on the "
                  "general-width engine, which has the shared step only (bgm_bgm_hmc_run)");
    return BGM_E_UNSUPPORTED;
  }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  rc = bgm_bgm_build_blob(h, stream);
  if (rc) return rc;
  // the kernels with a number of steps per chain run only when something of it is asked for
  const bool want_traj = traj && (traj->max_trajectory > 0.0f || traj->jitter != 0 || traj->n_steps != nullptr);
  BgmTrajHmcKArgs ka{};
  bgm_hmc_rows_fill(ka, s, a, up_dev, dn_dev, n_table, s_min, s_max, traj, want_traj);
  const long long tiles = (a->n + 15) / 16;
  if (s->precision != 0) {      // split precision (bgm_kernels.h, PREC 2), as bgm_bgm_hmc_run
    ka.blob = s->sx3_bias_dev; ka.m = s->sx3_meta; ka.hx3 = s->sx3_dev;
    const char *what = want_traj ? "BGM HMC with per-chain steps and trajectories (split precision)" : "BGM HMC with per-chain steps (split precision)";
    return bgm_bgm_dispatch(BgmSx3Variants{}, s->KTQ, s->NTX, s->NH, what, [&](auto v) {
      using V = decltype(v);
      constexpr int W = BGM_SX3_WAVES_DEFAULT;
      const int grid = bgm_tile_grid(h, tiles, W);
      return (s->sx3_meta.p & 3) == 0 ? bgm_hmc_rows_launch<V::KTQ, 0, V::NH, W, 2, true>(want_traj, grid, s->lds_bytes_sx3, stream, ka)
                                      : bgm_hmc_rows_launch<V::KTQ, 0, V::NH, W, 2, false>(want_traj, grid, s->lds_bytes_sx3, stream, ka);
    });
  }
  return bgm_bgm_dispatch(s, want_traj ? "BGM HMC with per-chain steps and trajectories" : "BGM HMC with per-chain steps", [&](auto v) {
    using V = decltype(v);
    constexpr int W = V::NTX == 0 ? BGM_WAVES_WIDE_HMC : BGM_WAVES;
    return bgm_hmc_rows_launch<V::KTQ, V::NTX, V::NH, W>(want_traj, bgm_tile_grid(h, tiles, W), s->lds_bytes, stream, ka);
  });
}

extern "C" int bgm_bgm_hmc_run_rows(bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                                    float s_min, float s_max, void *stream_) {
  return bgm_hmc_rows_run("bgm_bgm_hmc_run_rows", h, a, up_dev, dn_dev, n_table, s_min, s_max, nullptr, stream_);
}

extern "C" int bgm_bgm_hmc_run_rows_traj(bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                                         float s_min, float s_max, float max_trajectory, int32_t jitter, int32_t *n_steps_dev, void *stream_) {
  const BgmTrajOpts t{max_trajectory, jitter, n_steps_dev};
  return bgm_hmc_rows_run("bgm_bgm_hmc_run_rows_traj", h, a, up_dev, dn_dev, n_table, s_min, s_max, &t, stream_);
}
