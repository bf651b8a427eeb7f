// bgm_rowstep_api.hip -- BGM HMC with a step size per chain, adapted by that chain alone during burn-in (bgm_bgm_hmc_run_rows,
// include/bgm_hip.h): the instantiations of bgm_hmc_rows_kernel (bgm_rowstep_kernels.h) for every variant of bgm_launch.h, fp32 and
// split precision, at the wave counts of their scalar-step twins -- kept in their own translation unit.  The default path
// (bgm_api.hip, bgm_bgm_hmc_run + bgm_bgm_hmc_adapt) is untouched.
// replaces: the shared step of tfp.mcmc.SimpleStepSizeAdaptation in tfp_mcmc_sampler (bgm/base.py:798-821), opt-in.
#include <cmath>
#include <string>

#include "bgm_host.h"
#include "bgm_rowstep_kernels.h"
#include "bgm_launch.h"
#include "gx_bgm_host.h"

extern "C" int bgm_bgm_hmc_run_rows(bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                                    float s_min, float s_max, void *stream_) {
  if (!h || !h->bgm_state || !bst(h)->configured) { bgm_set_error("bgm_bgm_hmc_run_rows: not configured"); return BGM_E_STATE; }
  if (!a) { bgm_set_error("bgm_bgm_hmc_run_rows: NULL args"); return BGM_E_INVALID; }
  if ((up_dev == nullptr) != (dn_dev == nullptr)) { bgm_set_error("bgm_bgm_hmc_run_rows: up_dev and dn_dev must both be given or both be NULL"); return BGM_E_INVALID; }
  if (n_table < 0) { bgm_set_error("bgm_bgm_hmc_run_rows: n_table must be >= 0"); return BGM_E_INVALID; }
  if (!(s_min > 0.0f) || !(s_max >= s_min) || !std::isfinite(s_max)) { bgm_set_error("bgm_bgm_hmc_run_rows: the clamp needs 0 < s_min <= s_max < inf"); return BGM_E_INVALID; }
  if (a->n <= 0 || a->n_iters <= 0) return BGM_OK;
  const char *null_arg = !a->x_dev ? "x_dev" : !a->state_dev ? "state_dev" : !a->logp_dev ? "logp_dev" : !a->grad_dev ? "grad_dev" : !a->step_dev ? "step_dev" : nullptr;
  if (null_arg) { bgm_set_error(std::string("bgm_bgm_hmc_run_rows: NULL pointer ") + null_arg); return BGM_E_INVALID; }
  if (a->n_leapfrog < 1) { bgm_set_error("bgm_bgm_hmc_run_rows: n_leapfrog (num_leapfrog_steps) must be >= 1"); return BGM_E_INVALID; }
  if (a->row_base < 0 || a->row_base + a->n > 0xFFFFFFFFll) { bgm_set_error("bgm_bgm_hmc_run_rows: row_base + n: row index exceeds the 32-bit RNG counter"); return BGM_E_INVALID; }
  BgmState *s = bst(h);
  if (gxb_wanted(s)) {
    bgm_set_error("bgm_bgm_hmc_run_rows: the per-chain step exists for trunks [64] x 3 / [64] x 5 with z_dim <= 16; this shape runs on the "
                  "general-width engine, which has the shared step only (bgm_bgm_hmc_run)");
    return BGM_E_UNSUPPORTED;
  }
  hipStream_t stream = (hipStream_t)stream_;
  BGM_HIP_CHECK(hipSetDevice(h->device));
  int rc = bgm_bgm_build_blob(h, stream);
  if (rc) return rc;
  BgmRowHmcKArgs ka{};
  bgm_hmc_fill(ka, a);
  ka.step = nullptr;
  ka.row_step = const_cast<float *>(a->step_dev);      // (in / out here: [n] steps)
  ka.up = up_dev; ka.dn = dn_dev; ka.n_table = up_dev ? n_table : 0; ka.s_min = s_min; ka.s_max = s_max;
  ka.blob = s->blob_dev; ka.m = s->meta;
  const long long tiles = (a->n + 15) / 16;
  if (s->precision != 0) {      // split precision (bgm_kernels.h, PREC 2), as bgm_bgm_hmc_run
    ka.blob = s->sx3_bias_dev; ka.m = s->sx3_meta; ka.hx3 = s->sx3_dev;
    return bgm_bgm_dispatch(BgmSx3Variants{}, s->KTQ, s->NTX, s->NH, "BGM HMC with per-chain steps (split precision)", [&](auto v) {
      using V = decltype(v);
      constexpr int W = BGM_SX3_WAVES_DEFAULT;
      return bgm_launch((s->sx3_meta.p & 3) == 0 ? bgm_hmc_rows_kernel<V::KTQ, 0, V::NH, W, 2, true> : bgm_hmc_rows_kernel<V::KTQ, 0, V::NH, W, 2, false>,
                        bgm_tile_grid(h, tiles, W), W, s->lds_bytes_sx3, stream, ka);
    });
  }
  return bgm_bgm_dispatch(s, "BGM HMC with per-chain steps", [&](auto v) {
    using V = decltype(v);
    constexpr int W = V::NTX == 0 ? BGM_WAVES_WIDE_HMC : BGM_WAVES;
    return bgm_launch(bgm_hmc_rows_kernel<V::KTQ, V::NTX, V::NH, W>, bgm_tile_grid(h, tiles, W), W, s->lds_bytes, stream, ka);
  });
}
