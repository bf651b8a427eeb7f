// bgm_rowstep_host.h -- what the entry points of the per-chain BGM HMC kernels (bgm_rowstep_api.hip, bgm_impute_api.hip) check and fill
// alike: the argument checks of bgm_bgm_hmc_run_rows / _traj and the kernel arguments up to BgmTrajHmcKArgs.  Host only.
#pragma once
#include <cmath>
#include <string>

#include "bgm_host.h"
#include "bgm_rowstep_kernels.h"
#include "bgm_state.h"

struct BgmTrajOpts { float max_trajectory; int jitter; int *n_steps; };

// The checks every entry makes before it looks at the handle's shape; fn ends in ": ".  BGM_OK with *go = false: nothing to do.
static int bgm_hmc_rows_check(const std::string &fn, bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                              float s_min, float s_max, const BgmTrajOpts *traj, bool *go) {
  *go = false;
  if (!h || !h->bgm_state || !bst(h)->configured) { bgm_set_error(fn + "not configured"); return BGM_E_STATE; }
  if (!a) { bgm_set_error(fn + "NULL args"); return BGM_E_INVALID; }
  if ((up_dev == nullptr) != (dn_dev == nullptr)) { bgm_set_error(fn + "up_dev and dn_dev must both be given or both be NULL"); return BGM_E_INVALID; }
  if (n_table < 0) { bgm_set_error(fn + "n_table must be >= 0"); return BGM_E_INVALID; }
  if (!(s_min > 0.0f) || !(s_max >= s_min) || !std::isfinite(s_max)) { bgm_set_error(fn + "the clamp needs 0 < s_min <= s_max < inf"); return BGM_E_INVALID; }
  if (traj) {
    if (!(traj->max_trajectory >= 0.0f) || !std::isfinite(traj->max_trajectory)) { bgm_set_error(fn + "max_trajectory must be 0 (no cap) or a finite number > 0"); return BGM_E_INVALID; }
    if (traj->jitter != 0 && traj->jitter != 1) { bgm_set_error(fn + "jitter must be 0 or 1"); return BGM_E_INVALID; }
  }
  if (a->n <= 0 || a->n_iters <= 0) return BGM_OK;
  const char *null_arg = !a->x_dev ? "x_dev" : !a->state_dev ? "state_dev" : !a->logp_dev ? "logp_dev" : !a->grad_dev ? "grad_dev" : !a->step_dev ? "step_dev" : nullptr;
  if (null_arg) { bgm_set_error(fn + "NULL pointer " + null_arg); return BGM_E_INVALID; }
  if (a->n_leapfrog < 1) { bgm_set_error(fn + "n_leapfrog (num_leapfrog_steps) must be >= 1"); return BGM_E_INVALID; }
  if (a->row_base < 0 || a->row_base + a->n > 0xFFFFFFFFll) { bgm_set_error(fn + "row_base + n: row index exceeds the 32-bit RNG counter"); return BGM_E_INVALID; }
  *go = true;
  return BGM_OK;
}

// the kernel arguments of a launch on the fp32 blob; want_traj: something of the trajectory options is asked for
static void bgm_hmc_rows_fill(BgmTrajHmcKArgs &ka, const BgmState *s, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                              float s_min, float s_max, const BgmTrajOpts *traj, bool want_traj) {
  bgm_hmc_fill(ka, a);
  ka.step = nullptr;
  ka.row_step = const_cast<float *>(a->step_dev);      // (in / out here: [n] steps)
  ka.up = up_dev; ka.dn = dn_dev; ka.n_table = up_dev ? n_table : 0; ka.s_min = s_min; ka.s_max = s_max;
  ka.blob = s->blob_dev; ka.m = s->meta;
  if (want_traj) { ka.max_traj = traj->max_trajectory; ka.jitter = traj->jitter; ka.n_steps = traj->n_steps; }
}
