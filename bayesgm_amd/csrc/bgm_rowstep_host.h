// bgm_rowstep_host.h -- what the entry points of the per-chain BGM HMC kernels (bgm_rowstep_api.hip, bgm_impute_api.hip,
// bgm_impute_tails_api.hip) check and fill alike: the argument checks of bgm_bgm_hmc_run_rows / _traj and the kernel arguments up to
// BgmTrajHmcKArgs; the checks of bgm_bgm_hmc_run_rows_impute and the kernel arguments up to BgmImputeHmcKArgs.  Host only.
#pragma once
#include <cmath>
#include <string>

#include "bgm_host.h"
#include "bgm_rowstep_kernels.h"
#include "bgm_state.h"
#include "gx_bgm_host.h"

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

struct BgmImputeOpts { float *moments; float *cells; const int32_t *slot; int32_t k_slots, n_keep, add_noise; };

// The checks of bgm_bgm_hmc_run_rows_impute, in its order and with its words (fn ends in ": "): those of bgm_hmc_rows_check, then the
// entry's own arguments, then the handle's shape and precision.  BGM_OK with *go = false: nothing to do.
static int bgm_hmc_impute_check(const std::string &fn, bgm_handle *h, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                                float s_min, float s_max, const BgmTrajOpts *traj, const BgmImputeOpts &o, bool *go) {
  int rc = bgm_hmc_rows_check(fn, h, a, up_dev, dn_dev, n_table, s_min, s_max, traj, go);
  if (rc || !*go) return rc;
  *go = false;
  if (!o.moments) { bgm_set_error(fn + "NULL pointer moments_dev"); return BGM_E_INVALID; }
  if (o.cells && !o.slot) { bgm_set_error(fn + "cells_dev needs slot_dev"); return BGM_E_INVALID; }
  if (o.cells && o.k_slots < 1) { bgm_set_error(fn + "cells_dev needs k_slots >= 1"); return BGM_E_INVALID; }
  if (o.n_keep < 1) { bgm_set_error(fn + "n_keep must be >= 1"); return BGM_E_INVALID; }
  if (o.add_noise != 0 && o.add_noise != 1) { bgm_set_error(fn + "add_noise must be 0 or 1"); return BGM_E_INVALID; }
  if (a->burn_in < 0 || (long long)a->it_begin + a->n_iters > (long long)a->burn_in + o.n_keep) {
    bgm_set_error(fn + "it_begin + n_iters = " + std::to_string((long long)a->it_begin + a->n_iters) + " lies beyond burn_in + n_keep = " +
                  std::to_string((long long)a->burn_in + o.n_keep));
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
  *go = true;
  return BGM_OK;
}

static void bgm_hmc_impute_fill(BgmImputeHmcKArgs &ka, const BgmState *s, const bgm_hmc_args *a, const float *up_dev, const float *dn_dev, int32_t n_table,
                                float s_min, float s_max, const BgmTrajOpts *traj, const BgmImputeOpts &o) {
  bgm_hmc_rows_fill(ka, s, a, up_dev, dn_dev, n_table, s_min, s_max, traj, true);
  ka.moments = o.moments; ka.cells = o.cells; ka.slot = o.slot; ka.k_slots = o.k_slots; ka.n_keep = o.n_keep; ka.add_noise = o.add_noise;
}
