// bnf_api.hip -- host side of the fixed-normalisation Bayesian-network sampling path (bnf_kernels.h): shape check, fragment
// index tables, buffers, launch sequences.  Entered from bgm_bnn_logpost / bgm_bnn_mh_run / bgm_bnn_effects (bnn_sample_api.hip)
// when the session's route says so (bnn_sample_host.h): the nets have the default shapes and params['bnn_norm'] = "fixed";
// everything else keeps the batch-statistics kernels of bnn_sample_kernels.h or the any-width ones of bnw_kernels.h.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bgm_host.h"
#include "bnf_build.h"
#include "bnf_kernels.h"
#include "bnn_state.h"
#include "bnx_host.h"

static_assert(BNN_BNF_MAX_DOSES == BNF_MAX_DOSES, "the route sends calls with more doses to the second family");

namespace {

BnfNetSrc src_of(const BnnNet &b) {
  BnfNetSrc n;
  n.n_layers = b.n_layers; n.net_id = b.net_id;
  for (int l = 0; l <= b.n_layers && l < 9; ++l) n.dims[l] = b.dims[l];
  for (int l = 0; l < b.n_layers && l < 8; ++l) {
    const int cnt = b.dims[l] * b.dims[l + 1];
    n.woff[l] = b.woff[l]; n.roff[l] = b.woff[l] + cnt; n.boff[l] = b.woff[l] + 2 * cnt;
  }
  n.gamma = b.off; n.beta = b.off + b.dims[0];
  return n;
}
// false when the session is outside this path (inference-mode normalisation, default widths, q <= 31, 4 <= p <= 207)
bool bnf_build_bnn(const BnnState *s, BnfState &st, BnfTabs &tb) {
  for (int k : {BNN_G, BNN_H, BNN_F}) {
    const BnnNet &b = s->net[k];
    if (b.bn_fixed != 1 || b.heads || b.mv || b.n_layers > 8) return false;
  }
  BnfSrc S;
  S.g = src_of(s->net[BNN_G]); S.h = src_of(s->net[BNN_H]); S.f = src_of(s->net[BNN_F]);
  S.q = s->q; S.p = s->p; S.z0 = s->cfg.z_dims[0]; S.z1 = s->cfg.z_dims[1]; S.z2 = s->cfg.z_dims[2]; S.binary = s->cfg.binary_treatment;
  S.det = false;
  return bnf_build(S, st, tb);
}

// ---- kernel variants: (R row tiles per wave, WAVES per workgroup).  The shipped one is (BNF_R, BNF_W); a development build
// (-D BNF_ALL_CFGS) also carries the others for the bench shape (KS = 3) and picks by the environment variable BGM_BNF_CFG=r<R>w<W>.
#ifndef BNF_R
#define BNF_R 2
#define BNF_W 8
#endif
#ifndef BNF_ER
#define BNF_ER 2
#define BNF_EW 8
#endif
struct BnfCfg { int R, W; };
BnfCfg env_cfg(const char *name, BnfCfg d) {
#ifdef BNF_ALL_CFGS
  if (const char *e = std::getenv(name)) {
    int r = 0, w = 0;
    if (std::sscanf(e, "r%dw%d", &r, &w) == 2) d = BnfCfg{r, w};
  }
#endif
  (void)name;
  return d;
}
using MhFn = void (*)(BnfMhArgs);
using EffFn = void (*)(BnfEffArgs);
template <int KS, int MODE>
MhFn mh_fn_ks(BnfCfg &c) {
#ifdef BNF_ALL_CFGS
  if constexpr (KS == 3) {
    if (c.R == 1 && c.W == 8) return bnf_mh_kernel<KS, 1, 8, MODE>;
    if (c.R == 2 && c.W == 8) return bnf_mh_kernel<KS, 2, 8, MODE>;
    if (c.R == 2 && c.W == 4) return bnf_mh_kernel<KS, 2, 4, MODE>;
    if (c.R == 3 && c.W == 4) return bnf_mh_kernel<KS, 3, 4, MODE>;
    if (c.R == 1 && c.W == 12) return bnf_mh_kernel<KS, 1, 12, MODE>;
  }
#endif
  c = BnfCfg{BNF_R, BNF_W};
  return bnf_mh_kernel<KS, BNF_R, BNF_W, MODE>;
}
template <int KS>
EffFn eff_fn_ks(BnfCfg &c) {
#ifdef BNF_ALL_CFGS
  if constexpr (KS == 1) {
    if (c.R == 1 && c.W == 8) return bnf_effects_kernel<KS, 1, 8>;
    if (c.R == 2 && c.W == 8) return bnf_effects_kernel<KS, 2, 8>;
    if (c.R == 2 && c.W == 4) return bnf_effects_kernel<KS, 2, 4>;
    if (c.R == 4 && c.W == 4) return bnf_effects_kernel<KS, 4, 4>;
    if (c.R == 1 && c.W == 12) return bnf_effects_kernel<KS, 1, 12>;
    if (c.R == 1 && c.W == 16) return bnf_effects_kernel<KS, 1, 16>;
    if (c.R == 2 && c.W == 12) return bnf_effects_kernel<KS, 2, 12>;
  }
#endif
  c = BnfCfg{BNF_ER, BNF_EW};
  return bnf_effects_kernel<KS, BNF_ER, BNF_EW>;
}
// c: in = the requested variant, out = the one returned
template <int MODE>
MhFn mh_fn(int KS, BnfCfg &c) {
  c = env_cfg("BGM_BNF_CFG", BnfCfg{BNF_R, BNF_W});
  switch (KS) {
    case 3: return mh_fn_ks<3, MODE>(c);
    case 4: return mh_fn_ks<4, MODE>(c);
    case 5: return mh_fn_ks<5, MODE>(c);
    case 6: return mh_fn_ks<6, MODE>(c);
    default: return mh_fn_ks<8, MODE>(c);
  }
}
EffFn eff_fn(int KSF, BnfCfg &c) {
  c = env_cfg("BGM_BNF_ECFG", BnfCfg{BNF_ER, BNF_EW});
  switch (KSF) {
    case 1: return eff_fn_ks<1>(c);
    case 2: return eff_fn_ks<2>(c);
    case 3: return eff_fn_ks<3>(c);
    case 4: return eff_fn_ks<4>(c);
    default: return eff_fn_ks<8>(c);
  }
}

// BnnState::bnf.  tabs: the index tables as bnf_accepts built them, kept until the first call uploads them
struct BnfSession { BnfState *st = nullptr; BnfTabs tabs; bool uploaded = false; };

struct SgLayout { uint4 *g; uint32_t *gout; uint4 *h, *f; size_t bytes; };
SgLayout sg_layout(void *base, long long n, int states_ghf, int states_f_only) {
  SgLayout L{};
  char *p = (char *)base;
  const size_t n16 = (size_t)n * 16;
  L.g = (uint4 *)p; p += (size_t)states_ghf * BNF_NG_G * n16;
  L.gout = (uint32_t *)p; p += (size_t)states_ghf * n * BNF_GOUT * 4;
  L.h = (uint4 *)p; p += (size_t)states_ghf * BNF_NG_H * n16;
  L.f = (uint4 *)p; p += (size_t)std::max(states_ghf, states_f_only) * BNF_NG_H * n16;
  L.bytes = (size_t)(p - (char *)base);
  return L;
}

// One call on this family: the session's tables, the call's rows and noise key, the sign groups of its states.  rib0: the position of
// the first row inside its block (a rank's share of ONE block, bgm_bnn_mh_args::block_row0; 0 for calls that start a block)
struct BnfRun { BnfState *st; BnnRows r; long long rib0; uint64_t seed; bool x3; int grid; SgLayout L; };

// tables on the device, blobs current for the session's parameters and precision
int bnf_begin(bgm_handle *h, BnnState *s, const BnnRows &r, uint64_t seed, hipStream_t stream, BnfRun &run) {
  BnfSession *b = static_cast<BnfSession *>(s->bnf);
  BnfState *st = b->st;
  if (!b->uploaded) {
    if (!bnf_upload(st, b->tabs)) {      // nothing half-made stays behind: the next call decides and builds again
      bnf_free(b); s->bnf = nullptr; s->route = BnnRoute{};
      bgm_set_error("bnf: device allocation failed"); return BGM_E_HIP;
    }
    b->tabs = BnfTabs{}; b->uploaded = true;
  }
  if (!s->bnf_valid) {
    int rc = bnf_pack(st, s->theta_dev, stream);
    if (rc) return rc;
    s->bnf_valid = true;
  }
  run = BnfRun{st, r, 0, seed, s->precision == 2, std::max(8, (h->n_cus / 8) * 8), SgLayout{}};
  return run.x3 ? bnx_prepare(st, stream) : BGM_OK;      // split precision: the blobs in the fragment encoding of bnx_kernels.h
}

// Perturbation sets (dw_floats, cleared: their padding positions must be zero and the noise kernel writes real elements only; the set
// boundaries move with (n_blocks, n_doses), so the used part is cleared at every call -- tens of MB, once per call) and sign groups
int bnf_buffers(BnfRun &run, size_t dw_floats, int states_ghf, int states_f_only, hipStream_t stream) {
  BnfState *st = run.st;
  int rc = bnn_reserve(st->dw_dev, st->dw_cap, dw_floats, stream);
  if (rc) return rc;
  if (dw_floats) BGM_HIP_CHECK(hipMemsetAsync(st->dw_dev, 0, sizeof(float) * dw_floats, stream));
  char *sg = static_cast<char *>(st->sg_dev);
  rc = bnn_reserve(sg, st->sg_cap, sg_layout(nullptr, run.r.n, states_ghf, states_f_only).bytes, stream);
  st->sg_dev = sg;
  run.L = sg_layout(sg, run.r.n, states_ghf, states_f_only);
  return rc;
}

// effects = true: sets of the outcome net in the effects layout
void launch_noise(const BnfRun &run, bool effects, float *dw, int n_states, uint32_t stream0, hipStream_t stream) {
  const BnfState *st = run.st;
  BnfNoiseArgs na{};
  const int n_lay = effects ? 4 : 14;
  for (int i = 0; i < n_lay; ++i) na.lay[i] = effects ? st->lay_e[i] : st->lay[i];
  na.n_lay = n_lay; na.n_calls = effects ? st->n_calls_e : st->n_calls; na.npos = effects ? st->npos_e_dev : st->npos_dev;
  na.sf = effects ? st->esf_dev : st->sf_dev; na.dw = dw; na.set_floats = effects ? (long long)st->P.e_frags * 256 : st->P.set_floats;
  na.n_states = n_states; na.k0 = (uint32_t)run.seed; na.k1 = (uint32_t)(run.seed >> 32); na.stream0 = stream0; na.block0 = run.r.block0;
  if (run.x3) bnx_launch_noise(na, effects ? st->posx_e_dev : st->posx_dev, run.r.n_blocks * n_states, stream);
  else hipLaunchKernelGGL(bnf_noise_kernel, dim3((na.n_calls + 1023) / 1024, run.r.n_blocks * n_states), dim3(256), 0, stream, na);
}

void launch_signs(const BnfRun &run, int n_states, int nets, uint32_t stream0, unsigned *queue, hipStream_t stream) {
  const SgLayout &L = run.L;
  BnfSignArgs sa{};
  sa.rib0 = run.rib0;
  sa.g = L.g; sa.gout = L.gout; sa.h = L.h; sa.f = L.f; sa.n = run.r.n; sa.bs = run.r.bs; sa.block0 = run.r.block0; sa.n_states = n_states; sa.nets = nets;
  sa.k0 = (uint32_t)run.seed; sa.k1 = (uint32_t)(run.seed >> 32); sa.stream0 = stream0; sa.queue = queue;
  hipLaunchKernelGGL(bnf_signs_kernel, dim3((unsigned)((run.r.n + 255) / 256), n_states), dim3(256), 0, stream, sa);
}

// workgroups hold c.R row tiles of 16 per wave: the items of a block
int groups_per_block(int bs, const BnfCfg &c) { return ((bs + 15) / 16 + c.R - 1) / c.R; }

// the fields a call fixes of its log-posterior / MH launches
BnfMhArgs mh_args(const BnfRun &run, const BnnState *s, const BnfCfg &c) {
  const BnfState *st = run.st;
  BnfMhArgs a{};
  a.pl = st->P; a.blob = run.x3 ? st->blobx_dev : st->blob_dev; a.dw = st->dw_dev;
  const BnnSig2 sig2 = bnn_sig2(s->cfg);
  a.sig2_v = sig2.v; a.sig2_x = sig2.x; a.sig2_y = sig2.y;
  a.sg.g = run.L.g; a.sg.gout = run.L.gout; a.sg.h = run.L.h; a.sg.f = run.L.f;
  a.n = run.r.n; a.row_base = run.r.row_base; a.bs = run.r.bs; a.n_blocks = run.r.n_blocks; a.block0 = run.r.block0;
  a.groups_per_block = groups_per_block(run.r.bs, c); a.n_items = run.r.n_blocks * a.groups_per_block;
  a.k0 = (uint32_t)run.seed; a.k1 = (uint32_t)(run.seed >> 32); a.queue = st->queue_dev;
  return a;
}

// the effects launches of one call: everything but the draw
struct BnfEffects { BnfEffArgs ea; EffFn fn; int W; };
int effects_begin(const BnfRun &run, const BnnState *s, float *dw, int sample_y, BnfEffects &e) {
  const BnfState *st = run.st;
  BnfCfg c;
  e.fn = run.x3 ? bnx_eff_fn(st->KSFc, &c.R, &c.W) : eff_fn(st->KSFc, c);
  e.W = c.W;
  BnfEffArgs &ea = e.ea;
  ea = BnfEffArgs{};
  ea.pl = st->P; ea.eblob = run.x3 ? st->eblobx_dev : st->eblob_dev; ea.dw = dw; ea.sgf = run.L.f; ea.n = run.r.n; ea.row_base = run.r.row_base;
  ea.sig2_y = bnn_sig2(s->cfg).y;
  ea.bs = run.r.bs; ea.n_blocks = run.r.n_blocks; ea.block0 = run.r.block0;
  ea.groups_per_block = groups_per_block(run.r.bs, c); ea.n_items = run.r.n_blocks * ea.groups_per_block;
  ea.k0 = (uint32_t)run.seed; ea.k1 = (uint32_t)(run.seed >> 32); ea.sample_y = sample_y; ea.queue = st->queue_dev + 8;
  return bgm_set_lds(e.fn, st->lds_eff);
}
// effects of ONE draw (state z) -> adrf column / ite column of the slot
void effects_of(const BnfRun &run, BnfEffects &e, const BnnEffectSlot &sl, const float *z, uint32_t it_noise, hipStream_t stream) {
  launch_noise(run, true, const_cast<float *>(e.ea.dw), sl.n_doses, sl.stream0, stream);
  launch_signs(run, sl.n_doses, 4, sl.stream0, run.st->queue_dev + 8, stream);
  BnfEffArgs &ea = e.ea;
  ea.z = z; ea.n_doses = sl.n_doses; ea.xvals = sl.xvals; ea.it_noise = it_noise;
  ea.sum_out = sl.sum_out; ea.sum_stride = sl.stride; ea.ite_out = sl.ite_out; ea.ite_stride = sl.stride;
  hipLaunchKernelGGL(e.fn, dim3(run.grid), dim3(64 * e.W), run.st->lds_eff, stream, ea);
}

}  // namespace

void bnf_free(void *state) { if (BnfSession *b = static_cast<BnfSession *>(state)) { bnf_release(b->st); delete b; } }

bool bnf_accepts(BnnState *s) {
  BnfSession *b = new BnfSession();
  b->st = new BnfState();
  if (!bnf_build_bnn(s, *b->st, b->tabs)) { bnf_free(b); return false; }
  s->bnf = b; s->bnf_valid = false;
  return true;
}

extern "C" int bgm_bnn_set_precision(bgm_handle *h, int32_t mode) {
  if (!h || !h->bnn_state) { bgm_set_error("bgm_bnn_set_precision: no Bayesian-network session (bgm_bnn_begin)"); return BGM_E_STATE; }
  if (mode != 0 && mode != 2) {
    bgm_set_error("bgm_bnn_set_precision: mode must be 0 (fp32) or 2 (f16x3); the Bayesian sampling kernels have no bf16 form");
    return mode == 1 ? BGM_E_UNSUPPORTED : BGM_E_INVALID;
  }
  BnnState *s = static_cast<BnnState *>(h->bnn_state);
  if (mode == 2 && bnn_route(s).primary != BNF) {      // the split-precision kernels exist for the sessions bnf_kernels.h serves: say so now, not at the first sampling call
    bgm_set_error("bgm_bnn_set_precision: split precision exists on the default-shape sampling kernels with inference-mode input normalisation "
                  "(bnn_norm='fixed', g_units [64]x5, f_units / h_units [64,32,8], sum(z_dims) <= 31, v_dim <= 207)");
    return BGM_E_UNSUPPORTED;
  }
  s->precision = mode;
  return BGM_OK;
}

int bnf_logpost(bgm_handle *h, BnnState *s, const BnnLogpostCall &c, hipStream_t stream) {
  BnfRun run;
  int rc = bnf_begin(h, s, bnn_rows(c.n, c.block_rows, c.block0, 0), c.seed, stream, run);
  if (rc) return rc;
  BnfState *st = run.st;
  BnfCfg cfg;
  MhFn fn = run.x3 ? bnx_mh_fn(st->KSc, 0, &cfg.R, &cfg.W) : mh_fn<0>(st->KSc, cfg);
  rc = bnf_buffers(run, (size_t)run.r.n_blocks * st->P.set_floats, 1, 0, stream);
  if (rc) return rc;
  launch_noise(run, false, st->dw_dev, 1, c.stream_id, stream);
  launch_signs(run, 1, 7, c.stream_id, st->queue_dev, stream);
  BnfMhArgs a = mh_args(run, s, cfg);
  a.x = c.x; a.y = c.y; a.v = c.v; a.z = const_cast<float *>(c.z); a.n_states = 1; a.mode = 0; a.out = c.out;
  if (s->bp_on) {      // conditional prior: one noisy call of the prior net for this evaluation (bprior_api.hip)
    if ((rc = bprior_rows(h, s, c.n, c.block_rows, c.block0, c.seed, c.stream_id, 1, stream))) return rc;
    a.prior = s->bp_rows; a.prior_stride = 0;
  }
  rc = bgm_set_lds(fn, st->lds_mh);
  if (rc) return rc;
  hipLaunchKernelGGL(fn, dim3(run.grid), dim3(64 * cfg.W), st->lds_mh, stream, a);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

int bnf_mh_run(bgm_handle *h, BnnState *s, const bgm_bnn_mh_args &g, hipStream_t stream) {
  // A rank's share of ONE block (row_base inside the block block0): the Flipout sign words of the samplers and of the prior net are keyed
  // by (block, position in the block), so the position of the first row travels with the call -- results do not depend on how the block's
  // rows are split over ranks.
  const long long rib0 = g.block_row0, n = g.n;
  const int bs = g.block_rows, q = s->q, n_doses = bnn_effect_doses(g.effect, g.n_doses);
  if (rib0 < 0 || rib0 >= bs || (rib0 > 0 && rib0 + n > bs)) { bgm_set_error("bgm_bnn_mh_run: block_row0 must lie inside the block, and a call that starts inside a block must end inside it"); return BGM_E_INVALID; }
  BnfRun run;
  int rc = bnf_begin(h, s, bnn_rows(g), g.seed, stream, run);
  if (rc) return rc;
  run.rib0 = rib0;
  BnfState *st = run.st;
  const BnfPlan &P = st->P;
  const int n_blocks = run.r.n_blocks;
  BnfCfg c;
  // split precision: a three-launch iteration (proposal / both evaluations as (item, state) units / accept step)
  const bool x3 = run.x3;
  MhFn fn = x3 ? bnx_mh_fn(st->KSc, 1, &c.R, &c.W) : mh_fn<1>(st->KSc, c);
  const size_t dw_mh = (size_t)n_blocks * 2 * P.set_floats, dw_eff = (size_t)n_blocks * n_doses * P.e_frags * 256;
  rc = bnf_buffers(run, dw_mh + dw_eff, 2, n_doses, stream);
  if (rc) return rc;
  BnfMhArgs a = mh_args(run, s, c);
  a.x = g.x_dev; a.y = g.y_dev; a.v = g.v_dev; a.z = g.state_dev; a.n_states = 2;
  a.mode = 1; a.q_sd = g.q_sd; a.q_sd_blocks = g.q_sd_blocks_dev; a.acc_count = g.acc_count_dev;
  rc = bgm_set_lds(fn, st->lds_mh);
  if (rc) return rc;
  BnfEffects eff;
  if (g.effect && (rc = effects_begin(run, s, st->dw_dev + dw_mh, g.sample_y, eff))) return rc;
#ifdef BNF_PROF
  static unsigned long long *prof_dev = nullptr;
  if (!prof_dev) hipMalloc((void **)&prof_dev, 256);
  hipMemsetAsync(prof_dev, 0, 256, stream);
  a.prof = prof_dev;
#endif
  if (x3) {      // proposals [n x q] | the two log posteriors [2][n] of the three-launch iteration
    rc = bnn_reserve(st->mh_dev, st->mh_cap, (size_t)n * (q + 2), stream);
    if (rc) return rc;
    a.zprop = st->mh_dev; a.out = st->mh_dev + (size_t)n * q; a.mode = 3;
  }
  for (int i = 0; i < g.n_iters; ++i) {
    const int it = g.it_begin + i;
    launch_noise(run, false, st->dw_dev, 2, 2u * (uint32_t)it, stream);
    launch_signs(run, 2, 7, 2u * (uint32_t)it, st->queue_dev, stream);
    a.it = it; a.init = (i == 0 && g.init) ? 1 : 0;
    if (s->bp_on) {    // conditional prior: the two evaluations' own calls of the prior net (streams 2 it, 2 it + 1)
      if ((rc = bprior_rows(h, s, n, bs, g.block0, g.seed, 2u * (uint32_t)it, 2, stream, rib0))) return rc;
      a.prior = s->bp_rows; a.prior_stride = n * (long long)(q + 2);
    }
    a.acc_blocks = g.acc_blocks_dev ? g.acc_blocks_dev + (long long)i * n_blocks : nullptr;
    if (x3) {      // proposal, both evaluations as independent (item, state) units, accept step (bnx_kernels.h)
      BnxMhStep ms{};
      ms.z = g.state_dev; ms.zprop = st->mh_dev; ms.lp = a.out; ms.n = n; ms.row_base = g.row_base; ms.q = q; ms.bs = bs; ms.it = it; ms.init = a.init;
      ms.q_sd = g.q_sd; ms.q_sd_blocks = g.q_sd_blocks_dev; ms.k0 = a.k0; ms.k1 = a.k1; ms.acc_count = g.acc_count_dev; ms.acc_blocks = a.acc_blocks;
      bnx_launch_propose(ms, stream);
      hipLaunchKernelGGL(fn, dim3(run.grid), dim3(64 * c.W), st->lds_mh, stream, a);
      bnx_launch_accept(ms, stream);
    } else {
      hipLaunchKernelGGL(fn, dim3(run.grid), dim3(64 * c.W), st->lds_mh, stream, a);
    }
    const int d = bnn_kept(g, it);
    if ((rc = bnn_keep_draw(g, d, q, stream))) return rc;
    if (d >= 0 && g.effect) effects_of(run, eff, bnn_effect_slot(g, st->pair_dev, d), g.state_dev, (uint32_t)it, stream);
  }
#ifdef BNF_PROF
  {
    unsigned long long hp[32];
    hipStreamSynchronize(stream);
    hipMemcpy(hp, prof_dev, sizeof(hp), hipMemcpyDeviceToHost);
    const double d = (double)run.grid * std::max(1, g.n_iters);
    fprintf(stderr, "[BNF_PROF] cycles per workgroup-launch (wave 0, R=%d W=%d): prologue %.0f g-first %.0f g-hidden %.0f g-last %.0f h %.0f f %.0f rest %.0f\n",
            c.R, c.W, hp[0] / d, hp[1] / d, hp[2] / d, hp[3] / d, hp[4] / d, hp[5] / d, hp[6] / d);
    fprintf(stderr, "[BNF_PROF] extra stamp 7 (split precision: hidden-layer epilogues; 2 = their matrix products): %.0f\n", hp[28] / d);
    const double dw = d * c.W;
    fprintf(stderr, "[BNF_PROF] wave busy cycles per launch: mean %.0f, max (over all launches) %llu; by wave index:", hp[7] / dw, hp[8]);
    for (int w = 0; w < c.W; ++w) fprintf(stderr, " %.0f", hp[9 + w] / d);
    fprintf(stderr, "\n");
  }
#endif
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

int bnf_effects(bgm_handle *h, BnnState *s, const BnnEffectsCall &c, hipStream_t stream) {
  BnfRun run;
  int rc = bnf_begin(h, s, bnn_rows(c), c.seed, stream, run);
  if (rc) return rc;
  BnfState *st = run.st;
  const int nd = bnn_effect_doses(c.effect, c.n_doses);
  rc = bnf_buffers(run, (size_t)run.r.n_blocks * nd * st->P.e_frags * 256, 0, nd, stream);
  if (rc) return rc;
  BnfEffects eff;
  if ((rc = effects_begin(run, s, st->dw_dev, c.sample_y, eff))) return rc;
  for (int d = 0; d < c.n_keep; ++d)
    effects_of(run, eff, bnn_effect_slot(c, st->pair_dev, d), c.draws + (long long)d * c.n * s->q, (uint32_t)(c.it0 + d), stream);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
