// bnn_sample_host.h -- host side shared by the three kernel families behind the Bayesian CausalBGM sampling calls (bgm_bnn_logpost /
// _mh_run / _effects / _evaluate, bnn_sample_api.hip): which family serves a session, the calls as records, and the small computations
// every family needs.  Host only: no kernel text.
//   bnf  default shapes with inference-mode normalisation, fp32 or split precision (bnf_api.hip, bnx_api.hip)
//   bns  batch statistics, LDS fragments (bnn_sample_api.hip)
//   bnw  any width (bnw_api.hip)
#pragma once
#include "bgm_host.h"

struct BnnState;
enum BnnFamily { BNF = 0, BNS = 1, BNW = 2 };
// Decided once per session from its nets and configuration alone (bnn_route).  primary: bnf iff the shapes and the normalisation pass
// bnf_build_bnn, else the second family; second: bns iff bns_plan accepts the nets, else bnw.
struct BnnRoute { bool known = false; BnnFamily primary = BNW, second = BNW; };
const BnnRoute &bnn_route(BnnState *s);
bool bnf_accepts(BnnState *s);      // bnf_api.hip: keeps the tables it built for the answer in s->bnf, for the upload at the first call
bool bns_accepts(const BnnState *s);

// the calls as the C ABI hands them over (bgm_bnn_mh_run's record is its own argument, bgm_bnn_mh_args)
struct BnnLogpostCall { const float *x, *y, *v, *z; int64_t n; int32_t block_rows, block0; uint64_t seed; uint32_t stream_id; float *out; };
struct BnnEffectsCall {
  const float *draws; int64_t n; int32_t block_rows, block0; int64_t row_base; int32_t n_keep, it0; uint64_t seed; int32_t effect, sample_y;
  const float *x_values; int32_t n_doses; double *adrf_sum; float *ite;
};
struct BnnEvalCall {
  const float *x, *y, *v; float *z; int32_t encode; int64_t n; const float *x_values; int32_t n_doses; uint64_t seed; uint32_t stream_id;
  double *sums, *dose_sums; float *ite;
};

constexpr int BNN_BNF_MAX_DOSES = 256;      // BNF_MAX_DOSES (bnf_kernels.h): the per-wave dose accumulators of bnf's effects kernel
inline int bnn_effect_doses(int effect, int n_doses) { return effect == 1 ? n_doses : effect == 2 ? 2 : 0; }
// The family of one call: the primary one, except that bnf has no evaluation and holds at most BNN_BNF_MAX_DOSES doses per call.
inline BnnFamily bnn_family_for(const BnnRoute &r, int doses) { return r.primary == BNF && doses > BNN_BNF_MAX_DOSES ? r.second : r.primary; }
inline BnnFamily bnn_family_for(BnnState *s, const BnnLogpostCall &) { return bnn_route(s).primary; }
inline BnnFamily bnn_family_for(BnnState *s, const bgm_bnn_mh_args &g) { return bnn_family_for(bnn_route(s), bnn_effect_doses(g.effect, g.n_doses)); }
inline BnnFamily bnn_family_for(BnnState *s, const BnnEffectsCall &c) { return bnn_family_for(bnn_route(s), bnn_effect_doses(c.effect, c.n_doses)); }
inline BnnFamily bnn_family_for(BnnState *s, const BnnEvalCall &) { return bnn_route(s).second; }

int bnf_logpost(bgm_handle *h, BnnState *s, const BnnLogpostCall &c, hipStream_t stream);
int bnf_mh_run(bgm_handle *h, BnnState *s, const bgm_bnn_mh_args &g, hipStream_t stream);
int bnf_effects(bgm_handle *h, BnnState *s, const BnnEffectsCall &c, hipStream_t stream);
void bnf_free(void *state);
int bnw_logpost(bgm_handle *h, BnnState *s, const BnnLogpostCall &c, hipStream_t stream);
int bnw_mh_run(bgm_handle *h, BnnState *s, const bgm_bnn_mh_args &g, hipStream_t stream);
int bnw_effects(bgm_handle *h, BnnState *s, const BnnEffectsCall &c, hipStream_t stream);
int bnw_evaluate(bgm_handle *h, BnnState *s, const BnnEvalCall &c, hipStream_t stream);
void bnw_free(void *state);

// fixed likelihood variances params['sigma_*']^2 (0: the variance heads)
struct BnnSig2 { float v, x, y; };
inline BnnSig2 bnn_sig2(const bgm_bnn_config &cfg) {
  auto sq = [](float sd) { return sd > 0.0f ? sd * sd : 0.0f; };
  return BnnSig2{sq(cfg.sigma_v), sq(cfg.sigma_x), sq(cfg.sigma_y)};
}
// rows of a call in blocks of `bs` (the batch of a network call), the first of them block `block0` of the panel
struct BnnRows { long long n, row_base; int bs, n_blocks, block0; };
inline BnnRows bnn_rows(long long n, int bs, int block0, long long row_base) { return BnnRows{n, row_base, bs, (int)((n + bs - 1) / bs), block0}; }
inline BnnRows bnn_rows(const bgm_bnn_mh_args &g) { return bnn_rows(g.n, g.block_rows, g.block0, g.row_base); }
inline BnnRows bnn_rows(const BnnEffectsCall &c) { return bnn_rows(c.n, c.block_rows, c.block0, c.row_base); }

// retained draw d = it - burn_in of a sampling call, or -1 when iteration `it` keeps none; its copy into draws_dev [n_keep][n][q]
inline int bnn_kept(const bgm_bnn_mh_args &g, int it) { return it >= g.burn_in && it - g.burn_in < g.n_keep ? it - g.burn_in : -1; }
inline bool bnn_kept_effect(const bgm_bnn_mh_args &g, int it) { return g.effect && bnn_kept(g, it) >= 0; }
inline int bnn_keep_draw(const bgm_bnn_mh_args &g, int d, int q, hipStream_t stream) {
  if (d >= 0 && g.draws_dev)
    BGM_HIP_CHECK(hipMemcpyAsync(g.draws_dev + (long long)d * g.n * q, g.state_dev, sizeof(float) * g.n * q, hipMemcpyDeviceToDevice, stream));
  return BGM_OK;
}
// Effects of retained draw d: the doses (the grid of an ADRF, the pair (1, 0) of an ITE), the first noise stream of the outcome net's
// calls (one per dose), and column d of the output [..][n_keep].
struct BnnEffectSlot { int n_doses; const float *xvals; uint32_t stream0; double *sum_out; float *ite_out; long long stride; };
inline BnnEffectSlot bnn_effect_slot(int effect, int n_doses, const float *x_values, const float *pair, double *sum, float *ite, int n_keep, int d) {
  const int nd = bnn_effect_doses(effect, n_doses);
  return BnnEffectSlot{nd, effect == 1 ? x_values : pair, 0x40000000u + (uint32_t)d * (uint32_t)nd, effect == 1 ? sum + d : nullptr,
                       effect == 2 ? ite + d : nullptr, n_keep};
}
inline BnnEffectSlot bnn_effect_slot(const bgm_bnn_mh_args &g, const float *pair, int d) { return bnn_effect_slot(g.effect, g.n_doses, g.x_values_dev, pair, g.adrf_sum_dev, g.ite_dev, g.n_keep, d); }
inline BnnEffectSlot bnn_effect_slot(const BnnEffectsCall &c, const float *pair, int d) { return bnn_effect_slot(c.effect, c.n_doses, c.x_values, pair, c.adrf_sum, c.ite, c.n_keep, d); }
// the session's (1, 0) on the device, BnnState::pair_dev (bns, bnw; bnf's tables carry their own, shared with bnf_det_api.hip): made once
int bnn_pair(BnnState *s);

// bgm_reserve for a buffer that launches in flight may still read: the stream is drained before the old allocation is freed
template <class T>
static int bnn_reserve(T *&ptr, size_t &cap, size_t count, hipStream_t stream) {
  if (count > cap) BGM_HIP_CHECK(hipStreamSynchronize(stream));
  return bgm_reserve(ptr, cap, count);
}
