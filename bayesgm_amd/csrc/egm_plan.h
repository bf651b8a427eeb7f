// egm_plan.h -- host-side decisions of the EGM warm start (egm_api.hip, bnn_egm_api.hip) and of every path that runs the row-tile chains
// (fit_api.hip, bnn_api.hip) as plain functions of plain values: the chain shape rule and its net predicates, the working set of the
// workgroup discriminator kernel, the development switches and which kernel a session's two steps run.  No HIP and no kernel here, in
// the manner of fit_launch.h: the LDS sizes of the chain kernels come in as numbers (ech_disc_lds_floats / ecg_lds_floats /
// ecb_lds_floats stay with their kernels), and a route is mapped to kernel pointers where a unit instantiates them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

constexpr int EGM_LDS_LIMIT = 160 * 1024;      // bytes of LDS one workgroup may ask for
constexpr int chain_tiles(int n) { return (n + 15) / 16; }

// ---- the row-tile chains' shape rule.  t0: latent input tiles (q <= 16 t0); ntl_need: 16-wide tiles of g's output p + 1; ntl: the
// compiled extent that serves it -- 13 and 7 exactly, anything else (and every two-latent-tile model) the 13-tile kernels with masked
// columns; pad: those masked kernels, compiled for two row tiles (B = 32) only
struct ChainExtent { int t0, ntl_need, ntl; bool pad; };
constexpr ChainExtent chain_extent(int q, int p) {
  const int ntl_need = (p + 16) / 16, t0 = q <= 16 ? 1 : 2;
  const int ntl = ((ntl_need == 13 || ntl_need == 7) && t0 == 1) ? ntl_need : 13;
  return {t0, ntl_need, ntl, ntl != ntl_need || t0 == 2};
}
// the extent exists at B rows: at most 13 tiles, and a masked extent wants two row tiles
constexpr bool chain_extent_ok(const ChainExtent &x, int B) { return x.ntl_need <= 13 && (x.ntl == x.ntl_need || B == 32); }

// ---- the net predicates that go with it, on a net's dims[0..n_layers] (input, hidden..., output)
struct NetDims { const int *dims; int n_layers; };
// every hidden layer 64 wide
constexpr bool chain_hidden64(NetDims n) {
  for (int l = 1; l < n.n_layers; ++l) if (n.dims[l] != 64) return false;
  return true;
}
// g or e: at least min_layers layers, 64-wide hidden layers, and the given input / output widths (< 0: not looked at)
constexpr bool chain_trunk_ok(NetDims n, int min_layers, int in, int out) {
  return n.n_layers >= min_layers && (in < 0 || n.dims[0] == in) && (out < 0 || n.dims[n.n_layers] == out) && chain_hidden64(n);
}
// f or h: 64-32-(1..16) with at most 16 inputs; the output width in [out_lo, out_hi] (the fit wants the mean / variance pair == 2, the warm
// start takes 1..16)
constexpr bool chain_head_ok(NetDims n, int out_lo, int out_hi) {
  return n.n_layers == 4 && n.dims[0] <= 16 && n.dims[1] == 64 && n.dims[2] == 32 && n.dims[3] >= 1 && n.dims[3] <= 16 && n.dims[4] >= out_lo &&
         n.dims[4] <= out_hi;
}
// the discriminator (dims: q, d1, d2, d3, 1) of the register-chained steps: fixed normalisation, 4 / 2 / 1 tiles of hidden units, one or
// two 16-row tiles, one latent input tile or two (two: B = 32 only, the fourth pass's stash in global scratch)
constexpr bool chain_disc_ok(bool fixed_norm, int n_hidden, const int *d, int B) {
  return fixed_norm && n_hidden == 3 && d[0] <= 32 && (d[0] <= 16 || B == 32) && chain_tiles(d[1]) == 4 && chain_tiles(d[2]) == 2 && d[3] >= 1 &&
         d[3] <= 16 && (B == 16 || B == 32);
}
// the Bayesian nets (bnn_kernels.h BnnNet) as the predicates see them
struct BnnNetDims { NetDims n; int bn_fixed, heads, mv; };
constexpr bool bnn_chain_plain(const BnnNetDims &m) { return m.bn_fixed == 1 && !m.heads && !m.mv; }
// shapes the Bayesian row-tile chains are compiled for (need_e: the encoder takes part, the EGM generator step)
constexpr bool bnn_chain_shapes_ok(const BnnNetDims &g, const BnnNetDims &e, const BnnNetDims &f, const BnnNetDims &h, int q, int p, bool need_e) {
  return q <= 32 && chain_extent(q, p).ntl_need <= 13 && bnn_chain_plain(g) && bnn_chain_plain(f) && bnn_chain_plain(h) && chain_trunk_ok(g.n, 3, q, p + 1) &&
         (!need_e || (bnn_chain_plain(e) && chain_trunk_ok(e.n, 3, p, q))) && chain_head_ok(f.n, 1, 16) && chain_head_ok(h.n, 1, 16);
}

// ---- working set of the workgroup discriminator kernel (egm_disc_step_kernel, bnn_egm_disc_step_kernel): cache A | max(cache B + da + du,
// gradient-penalty scratch), in LDS behind the 64 reduction words while it fits.  dz: q, d1..dL (the scalar output is not part of it)
struct EgmArena { size_t cache, floats; int dmax; bool in_lds; int lds_bytes; };
constexpr EgmArena egm_arena(int B, int n_hidden, const int *dz) {
  int dmax = 0, dsum = 0, dall = 0;
  for (int l = 0; l <= n_hidden; ++l) { dmax = std::max(dmax, dz[l]); dall += dz[l]; }
  for (int l = 1; l <= n_hidden; ++l) dsum += dz[l];
  const size_t cache = ((size_t)(2 * B + 1) * dsum + B + 3) / 4 * 4;
  const size_t gp = ((size_t)B * dall + (size_t)(5 * B + 1) * dsum + 3) / 4 * 4 + 3 * (size_t)B * dmax;
  const size_t arena = cache + std::max(cache + 2 * (size_t)B * dmax, gp);
  const bool in_lds = (64 + arena) * sizeof(float) <= (size_t)EGM_LDS_LIMIT;
  return {cache, arena, dmax, in_lds, (int)((64 + (in_lds ? arena : 0)) * sizeof(float))};
}

// ---- development switches of the warm start: read when a session begins and kept in it, so that a process may begin sessions under
// different settings (tests/test_gpu_egm_edges.py) and no step call reads the environment
struct EgmSwitches {
  bool no_chain;          // BGM_EGM_NO_CHAIN: the discriminator step on the workgroup kernel
  bool no_chain_gen;      // BGM_EGM_NO_CHAIN_GEN: the generator step on the workgroup kernel
  bool no_chain_bnn;      // BGM_EGM_NO_CHAIN_BNN: the Bayesian discriminator chain with the general Flipout encoder
};
static inline EgmSwitches egm_switches_now() {
  return {std::getenv("BGM_EGM_NO_CHAIN") != nullptr, std::getenv("BGM_EGM_NO_CHAIN_GEN") != nullptr, std::getenv("BGM_EGM_NO_CHAIN_BNN") != nullptr};
}
// BGM_BNN_STEP_ONE_LAUNCH (a Bayesian general-width step inside its one workgroup, no noise / gradient / Adam launches around it): once
// per process
static inline bool bnn_step_one_launch() {
  static const bool on = std::getenv("BGM_BNN_STEP_ONE_LAUNCH") != nullptr;
  return on;
}

// ---- the deterministic session (egm_api.hip).  The routes under the names of tests/_egm_edges_ref.py, in the order egm_api.hip
// instantiates their kernels
enum class EgmDiscRoute { CHAIN_T2, CHAIN_32_K13, CHAIN_32_K7, CHAIN_32_STREAM, CHAIN_16, LDS, GLOBAL };
enum class EgmGenRoute { CHAIN_T2, CHAIN_PAD, CHAIN_32_N13, CHAIN_32_N7, CHAIN_16_N13, CHAIN_16_N7, STEP };
constexpr const char *EGM_DISC_ROUTE_NAMES[] = {"chain-t2", "chain-32-k13", "chain-32-k7", "chain-32-stream", "chain-16", "lds", "global"};
constexpr const char *EGM_GEN_ROUTE_NAMES[] = {"chain-t2", "chain-pad", "chain-32-n13", "chain-32-n7", "chain-16-n13", "chain-16-n7", "step"};
//   chain-t2         two latent tiles (q 17..32), B = 32        chain-t2       two latent tiles, masked 13-tile output of g
//   chain-32-k13     B = 32, (p + 15) / 16 == 13                chain-pad      B = 32, p + 1 narrower than a compiled extent: 13 tiles, masked
//   chain-32-k7      B = 32, (p + 15) / 16 == 7                 chain-32-n13   B = 32, (p + 16) / 16 == 13
//   chain-32-stream  B = 32, any other p                        chain-32-n7    B = 32, (p + 16) / 16 == 7
//   chain-16         B = 16                                     chain-16-n13   B = 16, 13 tiles
//   lds              workgroup kernel, arena in LDS             chain-16-n7    B = 16, 7 tiles
//   global           workgroup kernel, arena in the workspace   step           workgroup kernel
struct EgmShape { int q, p, B; bool fixed_norm; int dz_hidden; const int *dz; NetDims g, e, f, h; };
// chain_disc_lds / chain_gen_lds: bytes of LDS of the chain kernel chosen, 0 when the step runs the workgroup kernel
struct EgmPlan { EgmDiscRoute disc; EgmGenRoute gen; ChainExtent ext; EgmArena arena; int chain_disc_lds, chain_gen_lds; };
// chain_disc_bytes / chain_gen_bytes: what the chain kernels of this (B, t0) need, from the kernel headers
constexpr EgmPlan egm_plan(const EgmShape &s, const EgmSwitches &sw, size_t chain_disc_bytes, size_t chain_gen_bytes) {
  const ChainExtent x = chain_extent(s.q, s.p);
  const EgmArena arena = egm_arena(s.B, s.dz_hidden, s.dz);
  const bool dchain = chain_disc_ok(s.fixed_norm, s.dz_hidden, s.dz, s.B) && s.q <= 32 && chain_trunk_ok(s.e, 2, -1, s.q) && !sw.no_chain &&
                      chain_disc_bytes <= (size_t)EGM_LDS_LIMIT;
  // the generator chain: behind a chained discriminator only, g with 64-wide hidden layers and a compiled output extent, the heads
  const bool gchain = dchain && chain_extent_ok(x, s.B) && chain_trunk_ok(s.g, 2, s.q, -1) && chain_head_ok(s.f, 1, 16) && chain_head_ok(s.h, 1, 16) &&
                      !sw.no_chain_gen;
  const int kt0 = chain_tiles(s.p);      // compiled first-layer extents of e: p in (192, 208] and (96, 112]; any other p streams
  const EgmDiscRoute disc = !dchain ? (arena.in_lds ? EgmDiscRoute::LDS : EgmDiscRoute::GLOBAL)
                            : x.t0 == 2 ? EgmDiscRoute::CHAIN_T2
                            : s.B == 16 ? EgmDiscRoute::CHAIN_16
                            : kt0 == 13 ? EgmDiscRoute::CHAIN_32_K13 : kt0 == 7 ? EgmDiscRoute::CHAIN_32_K7 : EgmDiscRoute::CHAIN_32_STREAM;
  const EgmGenRoute gen = !gchain ? EgmGenRoute::STEP
                          : x.t0 == 2 ? EgmGenRoute::CHAIN_T2
                          : x.pad ? EgmGenRoute::CHAIN_PAD
                          : s.B == 32 ? (x.ntl == 13 ? EgmGenRoute::CHAIN_32_N13 : EgmGenRoute::CHAIN_32_N7)
                                      : (x.ntl == 13 ? EgmGenRoute::CHAIN_16_N13 : EgmGenRoute::CHAIN_16_N7);
  return {disc, gen, x, arena, dchain ? (int)chain_disc_bytes : 0, gchain ? (int)chain_gen_bytes : 0};
}

// ---- the Bayesian session (bnn_egm_api.hip), from the same predicates.  Discriminator step: the register-chained discriminator with the
// Flipout encoder as a 13- or 7-tile chain (E13: masked for a narrower p) or in its general form (E0), by rows and latent tiles, else the
// workgroup kernel (WG); in the order bnn_egm_api.hip instantiates the kernels.  The encoder call's noise: drawn by
// bnn_egm_disc_noise_kernel in front of an encoder chain; E0 and WG draw it over the chip in a launch of their own (`wide`), or inside
// the one workgroup under BGM_BNN_STEP_ONE_LAUNCH.  Generator step: the four chain launchers (bnn_egm_gen_chain.inc), else the
// general-width step, which `wide` splits over the chip in the same way.
enum class BnnEgmDiscRoute { T2_E13, T2_E0, B32_E13, B32_E7, B32_E0, B16_E13, B16_E7, B16_E0, WG };
enum class BnnEgmGenRoute { CHAIN_T2, CHAIN_PAD, CHAIN_N13, CHAIN_N7, STEP };
struct BnnEgmShape { int q, p, B; bool fixed_norm; int dz_hidden; const int *dz; BnnNetDims g, e, f, h; };
struct BnnEgmPlan { BnnEgmDiscRoute disc; BnnEgmGenRoute gen; bool wide; ChainExtent ext; EgmArena arena; int chain_disc_lds, chain_gen_lds; };
constexpr bool bnn_egm_disc_has_enc_chain(BnnEgmDiscRoute r) {
  return r != BnnEgmDiscRoute::T2_E0 && r != BnnEgmDiscRoute::B32_E0 && r != BnnEgmDiscRoute::B16_E0 && r != BnnEgmDiscRoute::WG;
}
constexpr BnnEgmPlan bnn_egm_plan(const BnnEgmShape &s, const EgmSwitches &sw, bool one_launch, size_t chain_disc_bytes, size_t chain_gen_bytes) {
  const ChainExtent x = chain_extent(s.q, s.p);
  const EgmArena arena = egm_arena(s.B, s.dz_hidden, s.dz);
  const bool dshape = chain_disc_ok(s.fixed_norm, s.dz_hidden, s.dz, s.B);
  // the one real difference from the deterministic plan: BGM_EGM_NO_CHAIN switches off the discriminator chain alone, and the generator
  // chain does not ask for it
  const bool dchain = dshape && !sw.no_chain && chain_disc_bytes <= (size_t)EGM_LDS_LIMIT;
  const bool gchain = dshape && chain_extent_ok(x, s.B) && bnn_chain_shapes_ok(s.g, s.e, s.f, s.h, s.q, s.p, true) && !sw.no_chain_gen;
  // the encoder chain of the discriminator step: 13 and 7 input tiles exactly, a narrower p on the 13-tile chain with masked inputs (two
  // latent tiles: 13 only), a wider one in the general form
  const bool ech = s.e.bn_fixed == 1 && !s.e.heads && s.q <= 32 && chain_trunk_ok(s.e.n, 2, -1, s.q) && !sw.no_chain_bnn;
  const int kt = chain_tiles(s.p), etl = !ech || kt > 13 ? 0 : (kt == 7 && x.t0 == 1) ? 7 : 13;
  const BnnEgmDiscRoute disc = !dchain ? BnnEgmDiscRoute::WG
                               : x.t0 == 2 ? (etl == 13 ? BnnEgmDiscRoute::T2_E13 : BnnEgmDiscRoute::T2_E0)
                               : s.B == 32 ? (etl == 13 ? BnnEgmDiscRoute::B32_E13 : etl == 7 ? BnnEgmDiscRoute::B32_E7 : BnnEgmDiscRoute::B32_E0)
                                           : (etl == 13 ? BnnEgmDiscRoute::B16_E13 : etl == 7 ? BnnEgmDiscRoute::B16_E7 : BnnEgmDiscRoute::B16_E0);
  const BnnEgmGenRoute gen = !gchain ? BnnEgmGenRoute::STEP
                             : x.t0 == 2 ? BnnEgmGenRoute::CHAIN_T2
                             : x.pad ? BnnEgmGenRoute::CHAIN_PAD
                             : x.ntl == 13 ? BnnEgmGenRoute::CHAIN_N13 : BnnEgmGenRoute::CHAIN_N7;
  return {disc, gen, !one_launch, x, arena, dchain ? (int)chain_disc_bytes : 0, gchain ? (int)chain_gen_bytes : 0};
}

// ---- the tables pinned at the edges tests/test_egm_edges_host.py and tests/test_gpu_egm_edges.py name
namespace egm_plan_pins {
constexpr bool extent_is(int q, int p, int t0, int ntl_need, int ntl, bool pad) {
  const ChainExtent x = chain_extent(q, p);
  return x.t0 == t0 && x.ntl_need == ntl_need && x.ntl == ntl && x.pad == pad;
}
static_assert(extent_is(10, 95, 1, 6, 13, true) && extent_is(10, 96, 1, 7, 7, false) && extent_is(10, 111, 1, 7, 7, false) && extent_is(10, 112, 1, 8, 13, true),
              "p + 1 opens the seventh tile at 96 and the eighth at 112");
static_assert(extent_is(10, 191, 1, 12, 13, true) && extent_is(10, 192, 1, 13, 13, false) && extent_is(10, 207, 1, 13, 13, false) &&
              extent_is(10, 208, 1, 14, 13, true), "... the thirteenth at 192 and the fourteenth at 208");
static_assert(extent_is(16, 100, 1, 7, 7, false) && extent_is(17, 100, 2, 7, 13, true) && extent_is(32, 200, 2, 13, 13, true) && extent_is(33, 200, 2, 13, 13, true),
              "two latent tiles above q = 16: the masked 13-tile kernels, whatever p (q <= 32 is the predicates' matter)");
static_assert(chain_extent_ok(chain_extent(10, 207), 16) && !chain_extent_ok(chain_extent(10, 208), 32) && chain_extent_ok(chain_extent(10, 95), 32) &&
              !chain_extent_ok(chain_extent(10, 95), 16), "no fourteenth tile; masked extents at B = 32 only");

// the default model of the tests at (p, q, B), a discriminator q-d1-d2-d3-1 and heads 64-32-head: deterministic routes
struct Routes { EgmDiscRoute disc; EgmGenRoute gen; };
constexpr bool operator==(const Routes &a, const Routes &b) { return a.disc == b.disc && a.gen == b.gen; }
constexpr Routes routes(int p, int q, int B, int d1 = 64, int d2 = 32, int d3 = 8, int head = 8, EgmSwitches sw = {false, false, false},
                        bool fixed_norm = true, size_t disc_bytes = 1, size_t gen_bytes = 1) {
  const int dz[5] = {q, d1, d2, d3, 1}, g[7] = {q, 64, 64, 64, 64, 64, p + 1}, e[7] = {p, 64, 64, 64, 64, 64, q}, f[5] = {3, 64, 32, head, 2},
            h[5] = {8, 64, 32, head, 2};
  const EgmPlan pl = egm_plan({q, p, B, fixed_norm, 3, dz, {g, 6}, {e, 6}, {f, 4}, {h, 4}}, sw, disc_bytes, gen_bytes);
  return {pl.disc, pl.gen};
}
using D = EgmDiscRoute;
using G = EgmGenRoute;
// p (tests/_egm_edges_ref.py EXTENT_PAIRS): the discriminator step keys on (p + 15) / 16, the generator step on (p + 16) / 16
static_assert(routes(95, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_PAD} && routes(96, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_32_N7} &&
              routes(111, 10, 32) == Routes{D::CHAIN_32_K7, G::CHAIN_32_N7} && routes(112, 10, 32) == Routes{D::CHAIN_32_K7, G::CHAIN_PAD}, "p = 95, 96, 111, 112");
static_assert(routes(191, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_PAD} && routes(192, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_32_N13} &&
              routes(207, 10, 32) == Routes{D::CHAIN_32_K13, G::CHAIN_32_N13} && routes(208, 10, 32) == Routes{D::CHAIN_32_K13, G::STEP}, "p = 191, 192, 207, 208");
static_assert(routes(96, 10, 16) == Routes{D::CHAIN_16, G::CHAIN_16_N7} && routes(207, 10, 16) == Routes{D::CHAIN_16, G::CHAIN_16_N13} &&
              routes(95, 10, 16) == Routes{D::CHAIN_16, G::STEP} && routes(208, 10, 16) == Routes{D::CHAIN_16, G::STEP}, "B = 16: no masked extent");
// q
static_assert(routes(100, 16, 32) == Routes{D::CHAIN_32_K7, G::CHAIN_32_N7} && routes(100, 17, 32) == Routes{D::CHAIN_T2, G::CHAIN_T2} &&
              routes(100, 32, 32) == Routes{D::CHAIN_T2, G::CHAIN_T2} && routes(100, 33, 32) == Routes{D::LDS, G::STEP} &&
              routes(100, 17, 16) == Routes{D::LDS, G::STEP}, "q = 16, 17, 32, 33; two latent tiles at B = 32 only");
// B
static_assert(routes(100, 10, 16) == Routes{D::CHAIN_16, G::CHAIN_16_N7} && routes(100, 10, 17) == Routes{D::LDS, G::STEP} &&
              routes(100, 10, 31) == Routes{D::LDS, G::STEP} && routes(100, 10, 32) == Routes{D::CHAIN_32_K7, G::CHAIN_32_N7} &&
              routes(100, 10, 33) == Routes{D::LDS, G::STEP}, "B = 16, 17, 31, 32, 33");
// the discriminator's widths: 4 / 2 / 1 tiles
static_assert(routes(100, 10, 32, 48).disc == D::LDS && routes(100, 10, 32, 49).disc == D::CHAIN_32_K7 && routes(100, 10, 32, 64).disc == D::CHAIN_32_K7 &&
              routes(100, 10, 32, 65).disc == D::LDS, "d1 = 48, 49, 64, 65");
static_assert(routes(100, 10, 32, 64, 16).disc == D::LDS && routes(100, 10, 32, 64, 17).disc == D::CHAIN_32_K7 &&
              routes(100, 10, 32, 64, 32).disc == D::CHAIN_32_K7 && routes(100, 10, 32, 64, 33).disc == D::LDS, "d2 = 16, 17, 32, 33");
static_assert(routes(100, 10, 32, 64, 32, 0).disc == D::LDS && routes(100, 10, 32, 64, 32, 1).disc == D::CHAIN_32_K7 &&
              routes(100, 10, 32, 64, 32, 16).disc == D::CHAIN_32_K7 && routes(100, 10, 32, 64, 32, 17).disc == D::LDS, "d3 = 0, 1, 16, 17");
// the heads: the generator step leaves the chains, the discriminator step stays
static_assert(routes(100, 10, 32, 64, 32, 8, 16) == Routes{D::CHAIN_32_K7, G::CHAIN_32_N7} && routes(100, 10, 32, 64, 32, 8, 17) == Routes{D::CHAIN_32_K7, G::STEP},
              "head widths 16 and 17");
// the switches, batch statistics and the LDS limit: a generator chain needs the discriminator chain
static_assert(routes(100, 10, 32, 64, 32, 8, 8, {true, false, false}) == Routes{D::LDS, G::STEP} &&
              routes(100, 10, 32, 64, 32, 8, 8, {false, true, false}) == Routes{D::CHAIN_32_K7, G::STEP} &&
              routes(100, 10, 32, 64, 32, 8, 8, {false, false, true}) == Routes{D::CHAIN_32_K7, G::CHAIN_32_N7}, "BGM_EGM_NO_CHAIN, _GEN; _BNN is the Bayesian plan's");
static_assert(routes(100, 10, 32, 64, 32, 8, 8, {}, false) == Routes{D::LDS, G::STEP} &&
              routes(100, 10, 32, 64, 32, 8, 8, {}, true, EGM_LDS_LIMIT) == Routes{D::CHAIN_32_K7, G::CHAIN_32_N7} &&
              routes(100, 10, 32, 64, 32, 8, 8, {}, true, EGM_LDS_LIMIT + 1) == Routes{D::LDS, G::STEP}, "batch statistics; a chain beyond the LDS limit");
// the workgroup kernel's arena at q = 10, 64-32-8 (tests/test_egm_edges_host.py): 39 rows are the last that fit
constexpr int DZ_DEF[4] = {10, 64, 32, 8};
static_assert(egm_arena(39, 3, DZ_DEF).lds_bytes == 162560 && egm_arena(39, 3, DZ_DEF).in_lds && !egm_arena(40, 3, DZ_DEF).in_lds &&
              (64 + egm_arena(40, 3, DZ_DEF).floats) * sizeof(float) == 166688 && egm_arena(40, 3, DZ_DEF).lds_bytes == 256, "arena of 39 and 40 rows");
static_assert(routes(23, 10, 39, 64, 32, 8, 8, {}, false).disc == D::LDS && routes(23, 10, 40, 64, 32, 8, 8, {}, false).disc == D::GLOBAL, "lds / global");

// ... and the Bayesian routes of the same model (Flipout nets with inference-mode normalisation, no sibling heads)
struct BRoutes { BnnEgmDiscRoute disc; BnnEgmGenRoute gen; };
constexpr bool operator==(const BRoutes &a, const BRoutes &b) { return a.disc == b.disc && a.gen == b.gen; }
constexpr BRoutes broutes(int p, int q, int B, EgmSwitches sw = {false, false, false}, int head = 8, int e_fixed = 1) {
  const int dz[5] = {q, 64, 32, 8, 1}, g[7] = {q, 64, 64, 64, 64, 64, p + 1}, e[7] = {p, 64, 64, 64, 64, 64, q}, f[5] = {3, 64, 32, head, 2},
            h[5] = {8, 64, 32, head, 2};
  const BnnEgmPlan pl = bnn_egm_plan({q, p, B, true, 3, dz, {{g, 6}, 1, 0, 0}, {{e, 6}, e_fixed, 0, 0}, {{f, 4}, 1, 0, 0}, {{h, 4}, 1, 0, 0}}, sw, false, 1, 1);
  return {pl.disc, pl.gen};
}
using BD = BnnEgmDiscRoute;
using BG = BnnEgmGenRoute;
static_assert(broutes(95, 10, 32) == BRoutes{BD::B32_E13, BG::CHAIN_PAD} && broutes(96, 10, 32) == BRoutes{BD::B32_E13, BG::CHAIN_N7} &&
              broutes(111, 10, 32) == BRoutes{BD::B32_E7, BG::CHAIN_N7} && broutes(112, 10, 32) == BRoutes{BD::B32_E7, BG::CHAIN_PAD}, "p = 95, 96, 111, 112");
static_assert(broutes(191, 10, 32) == BRoutes{BD::B32_E13, BG::CHAIN_PAD} && broutes(192, 10, 32) == BRoutes{BD::B32_E13, BG::CHAIN_N13} &&
              broutes(207, 10, 32) == BRoutes{BD::B32_E13, BG::CHAIN_N13} && broutes(208, 10, 32) == BRoutes{BD::B32_E13, BG::STEP} &&
              broutes(209, 10, 32) == BRoutes{BD::B32_E0, BG::STEP}, "p = 191, 192, 207, 208; the general encoder beyond 13 input tiles");
static_assert(broutes(45, 10, 16) == BRoutes{BD::B16_E13, BG::STEP} && broutes(100, 10, 16) == BRoutes{BD::B16_E7, BG::CHAIN_N7} &&
              broutes(200, 10, 16) == BRoutes{BD::B16_E13, BG::CHAIN_N13} && broutes(209, 10, 16) == BRoutes{BD::B16_E0, BG::STEP}, "B = 16");
static_assert(broutes(100, 16, 32) == BRoutes{BD::B32_E7, BG::CHAIN_N7} && broutes(100, 17, 32) == BRoutes{BD::T2_E13, BG::CHAIN_T2} &&
              broutes(209, 32, 32) == BRoutes{BD::T2_E0, BG::STEP} && broutes(100, 33, 32) == BRoutes{BD::WG, BG::STEP} &&
              broutes(100, 17, 16) == BRoutes{BD::WG, BG::STEP}, "q = 16, 17, 32, 33");
static_assert(broutes(100, 10, 17) == BRoutes{BD::WG, BG::STEP} && broutes(100, 10, 31) == BRoutes{BD::WG, BG::STEP} && broutes(100, 10, 33) == BRoutes{BD::WG, BG::STEP},
              "B = 17, 31, 33");
static_assert(broutes(100, 10, 32, {true, false, false}) == BRoutes{BD::WG, BG::CHAIN_N7} && broutes(100, 10, 32, {false, true, false}) == BRoutes{BD::B32_E7, BG::STEP} &&
              broutes(100, 10, 32, {false, false, true}) == BRoutes{BD::B32_E0, BG::CHAIN_N7}, "each switch: the generator chain stays under BGM_EGM_NO_CHAIN");
static_assert(broutes(100, 10, 32, {}, 16) == BRoutes{BD::B32_E7, BG::CHAIN_N7} && broutes(100, 10, 32, {}, 17) == BRoutes{BD::B32_E7, BG::STEP} &&
              broutes(100, 10, 32, {}, 8, 0) == BRoutes{BD::B32_E0, BG::STEP}, "head widths 16 and 17; an encoder on batch statistics");
}      // namespace egm_plan_pins
