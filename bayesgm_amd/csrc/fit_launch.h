// fit_launch.h -- host-side decisions of the fit paths (fit_api.hip, bnn_api.hip) as plain functions of plain values: the development
// switches, the Adam step size, which row-tile-chain variant a minibatch runs (fit_chain_launch) and which mode an epoch call runs in
// (fit_epoch_impl).  No HIP and no kernel here: which kernels a unit instantiates is decided where a FitVariant is mapped to them.
#pragma once
#include <cmath>
#include <cstdlib>

// ---- development switches of the fit paths (BGM_FIT_*): read from the environment once per process
struct FitDevSwitches {
  bool no_chain;            // BGM_FIT_NO_CHAIN: the row-tile chains decline every model (the LDS-blob / general-width step kernels instead)
  bool one_wg;              // BGM_FIT_ONE_WG: a phase's chains in one workgroup (dev A/B)
  bool no_workers;          // BGM_FIT_NO_WORKERS: g's last layer on the chain wave alone (dev A/B)
  bool no_overlap;          // BGM_FIT_NO_OVERLAP: the epoch calls on the caller's stream alone (dev A/B)
  bool no_fused_adam;       // BGM_FIT_NO_FUSED_ADAM: separate Adam launch + explicit row marks (dev A/B)
  bool no_replay_ahead;     // BGM_FIT_NO_REPLAY_AHEAD (dev A/B)
  bool no_flags;            // BGM_FIT_NO_FLAGS: the two streams ordered by HIP events (dev A/B)
  int epoch_depth;          // BGM_FIT_EPOCH_DEPTH: parameter buffers in the ring (2..4)
};
static inline const FitDevSwitches &fit_dev_switches() {
  auto on = [](const char *name) { return std::getenv(name) != nullptr; };
  static const FitDevSwitches sw{on("BGM_FIT_NO_CHAIN"), on("BGM_FIT_ONE_WG"), on("BGM_FIT_NO_WORKERS"), on("BGM_FIT_NO_OVERLAP"), on("BGM_FIT_NO_FUSED_ADAM"),
                                 on("BGM_FIT_NO_REPLAY_AHEAD"), on("BGM_FIT_NO_FLAGS"), on("BGM_FIT_EPOCH_DEPTH") ? std::atoi(std::getenv("BGM_FIT_EPOCH_DEPTH")) : 4};
  return sw;
}

// Keras Adam's bias-corrected step size at step t (in double, rounded once)
static inline float adam_lr_t(float lr, long long t, float b1, float b2) {
  return (float)((double)lr * std::sqrt(1.0 - std::pow((double)b2, (double)t)) / (1.0 - std::pow((double)b1, (double)t)));
}

// ---- the row-tile chains (fit_chain.h) of one minibatch.  ntl: 16-wide output tiles of g (13 or 7), t0: latent input tiles, pad: the
// 13-tile kernels on a narrower p + 1 (fit_chain_setup); rows: the minibatch, one row tile up to 16 rows, two up to 32.
//   T2, PAD      two row tiles in one workgroup (the padded / two-latent-tile instantiations are compiled for two only)
//   FS13, FS7    17..32 rows: the two row tiles on two workgroups -- on one CU the six chain waves share one address unit for their
//                weight streams (83.0 -> 77.4 us per minibatch at N = 1e6) -- and, in the theta phase (no cross-network term), one
//                network per workgroup as well (-> 75.8 us); g's last layer over the idle waves of its workgroup
//   FSN13, FSN7  the same grid without the worker waves (BGM_FIT_NO_WORKERS)
//   FW13, FW7    <= 16 rows (a rank's share under data parallelism): the same worker split, one row tile
//   FC<ntl>_<nb> everything of nb row tiles in one workgroup (BGM_FIT_ONE_WG; one row tile under BGM_FIT_NO_WORKERS: one network per
//                workgroup in the theta phase all the same)
enum class FitVariant { T2, PAD, FSN13, FS13, FSN7, FS7, FW13, FW7, FC13_2, FC13_1, FC7_2, FC7_1 };
// nchain: workgroups of the latent phase's chains (the replay riders follow them); grid_x, grid_y: the theta phase's row tiles x networks;
// dw_nb: row tiles the gradient-tile kernel runs over
struct FitChainPlan { FitVariant id; int nchain, grid_x, grid_y, dw_nb; };
constexpr FitChainPlan fit_chain_plan(int ntl, int t0, bool pad, int rows, bool one_wg, bool no_workers) {
  const int nb = rows <= 16 ? 1 : 2;
  const bool n13 = ntl == 13;
  if (t0 == 2) return {FitVariant::T2, 1, 1, 1, 2};
  if (pad) return {FitVariant::PAD, 1, 1, 1, 2};
  if (nb == 2 && !one_wg) return {no_workers ? (n13 ? FitVariant::FSN13 : FitVariant::FSN7) : (n13 ? FitVariant::FS13 : FitVariant::FS7), 2, 2, 3, 2};
  if (nb == 1 && !one_wg && !no_workers) return {n13 ? FitVariant::FW13 : FitVariant::FW7, 1, 1, 3, 1};
  return {nb == 2 ? (n13 ? FitVariant::FC13_2 : FitVariant::FC7_2) : (n13 ? FitVariant::FC13_1 : FitVariant::FC7_1), 1, 1, one_wg ? 1 : 3, nb};
}
constexpr bool operator==(const FitChainPlan &a, const FitChainPlan &b) {
  return a.id == b.id && a.nchain == b.nchain && a.grid_x == b.grid_x && a.grid_y == b.grid_y && a.dw_nb == b.dw_nb;
}

// the table without switches, under the names tests/_fit_epoch_cases.py plan() gives the variants: both edges of a row class (1 and 16
// rows, or 17 and 32) give the row `want`
constexpr bool fit_plan_is(int ntl, int t0, bool pad, bool two_row_tiles, FitChainPlan want) {
  return fit_chain_plan(ntl, t0, pad, two_row_tiles ? 17 : 1, false, false) == want && fit_chain_plan(ntl, t0, pad, two_row_tiles ? 32 : 16, false, false) == want;
}
static_assert(fit_plan_is(13, 1, false, false, {FitVariant::FW13, 1, 1, 3, 1}) && fit_plan_is(13, 1, false, true, {FitVariant::FS13, 2, 2, 3, 2}), "unpadded, 13 tiles");
static_assert(fit_plan_is(7, 1, false, false, {FitVariant::FW7, 1, 1, 3, 1}) && fit_plan_is(7, 1, false, true, {FitVariant::FS7, 2, 2, 3, 2}), "unpadded, 7 tiles");
static_assert(fit_plan_is(13, 1, true, false, {FitVariant::PAD, 1, 1, 1, 2}) && fit_plan_is(13, 1, true, true, {FitVariant::PAD, 1, 1, 1, 2}), "padded");
static_assert(fit_plan_is(7, 1, true, false, {FitVariant::PAD, 1, 1, 1, 2}) && fit_plan_is(7, 1, true, true, {FitVariant::PAD, 1, 1, 1, 2}), "pad wins over the tile count");
static_assert(fit_plan_is(13, 2, true, false, {FitVariant::T2, 1, 1, 1, 2}) && fit_plan_is(13, 2, true, true, {FitVariant::T2, 1, 1, 1, 2}), "two latent tiles");
static_assert(fit_plan_is(13, 2, false, false, {FitVariant::T2, 1, 1, 1, 2}) && fit_plan_is(13, 2, false, true, {FitVariant::T2, 1, 1, 1, 2}), "... win over pad");
static_assert(fit_plan_is(7, 2, false, false, {FitVariant::T2, 1, 1, 1, 2}) && fit_plan_is(7, 2, false, true, {FitVariant::T2, 1, 1, 1, 2}) &&
              fit_plan_is(7, 2, true, false, {FitVariant::T2, 1, 1, 1, 2}) && fit_plan_is(7, 2, true, true, {FitVariant::T2, 1, 1, 1, 2}), "... and over the tile count");
// ... and under the switches (ntl, t0, pad, rows, one_wg, no_workers): the forms they alone reach, with their grids
static_assert(fit_chain_plan(13, 1, false, 32, false, true) == FitChainPlan{FitVariant::FSN13, 2, 2, 3, 2} &&
              fit_chain_plan(7, 1, false, 17, false, true) == FitChainPlan{FitVariant::FSN7, 2, 2, 3, 2} &&
              fit_chain_plan(13, 1, false, 16, false, true) == FitChainPlan{FitVariant::FC13_1, 1, 1, 3, 1} &&
              fit_chain_plan(7, 1, false, 1, false, true) == FitChainPlan{FitVariant::FC7_1, 1, 1, 3, 1}, "no workers");
static_assert(fit_chain_plan(13, 1, false, 32, true, false) == FitChainPlan{FitVariant::FC13_2, 1, 1, 1, 2} &&
              fit_chain_plan(13, 1, false, 16, true, true) == FitChainPlan{FitVariant::FC13_1, 1, 1, 1, 1} &&
              fit_chain_plan(7, 1, false, 17, true, true) == FitChainPlan{FitVariant::FC7_2, 1, 1, 1, 2} &&
              fit_chain_plan(7, 1, false, 16, true, false) == FitChainPlan{FitVariant::FC7_1, 1, 1, 1, 1}, "one workgroup");

// ---- the mode of one bgm_causal_fit_epoch call.  chains: the session has the row-tile chains; dp: a rank's share of a data-parallel epoch
struct FitEpochMode {
  bool overlap;             // the latent phase of minibatch k on a second stream beside the theta phase of minibatch k + 1
  // D parameter buffers in a ring: step k's Adam reads buffer k % D and writes the next one, so the latent phase of minibatch k (reading
  // the new buffer) holds up nothing before the parameter update of minibatch k + D - 1, which overwrites the buffer the latent phase
  // k - 1 read.  With D = 2 the cycle  latent phase k -> (event) -> theta phase k + 2 -> (event) -> latent phase k + 2  carries two
  // cross-stream hops of ~10 us per two minibatches (46.3 us per minibatch measured = 36 + 10); D = 4 spreads them over four.
  int D;
  // chained: the machinery of the row-tile chains (replay ahead, device-side ordering, rows stamped by the latent step) is on;
  // fuse: the Adam step rides on the gradient-tile kernel -- not under data parallelism, where the all-reduce sits between the tiles
  // and Adam: there the step is its own launch that waits / counts like the tiles would (fit_adam_theta_sync_kernel)
  bool chained, fuse;
  // Replay mode: the pending zero-gradient steps of minibatch j's rows are replayed D minibatches ahead, on the second stream behind
  // the latent phase j - D -- off the parameter stream's critical path (replay + chains + gradient tiles), and covered by the event the
  // theta phase j waits for anyway.  Legal because the minibatches of one call are disjoint: nothing touches those rows in between,
  // and the step a replay runs to (the latent step count when minibatch j starts) is known in advance.
  bool ahead;
  // Ordering between the two streams without events (each record / wait pair costs the stream it sits in 4-6 us of command-processor
  // time: 45.0 us per minibatch with them, 34.7 with the dependencies dropped -- unsafe, measured for the bound): the gradient-tile
  // kernel counts its workgroups into a device counter the latent phase's kernel spins on at entry, and the latent kernel's workgroups
  // (chains + replay riders) count into a second one the theta phase D minibatches later waits for (fit_sync.h FitSync).
  // wants_flags: the mode allows it; whether the two streams really run side by side is probed per handle (epoch_flags_begin)
  bool wants_flags;
};
constexpr FitEpochMode fit_epoch_mode(int lazy, bool chains, int batch, bool dp, const FitDevSwitches &sw) {
  const bool overlap = !sw.no_overlap && lazy != 0 && chains && batch <= 32;
  const int D = !overlap ? 1 : sw.epoch_depth < 2 ? 2 : sw.epoch_depth > 4 ? 4 : sw.epoch_depth;
  const bool chained = overlap && !sw.no_fused_adam, ahead = chained && lazy == 2 && !sw.no_replay_ahead;
  return {overlap, D, chained, chained && !dp, ahead, chained && !sw.no_flags && (lazy != 2 || ahead)};
}
