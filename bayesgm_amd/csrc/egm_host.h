// egm_host.h -- host side shared by the four EGM warm-start sessions (egm_api.hip, bnn_egm_api.hip, bgm_egm_api.hip, bgmb_egm_api.hip):
// the discriminator's parameter layout, the session core (Adam rule and counters, the regions behind read / write / grad / apply), the
// transposed mirror and the gradient-tile table of the generator chains (also fit_api.hip), and the development clock of the
// deterministic steps.  Host only: no kernel text.  Include it behind the unit's kernel headers: it names the types and the two
// elementwise kernels of egm_kernels.h and adds no kernel header to a unit.  The decisions are in egm_plan.h.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "bgm_host.h"
#include "egm_kernels.h"
#include "egm_plan.h"
#include "fit_launch.h"

static constexpr int EGM_WAVES = EGM_THREADS / 64;      // of every step kernel, workgroup or chain (ECH_WAVES)
inline NetDims egm_dims(const EgmMlp &m) { return {m.dims, m.n_layers}; }

// ---- discriminator parameters: W0..WL | b0..bL | gamma0..gamma(L-1) | beta0..beta(L-1); batch statistics until the caller says
// otherwise.  Returns the parameter count.
inline int egm_fill_disc(EgmDisc &d, int in_dim, int n_hidden, const int32_t *units) {
  d.n_hidden = n_hidden;
  d.dims[0] = in_dim;
  for (int l = 0; l < n_hidden; ++l) d.dims[l + 1] = units[l];
  d.dims[n_hidden + 1] = 1;
  int o = 0;
  for (int l = 0; l <= n_hidden; ++l) { d.w[l] = o; o += d.dims[l] * d.dims[l + 1]; }
  for (int l = 0; l <= n_hidden; ++l) { d.b[l] = o; o += d.dims[l + 1]; }
  for (int l = 0; l < n_hidden; ++l) { d.gamma[l] = o; o += d.dims[l + 1]; }
  for (int l = 0; l < n_hidden; ++l) { d.beta[l] = o; o += d.dims[l + 1]; }
  d.n_params = o;
  egm_finish_disc(d);
  d.fixed_norm = 0;
  return o;
}

// ---- what every session keeps.  Sides: 0 the generator side (g | e | ...), 1 the discriminator(s)
struct EgmRegion { float *ptr = nullptr; size_t n = 0; };
struct EgmCore {
  float lr = 0.0f, b1 = 0.0f, b2 = 0.0f, eps = 0.0f;      // the session's Keras Adam
  long long t[2] = {0, 0};                                // iterations of g_pre_optimizer / d_pre_optimizer
  EgmRegion region[4];                                    // what = 0, 1: the parameters of the two sides; 2, 3: their gradients
  float *m[2] = {nullptr, nullptr}, *v[2] = {nullptr, nullptr};      // Adam slots of the two sides
  void set_adam(float lr_, float b1_, float b2_, float eps_) { lr = lr_; b1 = b1_; b2 = b2_; eps = eps_; }
  void set_side(int side, float *theta, float *m_, float *v_, float *grad, size_t n) {
    region[side] = {theta, n}; region[2 + side] = {grad, n}; m[side] = m_; v[side] = v_;
  }
  // the Adam record of one step of a side; apply: the step counts as an iteration
  EgmAdam adam(int side, bool apply) {
    if (apply) t[side] += 1;
    return {adam_lr_t(lr, std::max<long long>(1, t[side]), b1, b2), b1, b2, eps};
  }
};

// what -> region; `who` names the entry points in the error
inline int egm_region(const EgmCore &c, const char *who, int32_t what, EgmRegion &r) {
  if (what < 0 || what > 3) { bgm_set_error(std::string(who) + ": what must be 0..3"); return BGM_E_INVALID; }
  r = c.region[what];
  return BGM_OK;
}
// the bodies of <session>_read / _write behind their entry checks
inline int egm_read(const EgmCore &c, int device, const char *fn, const char *who, int32_t what, float *host, int64_t count, hipStream_t stream) {
  EgmRegion r;
  if (int rc = egm_region(c, who, what, r)) return rc;
  if ((size_t)count != r.n) { bgm_set_error(std::string(fn) + ": expected " + std::to_string(r.n) + " floats"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(device));
  BGM_HIP_CHECK(hipStreamSynchronize(stream));
  BGM_HIP_CHECK(hipMemcpy(host, r.ptr, r.n * sizeof(float), hipMemcpyDeviceToHost));
  return BGM_OK;
}
inline int egm_write(const EgmCore &c, int device, const char *fn, const char *who, int32_t what, const float *host, int64_t count, hipStream_t stream) {
  EgmRegion r;
  if (int rc = egm_region(c, who, what, r)) return rc;
  if (what > 1 || (size_t)count != r.n) { bgm_set_error(std::string(fn) + ": parameters only, expected " + std::to_string(r.n) + " floats"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(device));
  BGM_HIP_CHECK(hipStreamSynchronize(stream));
  BGM_HIP_CHECK(hipMemcpy(r.ptr, host, r.n * sizeof(float), hipMemcpyHostToDevice));
  return BGM_OK;
}
// ... of <session>_grad (the side's gradient, scaled, for the all-reduce of a data-parallel step) and _apply (Adam on the reduced
// gradient; thetaT / mirror: the transposed copy a session with generator chains keeps current)
inline int egm_grad(const EgmCore &c, int device, const char *fn, int32_t which, float scale, float *grad_dev, int64_t count, hipStream_t stream) {
  const size_t n = c.region[which == 0 ? 0 : 1].n;
  if ((which != 0 && which != 1) || !grad_dev || (size_t)count != n) {
    bgm_set_error(std::string(fn) + ": which must be 0 (g|e|f|h: " + std::to_string(c.region[0].n) + " floats) or 1 (discriminator: " +
                  std::to_string(c.region[1].n) + ")");
    return BGM_E_INVALID;
  }
  BGM_HIP_CHECK(hipSetDevice(device));
  hipLaunchKernelGGL(egm_dp_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, c.region[2 + which].ptr, grad_dev, (int)n, scale);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}
inline int egm_apply(EgmCore &c, int device, const char *fn, int32_t which, const float *grad_dev, int64_t count, hipStream_t stream, float *thetaT = nullptr,
                     const int *mirror = nullptr) {
  const size_t n = c.region[which == 0 ? 0 : 1].n;
  if ((which != 0 && which != 1) || !grad_dev || (size_t)count != n) { bgm_set_error(std::string(fn) + ": bad which / count"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(device));
  const EgmAdam ad = c.adam(which, true);
  hipLaunchKernelGGL(egm_dp_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, c.region[which].ptr, c.m[which], c.v[which], grad_dev, (int)n, ad,
                     which == 0 ? thetaT : nullptr, which == 0 ? mirror : nullptr);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

// ---- the two BGM sessions (bgm_egm_api.hip, bgmb_egm_api.hip: Args = BgmEgmArgs / BgmbEgmArgs) differ in their generator alone
static constexpr int BGM_EGM_LDS = 64 * (int)sizeof(float);      // the reduction words of their workgroup kernels
template <class Args>
struct BgmEgmSession {
  bgm_bgm_egm_config cfg{};
  Args base{};
  EgmCore core;
  size_t n_g = 0, n_e = 0, n_gen = 0, n_dz = 0, n_dx = 0, n_disc = 0, ws_floats = 0, enc_ws_per_block = 0;
  float *dev = nullptr;      // one allocation: theta_g|m_g|v_g|grad_g|theta_d|m_d|v_d|grad_d|ws
  float *enc_ws = nullptr;   // workspace of the whole-panel encoder passes
  int enc_blocks = 0;
  ~BgmEgmSession() {
    if (dev) hipFree(dev);
    if (enc_ws) hipFree(enc_ws);
  }
};
// the encoder p -> q behind the generator's n_g parameters and the two discriminators, from the configuration: fills base.e / dz / dx and
// the counts, and checks them against what the caller brought
template <class Args>
inline int bgm_egm_describe(BgmEgmSession<Args> &s, const char *fn, int q, int p, int disc_norm, int64_t count_e, int64_t count_dz, int64_t count_dx) {
  const bgm_bgm_egm_config &cfg = s.cfg;
  EgmMlp &e = s.base.e;
  e.n_layers = cfg.n_hidden_e + 1;
  e.dims[0] = p;
  for (int i = 0; i < cfg.n_hidden_e; ++i) e.dims[i + 1] = cfg.e_units[i];
  e.dims[cfg.n_hidden_e + 1] = q;
  e.off = (int)s.n_g;
  egm_finish_mlp(e);
  s.n_e = 0;
  for (int l = 0; l < e.n_layers; ++l) s.n_e += (size_t)e.dims[l] * e.dims[l + 1] + e.dims[l + 1];
  s.n_gen = s.n_g + s.n_e;
  s.n_dz = (size_t)egm_fill_disc(s.base.dz, q, cfg.n_hidden_dz, cfg.dz_units);
  s.n_dx = (size_t)egm_fill_disc(s.base.dx, p, cfg.n_hidden_dx, cfg.dx_units);
  s.base.dz.fixed_norm = s.base.dx.fixed_norm = disc_norm;
  s.n_disc = s.n_dz + s.n_dx;
  if ((int64_t)s.n_e != count_e || (int64_t)s.n_dz != count_dz || (int64_t)s.n_dx != count_dx) {
    bgm_set_error(std::string(fn) + ": expected " + std::to_string(s.n_e) + " / " + std::to_string(s.n_dz) + " / " + std::to_string(s.n_dx) +
                  " encoder / dz / dx parameters");
    return BGM_E_INVALID;
  }
  return BGM_OK;
}
// the session's allocation, `slack` floats behind the workspace, and the parameters the host brings (the generator's own are the caller's)
template <class Args>
inline int bgm_egm_allocate(BgmEgmSession<Args> &s, size_t slack, size_t enc_widths, int n_cus, const float *theta_e_host, const float *theta_dz_host,
                            const float *theta_dx_host) {
  Args &a = s.base;
  const size_t total = 4 * s.n_gen + 4 * s.n_disc + s.ws_floats + slack;
  BGM_HIP_CHECK(hipMalloc(&s.dev, total * sizeof(float)));
  BGM_HIP_CHECK(hipMemset(s.dev, 0, total * sizeof(float)));
  float *pp = s.dev;
  auto take = [&](size_t n) { float *r = pp; pp += (n + 3) / 4 * 4; return r; };
  a.theta_g = take(s.n_gen); a.m_g = take(s.n_gen); a.v_g = take(s.n_gen); a.grad_g = take(s.n_gen);
  a.theta_d = take(s.n_disc); a.m_d = take(s.n_disc); a.v_d = take(s.n_disc); a.grad_d = take(s.n_disc);
  a.ws = take(s.ws_floats);
  s.core.set_side(0, a.theta_g, a.m_g, a.v_g, a.grad_g, s.n_gen);
  s.core.set_side(1, a.theta_d, a.m_d, a.v_d, a.grad_d, s.n_disc);
  BGM_HIP_CHECK(hipMemcpy(a.theta_g + s.n_g, theta_e_host, s.n_e * sizeof(float), hipMemcpyHostToDevice));
  BGM_HIP_CHECK(hipMemcpy(a.theta_d, theta_dz_host, s.n_dz * sizeof(float), hipMemcpyHostToDevice));
  BGM_HIP_CHECK(hipMemcpy(a.theta_d + s.n_dz, theta_dx_host, s.n_dx * sizeof(float), hipMemcpyHostToDevice));
  s.enc_blocks = n_cus;
  s.enc_ws_per_block = (size_t)64 * (enc_widths + 8) + 64;
  BGM_HIP_CHECK(hipMalloc(&s.enc_ws, s.enc_ws_per_block * s.enc_blocks * sizeof(float)));
  return BGM_OK;
}
// z = e(x) over a whole panel, 64 rows per workgroup pass (kernel: bgm_egm_encode_kernel, which the unit instantiates)
template <class Args, class K>
inline int bgm_egm_encode(const BgmEgmSession<Args> &s, K kernel, int device, const char *fn, const float *x_dev, int64_t n, float *z_dev, hipStream_t stream) {
  if (n <= 0) return BGM_OK;
  if (!x_dev || !z_dev) { bgm_set_error(std::string(fn) + ": NULL pointer"); return BGM_E_INVALID; }
  BGM_HIP_CHECK(hipSetDevice(device));
  const int B = 64;
  const int grid = (int)std::max<long long>(1, std::min<long long>((n + B - 1) / B, s.enc_blocks));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(EGM_THREADS), BGM_EGM_LDS, stream, s.base.e, s.base.theta_g, x_dev, (long long)n, z_dev, s.enc_ws,
                     (long long)s.enc_ws_per_block, B);
  BGM_HIP_CHECK(hipGetLastError());
  return BGM_OK;
}

#ifdef ECG_TILE_INTS      // ---- units with the generator chains (egm_chain_gen.h, fit_chain.h in front of this header)
// transposed mirror of a net's weight matrices (the backward chains read W^T rows contiguously) and where each parameter's copy lives in
// it (-1: biases), for the Adam step that keeps it current
inline void egm_mirror_add(const EgmMlp &m, const float *theta, std::vector<float> &tT, std::vector<int> &mdst) {
  for (int l = 0; l < m.n_layers; ++l) {
    const int ni = m.dims[l], no = m.dims[l + 1];
    for (int f = 0; f < ni; ++f)
      for (int o = 0; o < no; ++o) {
        tT[m.woff[l] + (size_t)o * ni + f] = theta[m.woff[l] + (size_t)f * no + o];
        mdst[m.woff[l] + (size_t)f * no + o] = m.woff[l] + o * ni + f;
      }
  }
}
// weight-gradient tiles of a net: (layer, 16 input features, 16 output features) with the stash offsets x0 / d0 of the pass that feeds
// the layer (x1 / d1: a second pass, or NULL) and the padded widths xw / dw of the stashes, per layer
inline void egm_tiles_add(const EgmMlp &m, const int *x0, const int *x1, const int *d0, const int *d1, const int *xw, const int *dw, std::vector<int> &tiles) {
  for (int l = 0; l < m.n_layers; ++l) {
    const int ni = m.dims[l], no = m.dims[l + 1];
    for (int u = 0; u < chain_tiles(ni); ++u)
      for (int v = 0; v < chain_tiles(no); ++v) {
        const int e[ECG_TILE_INTS] = {x0[l], x1 ? x1[l] : -1, d0[l], d1 ? d1[l] : -1, xw[l], dw[l], u, v, m.woff[l], ni, no, u == 0 ? m.woff[l] + ni * no : -1, 0, 0, 0, 0};
        tiles.insert(tiles.end(), e, e + ECG_TILE_INTS);
      }
  }
}
#endif

// ---- -DEGM_PHASE_CLOCK (development, never in the shipped library): the cycle stamps of one deterministic step, printed at the 40th call
// of each (step, kernel family).  begin() in front of the step's launches, report() behind them.
struct EgmPhaseClock {
#ifdef EGM_PHASE_CLOCK
  static unsigned long long *buf() {
    static unsigned long long *b = nullptr;
    if (!b) hipMalloc(&b, sizeof(unsigned long long) * 8192);
    return b;
  }
  static void begin(EgmArgs &a, hipStream_t stream) {
    a.stamps = buf();
    hipMemsetAsync(a.stamps, 0, sizeof(unsigned long long) * 8192, stream);
  }
  static void report(const char *what, bool chain) {
    static int calls[2][2] = {};
    if (++calls[what[0] == 'g'][chain] != 40) return;
    hipDeviceSynchronize();
    std::vector<unsigned long long> st(8192);
    hipMemcpy(st.data(), buf(), sizeof(unsigned long long) * 8192, hipMemcpyDeviceToHost);
    if (!chain) {      // the workgroup kernels: (source line, cycles since the barrier before) per EGM_STAMP
      fprintf(stderr, "EGM_PHASE %s\n", what);
      for (int i = 1; i < 4096 && st[2 * i]; ++i) fprintf(stderr, "EGM_PHASE %s %3d line %4llu cycles %8llu\n", what, i, st[2 * i], st[2 * i + 1] - st[2 * i - 1]);
      return;
    }
    for (int w = 0; w < 8; ++w) {      // the chains: cycles between the ECH_STAMPs of each wave
      const unsigned long long *t = st.data() + 4096 + w * 16;
      fprintf(stderr, "ECH_PHASE %s wave %d:", what, w);
      for (int k = 1; k < 16; ++k) if (t[k] && t[k - 1]) fprintf(stderr, " %d:%llu", k, t[k] - t[k - 1]);
      if (t[8]) fprintf(stderr, "  enc_start-k0:%llu", t[8] - t[0]);
      fprintf(stderr, "\n");
    }
  }
#else
  static void begin(EgmArgs &, hipStream_t) {}
  static void report(const char *, bool) {}
#endif
};
