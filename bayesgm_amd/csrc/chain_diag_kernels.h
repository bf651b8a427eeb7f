// chain_diag_kernels.h -- split R-hat and effective sample size of every sampled series, float64 sums over float32 draws.
//
// Feeds bayesgm_amd.diagnostics.chain_diagnostics.  draws: [n_chains x n_draws x n_series] float32 (the draws_dev layout of the
// samplers with n_series = n * q: neighbouring series are contiguous).  With h = n_draws / 2 every chain is cut into its first
// and its next h draws (m = 2 n_chains half-chains); the definitions are the Stan / ArviZ "mean" forms without rank
// normalisation (include/bgm_hip.h, bgm_chain_diagnostics).
//
// Two kernels, both with a fixed summation order (no atomics: repeated calls are bit-identical):
//
//   chain_diag_means_kernel   one thread per series walks its draws once (rows are coalesced over the threads of a wave):
//                             half-chain means, the mean of all draws, min / max, the number of moves, the non-finite flag.
//   chain_diag_acov_kernel    a workgroup owns CD_TILE = 16 consecutive series and 16 * G threads, G = n_lags / 16 lag groups.
//                             Thread (s, g) keeps the 16 lag sums  sum_t d[t] d[t + 16 g + k], k < 16, of series s in registers,
//                             summed over all half-chains (acov(k) is their mean, W comes from k = 0).  A half-chain is streamed
//                             through LDS as centred float64 rows [time][series]: CD_CHUNK new rows per step behind a lookahead
//                             of 16 G + CD_LT rows, rows past the end of the half-chain are zero, so no product crosses into
//                             another half-chain and the inner loop has no bounds.  Per step a thread multiplies CD_LT = 8 rows
//                             d[t .. t+7] into a window of 23 rows: 31 ds_read_b64 feed 128 v_fma_f64.  The row pitch of
//                             CD_TILE + 1 doubles puts the lag groups g and g + 1 of one 32-lane half on disjoint banks.
//                             After the last half-chain the lag sums go to LDS and thread (s, 0) finishes series s: W, B, var+,
//                             R-hat, Geyer's initial monotone sequence, ESS, MCSE.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

constexpr int CD_TILE = 16;                 // series per workgroup
constexpr int CD_LG = 16;                   // lags per thread
constexpr int CD_LT = 8;                    // time rows per register block
constexpr int CD_PITCH = CD_TILE + 1;       // doubles per LDS row
constexpr int CD_MAX_CHAINS = 8;
constexpr int CD_MAX_LAG = 1024;

constexpr int CD_FLAG_CONSTANT = 1, CD_FLAG_TRUNCATED = 2, CD_FLAG_NONFINITE = 4;

struct ChainDiagShape {
  long long n_series;
  int n_chains, n_draws;
  int h;            // draws per half-chain
  int m;            // half-chains
  int max_lag;      // clamped
  int n_lags;       // lags 0 .. n_lags - 1 enter the Geyer pairs (even)
  int groups;       // lag groups of CD_LG
  int look;         // lookahead rows: CD_LG * groups + CD_LT
  int chunk;        // new rows per step (multiple of CD_LT)
};

// workspace (doubles): [m x n_series] half-chain means, then [n_series] the squared distance of the draws outside every
// half-chain (the odd last draw of each chain) from the mean of all draws.
__global__ __launch_bounds__(256) void chain_diag_means_kernel(const float *__restrict__ draws, ChainDiagShape sh,
                                                                double *__restrict__ out, int *__restrict__ flags,
                                                                double *__restrict__ ws) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= sh.n_series) return;
  const long long ns = sh.n_series;
  double total = 0.0, moves = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  bool finite = true;
  for (int c = 0; c < sh.n_chains; ++c) {
    const float *p = draws + (long long)c * sh.n_draws * ns + s;
    float prev = p[0];
    double chain_sum = 0.0;
    for (int half = 0; half < 2; ++half) {
      double sum = 0.0;
      const int t0 = half * sh.h;
#pragma unroll 8
      for (int t = t0; t < t0 + sh.h; ++t) {
        const float x = p[(long long)t * ns];
        sum += (double)x;
        moves += (x != prev) ? 1.0 : 0.0;
        finite = finite && (fabsf(x) <= 3.402823466e38f);
        lo = fminf(lo, x); hi = fmaxf(hi, x);
        prev = x;
      }
      ws[(long long)(2 * c + half) * ns + s] = sum / (double)sh.h;
      chain_sum += sum;
    }
    if (sh.n_draws & 1) {
      const float x = p[(long long)(sh.n_draws - 1) * ns];
      chain_sum += (double)x;
      moves += (x != prev) ? 1.0 : 0.0;
      finite = finite && (fabsf(x) <= 3.402823466e38f);
      lo = fminf(lo, x); hi = fmaxf(hi, x);
    }
    total += chain_sum;
  }
  const double mean = total / ((double)sh.n_chains * (double)sh.n_draws);
  double extra = 0.0;
  if (sh.n_draws & 1)
    for (int c = 0; c < sh.n_chains; ++c) {
      const double d = (double)draws[((long long)c * sh.n_draws + sh.n_draws - 1) * ns + s] - mean;
      extra += d * d;
    }
  ws[(long long)sh.m * ns + s] = extra;
  const double nan = __builtin_nan("");
  int f = 0;
  if (!finite) f = CD_FLAG_NONFINITE;
  else if (lo == hi) f = CD_FLAG_CONSTANT;
  out[s] = finite ? mean : nan;
  out[5 * ns + s] = finite ? moves : nan;
  flags[s] = f;                              // chain_diag_acov_kernel adds CD_FLAG_TRUNCATED
}

// rows [r0, r1) of the LDS image <- centred draws of times tbase + r (zero at and past the end of the half-chain)
__device__ inline void cd_stage_rows(double *lds, const float *__restrict__ src, long long ns, long long s0, int n_valid, int h, int tbase,
                                     int r0, int r1, const double *mean_tile, int tid, int n_threads) {
  const int count = (r1 - r0) * CD_TILE;
  for (int e = tid; e < count; e += n_threads) {
    const int r = r0 + e / CD_TILE, j = e % CD_TILE;
    const int t = tbase + r;
    double v = 0.0;
    if (t < h && j < n_valid) v = (double)src[(long long)t * ns + s0 + j] - mean_tile[j];
    lds[r * CD_PITCH + j] = v;
  }
}

__global__ __launch_bounds__(CD_TILE * (CD_MAX_LAG / CD_LG)) void chain_diag_acov_kernel(const float *__restrict__ draws, ChainDiagShape sh,
                                                                       double *__restrict__ out, int *__restrict__ flags,
                                                                       const double *__restrict__ ws) {
  extern __shared__ double cd_lds[];
  const int tid = threadIdx.x, n_threads = blockDim.x;
  const int j = tid % CD_TILE, g = tid / CD_TILE;
  const long long ns = sh.n_series;
  const long long s0 = (long long)blockIdx.x * CD_TILE;
  const int n_valid = (int)(ns - s0 < CD_TILE ? ns - s0 : CD_TILE);
  const int rows = sh.look + sh.chunk;
  double *img = cd_lds;                                   // [rows][CD_PITCH]
  double *mean_tile = cd_lds + (size_t)rows * CD_PITCH;   // [CD_TILE]

  double acc[CD_LG];
#pragma unroll
  for (int k = 0; k < CD_LG; ++k) acc[k] = 0.0;

  for (int c = 0; c < sh.m; ++c) {
    const float *src = draws + ((long long)(c >> 1) * sh.n_draws + (long long)(c & 1) * sh.h) * ns;
    __syncthreads();                                       // the previous half-chain's reads of img and mean_tile are done
    if (tid < CD_TILE) mean_tile[tid] = tid < n_valid ? ws[(long long)c * ns + s0 + tid] : 0.0;
    __syncthreads();
    cd_stage_rows(img, src, ns, s0, n_valid, sh.h, 0, 0, sh.look, mean_tile, tid, n_threads);
    for (int t0 = 0; t0 < sh.h; t0 += sh.chunk) {
      cd_stage_rows(img, src, ns, s0, n_valid, sh.h, t0, sh.look, rows, mean_tile, tid, n_threads);
      __syncthreads();
      const double *pa = img + j;
      const double *pw = img + (size_t)g * CD_LG * CD_PITCH + j;
      for (int tt = 0; tt < sh.chunk; tt += CD_LT) {
        double w[CD_LT + CD_LG - 1];
#pragma unroll
        for (int i = 0; i < CD_LT + CD_LG - 1; ++i) w[i] = pw[i * CD_PITCH];
#pragma unroll
        for (int i = 0; i < CD_LT; ++i) {
          const double a = pa[i * CD_PITCH];
#pragma unroll
          for (int k = 0; k < CD_LG; ++k) acc[k] = fma(a, w[i + k], acc[k]);
        }
        pa += CD_LT * CD_PITCH;
        pw += CD_LT * CD_PITCH;
      }
      __syncthreads();
      // slide: rows [chunk, chunk + look) -> [0, look), through registers (source and destination overlap when look > chunk)
      if (t0 + sh.chunk < sh.h) {
        const int count = sh.look * CD_TILE;
        for (int base = 0; base < count; base += 8 * n_threads) {
          double keep[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int e = base + u * n_threads + tid;
            keep[u] = e < count ? img[(sh.chunk + e / CD_TILE) * CD_PITCH + e % CD_TILE] : 0.0;
          }
          __syncthreads();
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int e = base + u * n_threads + tid;
            if (e < count) img[(e / CD_TILE) * CD_PITCH + e % CD_TILE] = keep[u];
          }
          // a later batch reads rows >= the rows this batch wrote + chunk > them, and writes rows it alone reads afterwards
        }
      }
    }
  }

  // lag sums -> LDS [n_lags][CD_PITCH], then one thread per series finishes
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CD_LG; ++k) img[(size_t)(g * CD_LG + k) * CD_PITCH + j] = acc[k];
  __syncthreads();
  if (tid >= n_valid) return;
  const long long s = s0 + tid;
  const double nan = __builtin_nan("");
  int f = flags[s];
  if (f & CD_FLAG_NONFINITE) {
    out[ns + s] = nan; out[2 * ns + s] = nan; out[3 * ns + s] = nan; out[4 * ns + s] = nan;
    return;
  }
  const double h = (double)sh.h, m = (double)sh.m;
  const double mean_all = out[s];
  double mm = 0.0;
  for (int c = 0; c < sh.m; ++c) mm += ws[(long long)c * ns + s];
  mm /= m;
  double bh = 0.0, ss = ws[(long long)sh.m * ns + s];     // B / h; sum of squares about the mean of all draws
  for (int c = 0; c < sh.m; ++c) {
    const double mc = ws[(long long)c * ns + s];
    bh += (mc - mm) * (mc - mm);
    ss += h * (mc - mean_all) * (mc - mean_all);
  }
  bh /= (m - 1.0);
  const double ss0 = img[tid];                            // sum over half-chains of sum_t d[t]^2
  ss += ss0;
  const double sd = sqrt(ss / ((double)sh.n_chains * (double)sh.n_draws - 1.0));
  out[ns + s] = sd;
  if (f & CD_FLAG_CONSTANT) {
    out[2 * ns + s] = nan; out[3 * ns + s] = nan; out[4 * ns + s] = nan;
    return;
  }
  const double W = ss0 / (m * (h - 1.0));
  const double var_plus = (h - 1.0) / h * W + bh;
  out[2 * ns + s] = sqrt(var_plus / W);
  const double inv_mh = 1.0 / (m * h);
  double sum_p = 0.0, prev = 0.0;
  bool truncated = true;
  for (int k = 0; k + 1 < sh.n_lags; k += 2) {
    const double r0 = k == 0 ? 1.0 : 1.0 - (W - img[(size_t)k * CD_PITCH + tid] * inv_mh) / var_plus;
    const double r1 = 1.0 - (W - img[(size_t)(k + 1) * CD_PITCH + tid] * inv_mh) / var_plus;
    double p = r0 + r1;
    if (!(p >= 0.0)) { truncated = false; break; }
    if (k > 0 && p > prev) p = prev;
    sum_p += p;
    prev = p;
  }
  const double tau = -1.0 + 2.0 * sum_p;
  const double cap = m * h * log10(m * h);
  double ess = m * h / tau;
  if (!(tau > 0.0) || !(ess <= cap)) ess = cap;           // an anti-correlated series: tau -> 0 and below
  out[3 * ns + s] = ess;
  out[4 * ns + s] = sd / sqrt(ess);
  if (truncated) flags[s] = f | CD_FLAG_TRUNCATED;
}
