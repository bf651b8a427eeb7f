// sdr_kernels.h -- first and second moments of a covariate panel in one read, in float64 on the matrix pipe.
//
// Feeds bayesgm_amd.latent_dims (estimate_latent_dims / get_SDR_dim: SIR + PCA of the reference's utils/helpers.py:140-222).
// With w_i = v_i - c (c an optional per-column shift), one pass over the N rows of V produces
//     extra row 0        sum_i w_i                                   (column sums)
//     extra row 1 + k    sum_{i : label0_i = k} w_i                  (slice sums of labeling 0, k < s0)
//     extra row 1+s0+k   sum_{i : label1_i = k} w_i                  (slice sums of labeling 1, k < s1)
//     Gram               sum_i w_i w_i^T                             (upper triangle of 16x16 tiles, mirrored on output)
// Every product is a v_mfma_f64_16x16x4_f64 with the rows of V as its K dimension: the A fragment of a Gram tile and the
// B fragment of every tile are reads of the same staged rows (lane l: row 4s + (l >> 4), column 16 * block + (l & 15)); the
// A fragment of an extra tile is the indicator (label == e) built in registers.  C/D of the f64 form: col = lane & 15,
// row = (lane >> 4) + 4 * reg.
//
// Work is split into tasks: one A block (a Gram row block, or a block of 16 extra rows) against a run of up to SDR_TPW
// consecutive column blocks (Gram: blocks [a, pb) -- the upper triangle -- in runs of SDR_TPW; extra rows: blocks [0, pb)).
// A wave owns one task: its A fragment is read (or built) once per K step and reused by every tile of the run, whose B fragments
// sit at compile-time offsets of one LDS address.  blockIdx.y takes SDR_WAVES consecutive tasks, blockIdx.x a contiguous range
// of rows, staged chunk by chunk into LDS as shifted float64.  Each workgroup writes its partial tiles to the workspace;
// sdr_reduce_kernel sums them in workgroup order (no atomics: repeated calls are bit-identical).
#pragma once
#include <hip/hip_runtime.h>

typedef double sdr_f64x4 __attribute__((ext_vector_type(4)));

constexpr int SDR_WAVES = 8;
constexpr int SDR_TPW = 16;                        // accumulator tiles per wave: 16 x 4 doubles = 128 VGPRs
constexpr int SDR_ROWS_BYTES = 136 * 1024;         // LDS budget of the staged rows: KR rows x (P + 1) doubles (KR >= 8 at p = 2048)
constexpr int SDR_MAX_KR = 64;                     // rows per staged chunk (multiple of 8)

struct SdrShape {
  long long n, ldv, rows_per_wg;
  int p, pb;        // columns, 16-column blocks
  int s0, s1;       // slices of labeling 0 / 1
  int eb;           // 16-row blocks of the 1 + s0 + s1 extra rows
  int n_tasks;      // Gram tasks + extra tasks
  int kr;           // rows per staged chunk
};

struct SdrTask {
  int a;            // A block (Gram row block, or extra-row block)
  int b0, nb;       // column blocks b0 .. b0 + nb - 1
  bool extra;
};

__host__ __device__ inline int sdr_n_tasks(int pb, int eb) {
  int n = 0;
  for (int a = 0; a < pb; ++a) n += (pb - a + SDR_TPW - 1) / SDR_TPW;
  return n + eb * ((pb + SDR_TPW - 1) / SDR_TPW);
}

__device__ inline SdrTask sdr_task(const SdrShape &s, int t) {
  SdrTask k;
  for (int a = 0; a < s.pb; ++a) {
    const int runs = (s.pb - a + SDR_TPW - 1) / SDR_TPW;
    if (t < runs) {
      k.a = a; k.b0 = a + SDR_TPW * t; k.nb = min(SDR_TPW, s.pb - k.b0); k.extra = false;
      return k;
    }
    t -= runs;
  }
  const int runs = (s.pb + SDR_TPW - 1) / SDR_TPW;
  k.a = t / runs; k.b0 = SDR_TPW * (t % runs); k.nb = min(SDR_TPW, s.pb - k.b0); k.extra = true;
  return k;
}

template <typename T>
__global__ __launch_bounds__(64 * SDR_WAVES) void sdr_moments_kernel(const T *__restrict__ v, const double *__restrict__ shift,
                                                                    const int *__restrict__ lab0, const int *__restrict__ lab1,
                                                                    SdrShape s, double *__restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double sdr_lds[];
  const int P = 16 * s.pb, LD = P + 1, KR = s.kr;
  double *vs = sdr_lds;                          // [KR][LD] staged rows, shifted, zero-padded
  double *sh = vs + KR * LD;                     // [P] shift
  int *labs = reinterpret_cast<int *>(sh + P);   // [2][KR] labels of the staged rows (-1 past the end)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int c = tid; c < P; c += 64 * SDR_WAVES) sh[c] = (shift != nullptr && c < s.p) ? shift[c] : 0.0;

  const int task = blockIdx.y * SDR_WAVES + wave;
  const bool active = task < s.n_tasks;
  const SdrTask k = sdr_task(s, active ? task : 0);
  sdr_f64x4 acc[SDR_TPW];
#pragma unroll
  for (int j = 0; j < SDR_TPW; ++j) acc[j] = sdr_f64x4{0.0, 0.0, 0.0, 0.0};

  const long long r_begin = (long long)blockIdx.x * s.rows_per_wg;
  const long long r_end = min(s.n, r_begin + s.rows_per_wg);
  const int col = lane & 15, krow = lane >> 4;
  const int a_col = 16 * k.a + col, b_col = 16 * k.b0 + col;
  for (long long r0 = r_begin; r0 < r_end; r0 += KR) {
    __syncthreads();                             // sh[] written / every wave done with the previous chunk
    // stage: wave w writes rows w, w + 8, ...; lanes run along the columns (coalesced reads of each row)
    for (int r = wave; r < KR; r += SDR_WAVES) {
      const long long row = r0 + r;
      const bool in = row < r_end;
      const T *src = v + (in ? row : 0) * s.ldv;
#pragma unroll 4
      for (int c = lane; c < P; c += 64) vs[r * LD + c] = (in && c < s.p) ? (double)src[c] - sh[c] : 0.0;
      if (lane == 0) {
        labs[r] = (in && lab0 != nullptr) ? lab0[row] : -1;
        labs[KR + r] = (in && lab1 != nullptr) ? lab1[row] : -1;
      }
    }
    __syncthreads();
    if (!active) continue;
    for (int k4 = 0; k4 < KR; k4 += 4) {
      const double *vrow = vs + (k4 + krow) * LD;
      double av;
      if (k.extra) {
        const int l0 = labs[k4 + krow], l1 = labs[KR + k4 + krow];
        av = a_col == 0 ? 1.0 : (a_col <= s.s0 ? (l0 == a_col - 1 ? 1.0 : 0.0) : (l1 == a_col - 1 - s.s0 ? 1.0 : 0.0));
      } else {
        av = vrow[a_col];
      }
      const double *brow = vrow + b_col;
#pragma unroll
      for (int j = 0; j < SDR_TPW; ++j)
        if (j < k.nb) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[16 * j], acc[j], 0, 0, 0);
    }
  }

  // partial tiles: ws[((blockIdx.x * n_tasks + task) * SDR_TPW + j) * 256 + 4 * lane + reg]
  if (!active) return;
#pragma unroll
  for (int j = 0; j < SDR_TPW; ++j)
    if (j < k.nb)
      *reinterpret_cast<sdr_f64x4 *>(ws + (((long long)blockIdx.x * s.n_tasks + task) * SDR_TPW + j) * 256 + 4 * lane) = acc[j];
}

// out = [ extra rows (1 + s0 + s1) x p | Gram p x p ], each entry the sum of the n_wg partials in workgroup order.
__global__ __launch_bounds__(256) void sdr_reduce_kernel(const double *__restrict__ ws, SdrShape s, int n_wg, double *__restrict__ out) {
  const long long total = (long long)s.n_tasks * SDR_TPW * 256;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const int slot = (int)(q >> 8), lane = (int)((q >> 2) & 63), reg = (int)(q & 3);
  const SdrTask k = sdr_task(s, slot / SDR_TPW);
  const int jt = slot % SDR_TPW;
  if (jt >= k.nb) return;                          // a slot past the task's run: never written
  const int row = (lane >> 4) + 4 * reg, col = lane & 15;
  const int j = 16 * (k.b0 + jt) + col;
  if (j >= s.p) return;
  const int i = 16 * k.a + row;
  if (k.extra ? i >= 1 + s.s0 + s.s1 : (i >= s.p || i > j)) return;   // padding; the diagonal tile's lower half mirrors its upper half
  double sum = 0.0;
  for (int x = 0; x < n_wg; ++x) sum += ws[(long long)x * total + q];
  if (k.extra) {
    out[(long long)i * s.p + j] = sum;
  } else {
    double *gram = out + (long long)(1 + s.s0 + s.s1) * s.p;
    gram[(long long)i * s.p + j] = sum;
    gram[(long long)j * s.p + i] = sum;
  }
}
