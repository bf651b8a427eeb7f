// row_tails.h -- one tail of one series of retained values, kept where the values are made (gfx950): the shared text of the kernels that
// return exact quantile bounds without stored draws -- causal_effects<..., TAILS> (causal_kernels.h, causal_hmc_tails_kernels.h) and
// bgm_impute_decode<..., TAILS> (bgm_rowstep_kernels.h, STEP 4).  bgm_row_tail_quantiles (aux_kernels.hip) reads the buffers.
//
// replaces: nothing of the reference; its intervals are np.quantile over stored draws (causalbgm/base.py:640-642, 664-666;
//   bgm/base.py:527-663).
//
// row_tail_push: one tail of one series, a binary heap in global memory with the tail's threshold at slot 0 -- the LARGEST of the K
// smallest values (MAX_HEAP, tail 0) or the smallest of the K largest (tail 1).  Slot s of the series is buf[s * stride].  Draw d < K
// appends y at slot d and sifts it up (d = 0 initialises the series: nothing is read); a later draw enters only when it is strictly
// beyond the threshold, replaces slot 0 and is sifted down.  A draw equal to the threshold stays out, which leaves the multiset
// right: the value is there already.  Nothing but d, K and y decides where the routine reads or writes: every slot index comes from
// d < K or from a loop condition `index < K`, never from a stored value, so NaN / Inf can spoil a series' buffer but not leave it.
// The loops are divergent per lane and hold no wave-level operation.
#pragma once
#include <hip/hip_runtime.h>

template <bool MAX_HEAP>
__device__ __forceinline__ bool row_tail_before(float a, float b) { return MAX_HEAP ? a > b : a < b; }     // a belongs nearer the root than b

template <bool MAX_HEAP>
__device__ __forceinline__ void row_tail_push(float *buf, long long stride, int K, long long d, float y) {
  if (d < (long long)K) {
    int i = (int)d;
    while (i > 0) {                                  // sift up: i < K, strictly decreasing
      const int p = (i - 1) >> 1;
      const float vp = buf[p * stride];
      if (!row_tail_before<MAX_HEAP>(y, vp)) break;
      buf[i * stride] = vp;
      i = p;
    }
    buf[i * stride] = y;
    return;
  }
#ifndef BGM_TAILS_MUTATE_NO_REPLACE                  // (the mutation of DESIGN.md sections 4ac / 4ad: without the replace step the buffers keep the first K draws)
  if (!row_tail_before<MAX_HEAP>(buf[0], y)) return; // the ONE load of a draw that does not enter
  int i = 0;
  for (int c = 1; c < K; c = 2 * i + 1) {            // sift down: c < K, i < c
    float vc = buf[c * stride];
    if (c + 1 < K) {
      const float v2 = buf[(c + 1) * stride];
      if (row_tail_before<MAX_HEAP>(v2, vc)) { vc = v2; ++c; }
    }
    if (!row_tail_before<MAX_HEAP>(vc, y)) break;
    buf[i * stride] = vc;
    i = c;
  }
  buf[i * stride] = y;
#endif
}
