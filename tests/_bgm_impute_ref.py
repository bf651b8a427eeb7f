"""What the tests of the imputation inside the BGM sampler (bgm_bgm_hmc_run_rows_impute) share: the cases, the missing pattern, the
float32 NumPy restatement of the kernel's sequential shifted sums, and the two error bounds with their derivation.

The kernel keeps per missing cell, over the k retained values x_0 .. x_{k-1} (float32):
    ref = x_0,   s1 = sum_{d >= 1} fl(x_d - ref),   s2 = sum_{d >= 1} fma(e_d, e_d, s2),  e_d = fl(x_d - ref)
and the caller forms  mean = ref + s1 / k,  var = (s2 - s1^2 / k) / (k - 1).

Bounds, with u = 2^-24, gamma_k = k u / (1 - k u), d = x - ref in exact arithmetic on the float64 reference values, and every float32
value within 2e-4 of its reference (the bar of test_predictive_draws_match_oracle_on_same_latents):
  mean:  the values' own error moves the mean by at most 2e-4; a sequential float32 sum of k terms has relative error gamma_k on
         sum |d| (each subtraction adds one more u, inside gamma_k's slack for k >= 2 terms), so  |mean - mean_ref| <= 2e-4 + gamma_k mean|d|.
  var:   with delta = 2e-4 sqrt(k / (k - 1)) the perturbed sample sd differs from sd_ref by at most delta (the centred perturbation has
         norm <= 2e-4 sqrt(k), divided by sqrt(k - 1)), so the variance moves by at most 2 sd_ref delta + delta^2; the rounding of the
         sum of squares is gamma_k sum d^2, that of s1^2 / k at most 2 gamma_k (sum |d|)^2 / k <= 2 gamma_k sum d^2 by Cauchy-Schwarz:
         |var - var_ref| <= 3 gamma_k sum d^2 / (k - 1) + 2 sd_ref delta + delta^2.
"""
import numpy as np

U = 2.0 ** -24
VALUE_BAR = 2e-4

# the fp32 rows of FROZEN in test_gpu_bgm_row_step.py and the streamed 3-layer trunk: all six compiled variants
CASES = [dict(p=20, n=50, nh=5), dict(p=100, n=50, nh=5), dict(p=61, n=50, nh=5), dict(p=500, n=50, nh=5), dict(p=20, n=17, nh=3, q=3),
         dict(p=100, n=1, nh=3), dict(p=61, n=33, nh=3)]
BURN, KEEP, LEAP = 4, 6, 3
LONG = dict(p=20, n=17, nh=3, q=3)      # the case that is also run at k = 400
KEEP_LONG = 400
MISS = 0.3


def case_id(c):
    return "p%d-n%d-nh%d" % (c["p"], c["n"], c["nh"])


def gamma(k):
    return k * U / (1.0 - k * U)


def slots_of(miss):
    """(slot int32 [n, p], k_slots): slot k of a row is its k-th missing cell, -1 at observed cells (BGM.predict's map)."""
    slot = (np.cumsum(miss, axis=1) - 1).astype(np.int32)
    slot[~miss] = -1
    return slot, int(max(1, miss.sum(axis=1).max()))


def moments_f32(x):
    """(ref, s1, s2) float32 of the values x [k, ...] float32, summed in the kernel's order."""
    x = np.asarray(x, np.float32)
    ref = x[0].copy()
    s1 = np.zeros_like(ref)
    s2 = np.zeros_like(ref)
    for d in range(1, x.shape[0]):
        e = (x[d] - ref).astype(np.float32)
        s1 = (s1 + e).astype(np.float32)
        s2 = (e.astype(np.float64) * e.astype(np.float64) + s2.astype(np.float64)).astype(np.float32)      # (one rounding: the fma)
    return ref, s1, s2


def mean_var(ref, s1, s2, k):
    """mean and variance (k - 1 in the denominator) from the three planes, in float64."""
    ref, s1, s2 = (np.asarray(a, np.float64) for a in (ref, s1, s2))
    return ref + s1 / k, (s2 - s1 * s1 / k) / (k - 1)


def reference(x64):
    """(mean_ref, var_ref, mean_bound, var_bound) from the float64 reference values x64 [k, ...]; mean_bound without the 2e-4 of the
    values' own error is mean_bound - VALUE_BAR."""
    x64 = np.asarray(x64, np.float64)
    k = x64.shape[0]
    d = x64 - x64[0]
    mean_ref, var_ref = x64.mean(axis=0), x64.var(axis=0, ddof=1)
    delta = VALUE_BAR * np.sqrt(k / (k - 1.0))
    mean_bound = VALUE_BAR + gamma(k) * np.abs(d).mean(axis=0)
    var_bound = 3.0 * gamma(k) * (d * d).sum(axis=0) / (k - 1) + 2.0 * np.sqrt(var_ref) * delta + delta * delta
    return mean_ref, var_ref, mean_bound, var_bound
