"""What the tests of the per-row dose contrasts (bgm_causal_hmc_run_row_contrasts) share: the two error bounds of the shifted
float32 moments against float64 on the same float32 series, and a synthetic contrast series.

The kernel keeps per (row, dose), over the m retained contrasts c_0 .. c_{m-1} (float32), the sums of tests/_bgm_impute_ref.py:
    ref = c_0,   s1 = sum_{d >= 1} fl(c_d - ref),   s2 = sum_{d >= 1} fma(e_d, e_d, s2),  e_d = fl(c_d - ref)
and the caller forms mean = ref + s1 / m, var = (s2 - s1^2 / m) / (m - 1) in float64 (causal_hmc.row_moments_finalize).

The bounds are those derived in tests/_bgm_impute_ref.py with d = c - ref in exact arithmetic on the series itself.  The reference
here is float64 on the run's OWN float32 values, so the values carry no error of their own: the value bar of that module is 0, hence
delta = 0, and what remains is the rounding of the sums alone:
    |mean - mean_ref| <= gamma_m mean|d|
    |var  - var_ref|  <= 3 gamma_m sum d^2 / (m - 1) + 2 sd_ref delta + delta^2,   delta = 0
with gamma_m = m u / (1 - m u), u = 2^-24.  The sd is compared through its square."""
import numpy as np

import _bgm_impute_ref as IR

DELTA = 0.0      # the values are the same on both sides


def bounds(c):
    """(mean_ref, var_ref, mean_bound, var_bound) of the float32 series c [..., m], in float64"""
    c = np.asarray(c, np.float32).astype(np.float64)
    m = c.shape[-1]
    d = c - c[..., :1]
    var_ref = c.var(axis=-1, ddof=1) if m > 1 else np.zeros(c.shape[:-1])
    mean_bound = IR.gamma(m) * np.abs(d).mean(axis=-1)
    var_bound = 3.0 * IR.gamma(m) * (d * d).sum(axis=-1) / max(m - 1, 1) + 2.0 * np.sqrt(var_ref) * DELTA + DELTA * DELTA
    return c.mean(axis=-1), var_ref, mean_bound, var_bound


def worst_ratios(mean, sd, c):
    """(worst |mean - ref| / bound, worst |sd^2 - var_ref| / bound) over the series with a non-zero bound, and whether every series
    -- those with bound 0, the constant ones, included -- is inside both bounds"""
    mean_ref, var_ref, mean_bound, var_bound = bounds(c)
    e_mean, e_var = np.abs(np.asarray(mean, np.float64) - mean_ref), np.abs(np.asarray(sd, np.float64) ** 2 - var_ref)
    inside = bool((e_mean <= mean_bound).all() and (e_var <= var_bound).all())
    r_mean = float((e_mean[mean_bound > 0] / mean_bound[mean_bound > 0]).max()) if (mean_bound > 0).any() else 0.0
    r_var = float((e_var[var_bound > 0] / var_bound[var_bound > 0]).max()) if (var_bound > 0).any() else 0.0
    return r_mean, r_var, inside


def synthetic_contrasts(rs, n, n_doses, m, ties=False):
    """float32 contrasts [n, n_doses, m] of correlated dose series, formed as the kernel forms them: one float32 subtraction of the
    rounded values, column 0 against itself.  ties: a chain that rejects most proposals holds each value for a run of draws."""
    level = 2.0 + rs.randn(n, 1, m)                                       # what the doses of a row share on a draw
    slope = 0.5 + 0.2 * rs.randn(n, 1, 1)
    y = level + slope * np.linspace(0.0, 3.0, n_doses)[None, :, None] + 0.05 * rs.randn(n, n_doses, m)
    if ties:
        y = np.repeat(y[..., ::7], 7, axis=-1)[..., :m]
    y = y.astype(np.float32)
    return (y - y[:, :1]).astype(np.float32)
