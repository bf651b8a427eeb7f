"""NumPy restatement of interval='tails' (csrc/causal_kernels.h row_tail_push, csrc/aux_kernels.hip row_tail_quantiles_kernel): the set
update of one tail of one series, draw by draw, and the finisher that turns the two tails into the two interpolated quantiles.  Shared
by tests/test_causal_hmc_tails_host.py and tests/test_gpu_causal_hmc_tails.py; no device is touched."""
import numpy as np


def tail_push(buf, K, d, y, smallest):
    """One draw into one tail, as the kernel does it: buf [K] float32 (in place), d the index of the draw, y its value.  smallest:
    tail 0 (a max-heap: its root is the largest of the K smallest), else tail 1 (a min-heap)."""
    before = (lambda a, b: a > b) if smallest else (lambda a, b: a < b)      # a belongs nearer the root than b
    if d < K:
        i = d
        while i > 0:
            p = (i - 1) >> 1
            if not before(y, buf[p]):
                break
            buf[i] = buf[p]
            i = p
        buf[i] = y
        return
    if not before(buf[0], y):
        return
    i, c = 0, 1
    while c < K:
        vc = buf[c]
        if c + 1 < K and before(buf[c + 1], vc):
            vc, c = buf[c + 1], c + 1
        if not before(vc, y):
            break
        buf[i] = vc
        i = c
        c = 2 * i + 1
    buf[i] = y


def tails_of(series, K, stop=None):
    """(tail 0, tail 1), each [K] float32 in the kernel's slot order, after the draws series[:stop]; slots not yet written are NaN"""
    series = np.asarray(series, np.float32)
    t0, t1 = np.full(K, np.nan, np.float32), np.full(K, np.nan, np.float32)
    for d, y in enumerate(series[:stop]):
        tail_push(t0, K, d, y, True)
        tail_push(t1, K, d, y, False)
    return t0, t1


def quantile_idx(q, m):
    """(i0, i1, t) of bgm_row_mean_quantiles: vi = q (m - 1) in double, i0 = floor(vi) clamped, i1 = min(i0 + 1, m - 1), t = vi - i0"""
    vi = np.float64(q) * np.float64(m - 1)
    i0 = int(min(max(np.floor(vi), 0), m - 1))
    return i0, min(i0 + 1, m - 1), float(vi - np.float64(i0))


def np_lerp(a, b, t):
    """numpy's _lerp as the device applies it: float32 ends, double arithmetic, rounded to float32"""
    a, b = np.float64(np.float32(a)), np.float64(np.float32(b))
    d = b - a
    return np.float32(b - d * (1.0 - t) if t >= 0.5 else a + d * t)


def needed(q_lo, q_hi, m):
    """(smallest values the lower bound reads, largest values the upper bound reads)"""
    return quantile_idx(q_lo, m)[1] + 1, m - quantile_idx(q_hi, m)[0]


def full_quantiles(series, q_lo, q_hi):
    """(lo, hi) float32 from the fully sorted series: the formula of row_mean_quantiles_kernel"""
    s = np.sort(np.asarray(series, np.float32))
    m = len(s)
    out = []
    for q in (q_lo, q_hi):
        i0, i1, t = quantile_idx(q, m)
        out.append(np_lerp(s[i0], s[i1], t))
    return tuple(out)


def tail_quantiles(t0, t1, m, q_lo, q_hi):
    """The finisher: (lo, hi) float32 from tail 0 (the K smallest of the m values, any order) and tail 1 (the K largest).  ValueError
    when K is below what the two bounds read."""
    t0, t1 = np.sort(np.asarray(t0, np.float32)), np.sort(np.asarray(t1, np.float32))
    K = len(t0)
    n_lo, n_hi = needed(q_lo, q_hi, m)
    if len(t1) != K or K > m or K < min(m, max(n_lo, n_hi)):
        raise ValueError("tail_quantiles: K = %d, the bounds read the %d smallest and the %d largest of %d values" % (K, n_lo, n_hi, m))
    i0, i1, t = quantile_idx(q_lo, m)
    lo = np_lerp(t0[i0], t0[i1], t)
    i0, i1, t = quantile_idx(q_hi, m)
    return lo, np_lerp(t1[i0 - (m - K)], t1[i1 - (m - K)], t)
