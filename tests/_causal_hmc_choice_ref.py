"""NumPy restatement of what the CHOICE kernels (csrc/causal_hmc_choice_kernels.h) keep per row, on an array of draws
y [n, n_doses, m] (float32, the run's own row_draws): the counts of the per-draw best dose with the lowest index on ties, the counts
of y > threshold, and the float32 sequential shifted sum of the per-draw best value."""
import numpy as np


def best_index(y, maximize=True):
    """[n, m] int: per (row, draw) the LOWEST dose index whose value is the largest (maximize) or the smallest; -1 where every value
    of the draw is NaN.  NaN never wins."""
    y = np.asarray(y, np.float32)
    s = y if maximize else -y                                            # exact
    s = np.where(np.isnan(s), -np.inf, s)
    idx = np.argmax(s, axis=1)                                           # numpy: the first occurrence of the maximum
    return np.where(np.isnan(y).all(axis=1), -1, idx)


def best_count(y, maximize=True):
    """[n, n_doses] int64: the draws at which dose k was the row's best"""
    n, nd, _ = np.shape(y)
    idx = best_index(y, maximize)
    out = np.zeros((n, nd), np.int64)
    for k in range(nd):
        out[:, k] = (idx == k).sum(axis=1)
    return out


def above_count(y, threshold):
    """[n, n_doses] int64: the draws with y > float32(threshold)"""
    return (np.asarray(y, np.float32) > np.float32(threshold)).sum(axis=-1).astype(np.int64)


def best_value(y, maximize=True):
    """[n, m] float32: the best value of every (row, draw) -- the value itself, not sign * value; NaN only where the draw is all NaN"""
    y = np.asarray(y, np.float32)
    return np.fmax.reduce(y, axis=1) if maximize else np.fmin.reduce(y, axis=1)


def best_moments(y, maximize=True):
    """(ref [n], s1 [n]) float32, as the kernel forms them: ref = the best of draw 0, then for d = 1 .. m - 1 in order
    s1 = fl(s1 + fl(best_d - ref)) -- one float32 subtraction and one float32 addition per draw."""
    b = best_value(y, maximize)
    ref = b[:, 0].copy()
    s1 = np.zeros_like(ref)
    for d in range(1, b.shape[1]):
        s1 = (s1 + (b[:, d] - ref).astype(np.float32)).astype(np.float32)
    return ref, s1


def shifted_mean_bound(series):
    """A bound on |float64(ref) + float64(s1) / m - the float64 mean| of float32 series [..., m] summed as the kernels sum them
    (ref = value 0, s1 += value - ref): the m - 1 subtractions and the m - 1 additions each round once, relative 2^-24, on
    magnitudes of at most R = max |value - ref| and, for the running sum, (m - 1) R: ((m - 1) + (m - 1)^2) R 2^-24 / m."""
    b = np.asarray(series, np.float64)
    m = b.shape[-1]
    r = np.abs(b - b[..., :1]).max(axis=-1)
    return ((m - 1) + (m - 1) ** 2) * r * 2.0 ** -24 / m


def best_mean_bound(y, maximize=True):
    """shifted_mean_bound of the per-draw best: [n]"""
    return shifted_mean_bound(best_value(y, maximize))
