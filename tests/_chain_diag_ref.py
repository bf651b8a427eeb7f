"""Float64 NumPy restatement of bgm_chain_diagnostics (include/bgm_hip.h): split R-hat and effective sample size per series, the
Stan / ArviZ "mean" forms without rank normalisation.  Test helper: plain loops over chains, lags and Geyer pairs, vectorised
over the series only."""
import numpy as np

FLAG_CONSTANT, FLAG_TRUNCATED, FLAG_NONFINITE = 1, 2, 4


def chain_diag_ref(draws, max_lag=256):
    """draws: (n_chains, n_draws, n_series) or (n_draws, n_series).  Returns dict(mean, sd, rhat, ess, mcse, moves: float64
    [n_series]; flags: int32 [n_series]; stop_lag: the lag 2j of the first negative pair, -1 when the sum was truncated)."""
    x = np.asarray(draws)
    if x.ndim == 2:
        x = x[None]
    x = x.astype(np.float64)
    n_chains, n_draws, n_series = x.shape
    assert n_draws >= 8 and 1 <= n_chains <= 8 and 1 <= max_lag <= 1024
    max_lag = min(max_lag, n_draws // 2 - 1)
    h = n_draws // 2
    m = 2 * n_chains
    halves = [x[c, half * h:(half + 1) * h] for c in range(n_chains) for half in range(2)]          # m arrays [h, n_series]

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        finite = np.isfinite(x).all(axis=(0, 1))
        pooled = x.reshape(n_chains * n_draws, n_series)
        mean = pooled.mean(axis=0)
        sd = np.sqrt(((pooled - mean) ** 2).sum(axis=0) / (n_chains * n_draws - 1))
        moves = (x[:, 1:] != x[:, :-1]).sum(axis=(0, 1)).astype(np.float64)
        constant = finite & (pooled.max(axis=0) == pooled.min(axis=0))

        means = np.stack([a.mean(axis=0) for a in halves])                                            # [m, n_series]
        cent = [a - mu for a, mu in zip(halves, means)]
        W = np.mean([(d * d).sum(axis=0) / (h - 1) for d in cent], axis=0)
        B_over_h = ((means - means.mean(axis=0)) ** 2).sum(axis=0) / (m - 1)
        var_plus = (h - 1) / h * W + B_over_h
        rhat = np.sqrt(var_plus / W)

        def rho(k):
            if k == 0:
                return np.ones(n_series)
            acov = np.mean([(d[:h - k] * d[k:]).sum(axis=0) / h for d in cent], axis=0)
            return 1.0 - (W - acov) / var_plus

        sum_p = np.zeros(n_series)
        prev = np.zeros(n_series)
        running = np.ones(n_series, dtype=bool)
        stop_lag = np.full(n_series, -1, dtype=np.int64)
        j = 0
        while 2 * j + 1 <= max_lag and running.any():
            p = rho(2 * j) + rho(2 * j + 1)
            stop = running & ~(p >= 0)
            stop_lag[stop] = 2 * j
            running &= ~stop
            if j > 0:
                p = np.minimum(p, prev)
            sum_p[running] += p[running]
            prev = p
            j += 1
        tau = -1.0 + 2.0 * sum_p
        cap = m * h * np.log10(m * h)
        ess = m * h / tau
        ess = np.where((tau > 0) & (ess <= cap), ess, cap)
        mcse = sd / np.sqrt(ess)

    flags = np.zeros(n_series, dtype=np.int32)
    flags[running] |= FLAG_TRUNCATED
    flags[constant] = FLAG_CONSTANT
    flags[~finite] = FLAG_NONFINITE
    nan = np.nan
    for a in (rhat, ess, mcse):
        a[constant | ~finite] = nan
    for a in (mean, sd, moves):
        a[~finite] = nan
    stop_lag[constant | ~finite] = -1
    return dict(mean=mean, sd=sd, rhat=rhat, ess=ess, mcse=mcse, moves=moves, flags=flags, stop_lag=stop_lag)


def ar1(rs, n_draws, n_series, phi, loc=0.0, n_chains=None):
    """Stationary AR(1) series with unit marginal variance around `loc`, float32: (n_draws, n_series) or, with n_chains,
    (n_chains, n_draws, n_series)."""
    shape = (n_draws, n_series) if n_chains is None else (n_chains, n_draws, n_series)
    e = rs.standard_normal(shape)
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (n_series,))
    out = np.empty(shape)
    t_axis = len(shape) - 2
    e = np.moveaxis(e, t_axis, 0)
    o = np.moveaxis(out, t_axis, 0)
    o[0] = e[0]
    s = np.sqrt(1.0 - phi ** 2)
    for t in range(1, n_draws):
        o[t] = phi * o[t - 1] + s * e[t]
    return (out + loc).astype(np.float32)
