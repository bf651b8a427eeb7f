"""NumPy restatement of the CausalBGM log posterior and HMC sampler for PARTIALLY OBSERVED rows (TEST INFRASTRUCTURE): NaN in y, or
in x and y, marks what a row does not observe, and the row's target is the log posterior of oracle.causal with the terms of the
unobserved variables left out -- p(z | x, v) without the outcome term of f, p(z | v) without the treatment term of h as well.
The terms are those of tests/_causal_hmc_ref.py (whose _gauss is imported); the sampler IS that module's hmc_sampler, run with this
module's log posterior in place of its own.  Everything takes the dtype of z.  Nothing is added to oracle/ or to that module."""
from unittest import mock

import numpy as np

import _causal_hmc_mass_ref as MREF
import _causal_hmc_ref as REF
from oracle import causal as OC
from oracle.nets import mlp_backward, mlp_forward_cache, sigmoid


def patterns(x, y):
    """(has_x, has_y) bool [n]"""
    return ~np.isnan(np.asarray(x).reshape(-1)), ~np.isnan(np.asarray(y).reshape(-1))


def log_posterior_terms(m, x, y, v, z):
    """The four terms apart, in the dtype of z: dict(v, x, y, prior) of (nll [n], dnll/dz [n, q]).  The x term is exactly zero in
    value and gradient for a row whose x is NaN, the y term for a row whose y is NaN (a select on the nll and on the head's
    gradient, so the backward pass of the net carries zeros); a missing x enters f's input as 0, where f's term is masked anyway."""
    dt = z.dtype
    t = dt.type
    m = OC.cast_model(m, dt)
    n = len(z)
    x, y, v = (np.asarray(a, dt).reshape(n, -1) for a in (x, y, v))
    has_x, has_y = patterns(x, y)
    assert not np.any(has_y & ~has_x), "a row with y observed and x not has no target"
    x0 = np.where(has_x[:, None], x, t(0))
    p = m["v_dim"]
    z0d, z1d, z2d, _ = m["z_dims"]
    z0, z1, z2 = OC.split_z(m, z)
    out, cache = mlp_forward_cache(m["g"], z)
    d = v - out[:, :p]
    nll_v, s2, ds_raw = REF._gauss((d ** 2).sum(axis=1), out[:, -1], p, m.get("sigma_v"), t)
    dout = np.zeros_like(out)
    dout[:, :p] = -d / s2[:, None]
    dout[:, -1] = ds_raw
    dz_v = mlp_backward(m["g"], cache, dout)[1].copy()
    # h: treatment
    out, cache = mlp_forward_cache(m["h"], np.concatenate([z0, z2], axis=-1))
    dout = np.zeros_like(out)
    with np.errstate(invalid="ignore"):
        if m["binary_treatment"]:
            l = out[:, 0]
            nll_x = np.maximum(l, 0) - l * x0[:, 0] + np.log1p(np.exp(-np.abs(l)))
            dout[:, 0] = sigmoid(l) - x0[:, 0]
        else:
            d = x0[:, 0] - out[:, 0]
            nll_x, s2, ds_raw = REF._gauss(d ** 2, out[:, -1], 1, m.get("sigma_x"), t)
            dout[:, 0] = -d / s2
            dout[:, -1] = ds_raw
    nll_x = np.where(has_x, nll_x, t(0))
    dout = np.where(has_x[:, None], dout, t(0))
    dinp = mlp_backward(m["h"], cache, dout)[1]
    dz_x = np.zeros_like(z)
    dz_x[:, :z0d] += dinp[:, :z0d]
    dz_x[:, z0d + z1d:z0d + z1d + z2d] += dinp[:, z0d:]
    # f: outcome
    out, cache = mlp_forward_cache(m["f"], np.concatenate([z0, z1, x0], axis=-1))
    y0 = np.where(has_y[:, None], y, t(0))
    d = y0[:, 0] - out[:, 0]
    nll_y, s2, ds_raw = REF._gauss(d ** 2, out[:, -1], 1, m.get("sigma_y"), t)
    dout = np.zeros_like(out)
    dout[:, 0] = -d / s2
    dout[:, -1] = ds_raw
    nll_y = np.where(has_y, nll_y, t(0))
    dout = np.where(has_y[:, None], dout, t(0))
    dinp = mlp_backward(m["f"], cache, dout)[1]
    dz_y = np.zeros_like(z)
    dz_y[:, :z0d + z1d] += dinp[:, :z0d + z1d]
    return dict(v=(nll_v, dz_v), x=(nll_x, dz_x), y=(nll_y, dz_y), prior=((z ** 2).sum(axis=1) / 2, z))


def log_posterior_and_grad(m, x, y, v, z):
    """(log p [n], gradient [n, q]) of the partially observed rows, summed in the order of tests/_causal_hmc_ref.py"""
    T = log_posterior_terms(m, x, y, v, z)
    dz = T["v"][1].copy()
    dz += T["x"][1]
    dz += T["y"][1]
    logp = -(T["v"][0] + T["x"][0] + T["y"][0] + T["prior"][0])
    grad = -(dz + z)
    assert logp.dtype == z.dtype and grad.dtype == z.dtype
    return logp, grad


def hmc_sampler(m, data, burn_in, n_keep, step0, n_leapfrog, seed, up, dn, row0=0):
    """tests/_causal_hmc_ref.py::hmc_sampler (transition, accept rule, step table) on the partial log posterior"""
    with mock.patch.object(REF, "log_posterior_and_grad", log_posterior_and_grad):
        return REF.hmc_sampler(m, data, burn_in, n_keep, step0, n_leapfrog, seed, up, dn, row0)


def hmc_mass_sampler(m, data, burn_in, n_keep, step0, n_leapfrog, seed, up, dn, row0=0, scale=None, windows=None):
    """tests/_causal_hmc_mass_ref.py::hmc_mass_sampler (the diagonal metric estimated in windows) on the partial log posterior"""
    with mock.patch.object(MREF, "log_posterior_and_grad", log_posterior_and_grad):
        return MREF.hmc_mass_sampler(m, data, burn_in, n_keep, step0, n_leapfrog, seed, up, dn, row0, scale, windows)


def mixed_panel(x, y, seed=0):
    """(x, y) [n, 1] float32 with the three patterns -- all observed, y missing, x and y missing -- scattered over the rows, so that
    every 16-row tile of more than two rows holds all of them (row i: pattern (i + shift) % 3 with a shift per tile)."""
    x, y = np.array(x, np.float32).reshape(-1, 1), np.array(y, np.float32).reshape(-1, 1)
    rs = np.random.RandomState(seed)
    n = len(x)
    shift = np.repeat(rs.randint(0, 3, (n + 15) // 16), 16)[:n]
    pat = (np.arange(n) + shift) % 3
    y[pat >= 1] = np.nan
    x[pat == 2] = np.nan
    return x, y
