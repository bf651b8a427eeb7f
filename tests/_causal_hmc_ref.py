"""NumPy restatement of the HMC latent sampler of CausalBGM (TEST INFRASTRUCTURE): the log posterior of oracle.causal with its gradient
(built from oracle.nets.mlp_forward_cache / mlp_backward, the way oracle/fit.py builds z_loss_and_grad), the leapfrog transition of
oracle/bgm.py::hmc_transition with a step per row, and the sampler with the per-chain step adaptation of bayesgm_amd/row_adapt.py.
Everything takes the dtype of z: float64 for parity bars, float32 for chain parity.  Nothing is added to oracle/."""
import numpy as np

from oracle import causal as OC
from oracle import rng as R
from oracle.nets import mlp_backward, mlp_forward_cache, sigmoid, softplus

from bayesgm_amd.row_adapt import S_MAX, S_MIN


def _gauss(rsq, s_raw, dim, fixed_sd, t):
    """nll = rsq / (2 s2) + dim log(s2) / 2 -> (nll, s2, dnll/ds_raw)"""
    if fixed_sd is not None:
        s2 = t(fixed_sd) ** 2 + 0 * s_raw
        ds_raw = np.zeros_like(s_raw)
    else:
        s2 = softplus(s_raw) + t(OC.EPS)
        ds_raw = (-rsq / (2 * s2 * s2) + t(dim) / (2 * s2)) * sigmoid(s_raw)
    return rsq / (2 * s2) + t(dim) * np.log(s2) / 2, s2, ds_raw


def log_posterior_and_grad(m, x, y, v, z):
    """(log p(z | x, y, v) [n], its gradient with respect to z [n, q]) in the dtype of z; the value is oracle.causal.log_posterior."""
    dt = z.dtype
    t = dt.type
    m = OC.cast_model(m, dt)
    x, y, v = (np.asarray(a, dt).reshape(len(z), -1) for a in (x, y, v))
    p = m["v_dim"]
    z0d, z1d, z2d, _ = m["z_dims"]
    z0, z1, z2 = OC.split_z(m, z)
    # g: covariates
    out, cache = mlp_forward_cache(m["g"], z)
    d = v - out[:, :p]
    nll_v, s2, ds_raw = _gauss((d ** 2).sum(axis=1), out[:, -1], p, m.get("sigma_v"), t)
    dout = np.zeros_like(out)
    dout[:, :p] = -d / s2[:, None]
    dout[:, -1] = ds_raw
    dz = mlp_backward(m["g"], cache, dout)[1].copy()
    # h: treatment
    out, cache = mlp_forward_cache(m["h"], np.concatenate([z0, z2], axis=-1))
    dout = np.zeros_like(out)
    if m["binary_treatment"]:
        l = out[:, 0]
        nll_x = np.maximum(l, 0) - l * x[:, 0] + np.log1p(np.exp(-np.abs(l)))
        dout[:, 0] = sigmoid(l) - x[:, 0]
    else:
        d = x[:, 0] - out[:, 0]
        nll_x, s2, ds_raw = _gauss(d ** 2, out[:, -1], 1, m.get("sigma_x"), t)
        dout[:, 0] = -d / s2
        dout[:, -1] = ds_raw
    dinp = mlp_backward(m["h"], cache, dout)[1]
    dz[:, :z0d] += dinp[:, :z0d]
    dz[:, z0d + z1d:z0d + z1d + z2d] += dinp[:, z0d:]
    # f: outcome (x is an input, not differentiated)
    out, cache = mlp_forward_cache(m["f"], np.concatenate([z0, z1, x], axis=-1))
    d = y[:, 0] - out[:, 0]
    nll_y, s2, ds_raw = _gauss(d ** 2, out[:, -1], 1, m.get("sigma_y"), t)
    dout = np.zeros_like(out)
    dout[:, 0] = -d / s2
    dout[:, -1] = ds_raw
    dinp = mlp_backward(m["f"], cache, dout)[1]
    dz[:, :z0d + z1d] += dinp[:, :z0d + z1d]
    logp = -(nll_v + nll_x + nll_y + (z ** 2).sum(axis=1) / 2)
    grad = -(dz + z)
    assert logp.dtype == dt and grad.dtype == dt
    return logp, grad


def leapfrog(m, x, y, v, z, mom, gr, step, n_leapfrog):
    """half kick, n_leapfrog position steps with full kicks between them, half kick -> (z, mom, logp, grad) at the end point"""
    e = np.asarray(step).astype(z.dtype)[:, None]
    zc, pc = z.copy(), mom + e / 2 * gr
    lpc, grc = None, gr
    for l in range(n_leapfrog):
        zc = zc + e * pc
        lpc, grc = log_posterior_and_grad(m, x, y, v, zc)
        pc = pc + (e if l < n_leapfrog - 1 else e / 2) * grc
    return zc, pc, lpc, grc


def hmc_transition(m, x, y, v, z, lp, gr, step, n_leapfrog, it, seed, row0=0):
    """oracle/bgm.py::hmc_transition with a step per row -> (z, lp, gr, log_accept_ratio, accepted)."""
    n, q = z.shape
    rows = np.arange(row0, row0 + n)
    mom = R.normals(rows, it, q, R.TAG_MOM, seed).astype(z.dtype)
    u = R.uniforms(rows, it, R.TAG_HACC, seed).astype(z.dtype)
    h0 = -lp + (mom ** 2).sum(axis=1) / 2
    zc, pc, lpc, grc = leapfrog(m, x, y, v, z, mom, gr, step, n_leapfrog)
    h1 = -lpc + (pc ** 2).sum(axis=1) / 2
    with np.errstate(invalid="ignore"):
        log_ratio = -(h1 - h0)
    log_ratio = np.where(np.isfinite(log_ratio), log_ratio, -np.inf)
    acc = np.log(u) < log_ratio
    return np.where(acc[:, None], zc, z), np.where(acc, lpc, lp), np.where(acc[:, None], grc, gr), log_ratio, acc


def hmc_sampler(m, data, burn_in, n_keep, step0, n_leapfrog, seed, up, dn, row0=0):
    """-> dict(draws [n_keep, n, q], state, logp, grad, acc [burn_in + n_keep, n] bool, step [n] float32).  up / dn: float32 factor tables
    (None: fixed step); after the decision of iteration it < len(up) a row's step is multiplied in float32 by up[it] if it moved, by
    dn[it] if not, and clamped to [S_MIN, S_MAX]."""
    x, y, v = data
    n, q = len(x), int(sum(m["z_dims"]))
    dt = v.dtype
    z = OC.mh_init_state(n, q, seed, row0).astype(dt)
    lp, gr = log_posterior_and_grad(m, x, y, v, z)
    step = np.full(n, np.float32(step0), np.float32)
    up = np.zeros(0, np.float32) if up is None else np.asarray(up, np.float32)
    dn = np.zeros(0, np.float32) if dn is None else np.asarray(dn, np.float32)
    draws, accs = [], []
    for it in range(burn_in + n_keep):
        z, lp, gr, _, acc = hmc_transition(m, x, y, v, z, lp, gr, step, n_leapfrog, it, seed, row0)
        if it < len(up):
            step = np.minimum(np.maximum(step * np.where(acc, up[it], dn[it]).astype(np.float32), np.float32(S_MIN)), np.float32(S_MAX))
            assert step.dtype == np.float32
        accs.append(acc)
        if it >= burn_in:
            draws.append(z.copy())
    return dict(draws=np.array(draws).reshape(n_keep, n, q), state=z, logp=lp, grad=gr, acc=np.array(accs).reshape(burn_in + n_keep, n), step=step)
