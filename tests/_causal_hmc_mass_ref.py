"""NumPy restatement of the CausalBGM HMC sampler with a diagonal metric per chain (TEST INFRASTRUCTURE): the transition of
tests/_causal_hmc_ref.py with the step of coordinate i multiplied by the chain's s_i, the moments the kernel accumulates during an
estimation window, the update rule written out row by row (independently of bayesgm_amd.causal_hmc.mass_update), and the sampler
that runs the windows.  Everything takes the dtype of the data: float32 for chain parity."""
import math

import numpy as np

from _causal_hmc_ref import log_posterior_and_grad
from oracle import causal as OC
from oracle import rng as R

from bayesgm_amd.row_adapt import S_MAX, S_MIN


def leapfrog_mass(m, x, y, v, z, mom, gr, step, scale, n_leapfrog):
    """_causal_hmc_ref.leapfrog with the step vector es = step * scale [n, q] (float32 product, as the kernel forms it)"""
    e = (np.asarray(step, np.float32)[:, None] * np.asarray(scale, np.float32)).astype(z.dtype)
    zc, pc = z.copy(), mom + e / 2 * gr
    lpc, grc = None, gr
    for l in range(n_leapfrog):
        zc = zc + e * pc
        lpc, grc = log_posterior_and_grad(m, x, y, v, zc)
        pc = pc + (e if l < n_leapfrog - 1 else e / 2) * grc
    return zc, pc, lpc, grc


def hmc_transition_mass(m, x, y, v, z, lp, gr, step, scale, n_leapfrog, it, seed, row0=0):
    """_causal_hmc_ref.hmc_transition in the scaled form: momentum and kinetic energy as with identity mass"""
    n, q = z.shape
    rows = np.arange(row0, row0 + n)
    mom = R.normals(rows, it, q, R.TAG_MOM, seed).astype(z.dtype)
    u = R.uniforms(rows, it, R.TAG_HACC, seed).astype(z.dtype)
    h0 = -lp + (mom ** 2).sum(axis=1) / 2
    zc, pc, lpc, grc = leapfrog_mass(m, x, y, v, z, mom, gr, step, scale, n_leapfrog)
    h1 = -lpc + (pc ** 2).sum(axis=1) / 2
    with np.errstate(invalid="ignore"):
        log_ratio = -(h1 - h0)
    log_ratio = np.where(np.isfinite(log_ratio), log_ratio, -np.inf)
    acc = np.log(u) < log_ratio
    return np.where(acc[:, None], zc, z), np.where(acc, lpc, lp), np.where(acc[:, None], grc, gr), log_ratio, acc


def accumulate(z, ref, s1, s2):
    """one iteration of the kernel's moments, float32 in its order: d = z - ref, S1 += d, S2 = fma(d, d, S2) -> (s1, s2)"""
    d = (z.astype(np.float32) - ref.astype(np.float32)).astype(np.float32)
    s1 = (s1 + d).astype(np.float32)
    s2 = (d.astype(np.float64) * d.astype(np.float64) + s2.astype(np.float64)).astype(np.float32)      # the product is exact in float64
    return s1, s2


def scale_from_moments(W, s1, s2, prev):
    """The update rule for ONE chain in plain Python float64 -> float32 [q]; prev when the chain's mean variance is 0 or not finite."""
    q = len(s1)
    var = []
    for i in range(q):
        mean = float(s1[i]) / W
        var.append(max(float(s2[i]) / W - mean * mean, 0.0))
    vbar = sum(var) / q
    if not (vbar > 0.0 and math.isfinite(vbar)):
        return np.array(prev, np.float32)
    t = [math.sqrt((W * var[i] + 5e-3 * vbar) / (W + 5.0)) for i in range(q)]
    gm = math.exp(sum(math.log(ti) for ti in t) / q)
    return np.array([min(max(ti / gm, 0.05), 20.0) for ti in t], np.float32)


def update(W, state, scale, ref, s1, s2):
    """end of a window of W draws for [n x q] arrays -> (scale, ref, s1, s2); W = 0 only resets"""
    scale = np.array(scale, np.float32)
    if W > 0:
        scale = np.stack([scale_from_moments(W, s1[r], s2[r], scale[r]) for r in range(len(scale))])
    return scale, np.array(state, np.float32), np.zeros_like(scale), np.zeros_like(scale)


def hmc_mass_sampler(m, data, burn_in, n_keep, step0, n_leapfrog, seed, up, dn, row0=0, scale=None, windows=None):
    """_causal_hmc_ref.hmc_sampler with a metric: scale [n, q] frozen (windows None), or estimated in windows = (start, ends) from
    ones.  -> its dict plus scale [n, q] float32."""
    x, y, v = data
    n, q = len(x), int(sum(m["z_dims"]))
    dt = v.dtype
    z = OC.mh_init_state(n, q, seed, row0).astype(dt)
    lp, gr = log_posterior_and_grad(m, x, y, v, z)
    step = np.full(n, np.float32(step0), np.float32)
    scale = np.ones((n, q), np.float32) if scale is None else np.array(scale, np.float32)
    up = np.zeros(0, np.float32) if up is None else np.asarray(up, np.float32)
    dn = np.zeros(0, np.float32) if dn is None else np.asarray(dn, np.float32)
    marks = [] if windows is None else [int(windows[0])] + [int(e) for e in windows[1]]
    ref = s1 = s2 = None
    on = False
    draws, accs = [], []
    for it in range(burn_in + n_keep):
        z, lp, gr, _, acc = hmc_transition_mass(m, x, y, v, z, lp, gr, step, scale, n_leapfrog, it, seed, row0)
        if it < len(up):
            step = np.minimum(np.maximum(step * np.where(acc, up[it], dn[it]).astype(np.float32), np.float32(S_MIN)), np.float32(S_MAX))
            assert step.dtype == np.float32
        if on:
            s1, s2 = accumulate(z, ref, s1, s2)
        accs.append(acc)
        if it >= burn_in:
            draws.append(z.copy())
        if it + 1 in marks:
            k = marks.index(it + 1)
            scale, ref, s1, s2 = update(0 if k == 0 else marks[k] - marks[k - 1], z, scale, ref, s1, s2)
            on = k < len(marks) - 1
    return dict(draws=np.array(draws).reshape(n_keep, n, q), state=z, logp=lp, grad=gr, acc=np.array(accs).reshape(burn_in + n_keep, n),
                step=step, scale=scale)
