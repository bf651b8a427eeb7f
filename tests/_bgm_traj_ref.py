"""NumPy restatement of the BGM HMC sampler with a step size AND a number of leapfrog steps per chain (TEST INFRASTRUCTURE):
tests/_bgm_row_step_ref.py::hmc_transition with L_i per row by the rule of bgm_bgm_hmc_run_rows_traj -- the cap of
row_adapt.leapfrog_cap from the row's current float32 step, the jitter uniform of call 1 of the accept purpose -- plus the count of the
steps taken.  Everything takes the dtype of x: float64 for the reference's own error, float32 for chain parity; the steps, the caps
and the jitter are float32 in both.  Nothing is added to oracle/."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bgm_row_step_ref import PARITY, PARITY_CASES  # noqa: E402,F401

from oracle import bgm as OB  # noqa: E402
from oracle import rng as R  # noqa: E402

from bayesgm_amd.row_adapt import S_MAX, S_MIN, leapfrog_cap, row_adapt_factors  # noqa: E402

# the parity settings of the trajectory tests (host and GPU): the row-step cases at L = 6 under a cap that binds late in burn-in
TRAJ_PARITY = dict(PARITY, n_leapfrog=6, max_trajectory=0.4)


def leapfrog_steps(step, n_leapfrog, max_trajectory, jitter, rows, it, seed):
    """L_i [n] int32 of iteration `it` from the rows' current float32 steps."""
    cap = leapfrog_cap(step, n_leapfrog, max_trajectory)
    if not jitter:
        return cap
    u = R.uniforms(rows, it, R.TAG_HACC, seed, call=1)
    assert u.dtype == np.float32
    k = (u * cap.astype(np.float32)).astype(np.int32)      # (float32 product, truncated)
    return (1 + np.minimum(cap - 1, k)).astype(np.int32)


def hmc_transition(m, z, x, mask, step, li, it, seed, row0, lp, gr):
    """_bgm_row_step_ref.hmc_transition with li [n] leapfrog steps per row -> (z, lp, gr, log_accept_ratio, accepted): row i drifts and
    kicks for l < li[i], its last half kick comes at l == li[i] - 1, and the log posterior and gradient it carries are those of the
    point after li[i] steps."""
    n, q = z.shape
    rows = np.arange(row0, row0 + n)
    mom = R.normals(rows, it, q, R.TAG_MOM, seed).astype(z.dtype)
    u = R.uniforms(rows, it, R.TAG_HACC, seed).astype(z.dtype)
    e = np.asarray(step).astype(z.dtype)[:, None]
    li = np.asarray(li)[:, None]
    h0 = -lp + (mom ** 2).sum(axis=1) / 2
    zc, pc = z.copy(), mom + e / 2 * gr
    lpc, grc = lp, gr
    for l in range(int(li.max())):
        on = l < li
        zc = np.where(on, zc + e * pc, zc)
        lpn, grn = OB.log_posterior_and_grad(m, zc, x, mask)
        lpc, grc = np.where(on[:, 0], lpn, lpc), np.where(on, grn, grc)
        pc = np.where(on, pc + np.where(l < li - 1, e, e / 2) * grc, pc)
    h1 = -lpc + (pc ** 2).sum(axis=1) / 2
    with np.errstate(invalid="ignore"):
        log_ratio = -(h1 - h0)
    log_ratio = np.where(np.isfinite(log_ratio), log_ratio, -np.inf)
    acc = np.log(u) < log_ratio
    return np.where(acc[:, None], zc, z), np.where(acc, lpc, lp), np.where(acc[:, None], grc, gr), log_ratio, acc


def hmc_sampler(m, x, mask, n_mcmc, burn_in, step_size, n_leapfrog, seed, target=0.75, max_trajectory=None, jitter=False, row0=0,
                table=True):
    """_bgm_row_step_ref.hmc_sampler with the trajectory rule -> its dict plus li [burn_in + n_mcmc, n] int32 (the steps of every
    transition) and n_steps [n] int32 (their sum over the n_mcmc retained transitions)."""
    n, q = len(x), m["z_dim"]
    m = OB.cast_model(m, x.dtype)
    mask = mask.astype(x.dtype)
    rows = np.arange(row0, row0 + n)
    z = OB.hmc_init_state(n, q, seed, row0).astype(x.dtype)
    lp, gr = OB.log_posterior_and_grad(m, z, x, mask)
    step = np.full(n, np.float32(step_size), np.float32)
    up, dn = row_adapt_factors(burn_in, target) if table else (np.zeros(0, np.float32),) * 2
    draws, accs, lis = [], [], []
    for it in range(burn_in + n_mcmc):
        li = leapfrog_steps(step, n_leapfrog, max_trajectory, jitter, rows, it, seed)
        z, lp, gr, _, acc = hmc_transition(m, z, x, mask, step, li, it, seed, row0, lp, gr)
        if it < len(up):
            step = np.minimum(np.maximum(step * np.where(acc, up[it], dn[it]).astype(np.float32), np.float32(S_MIN)), np.float32(S_MAX))
            assert step.dtype == np.float32
        accs.append(acc)
        lis.append(li)
        if it >= burn_in:
            draws.append(z.copy())
    lis = np.array(lis, np.int32).reshape(burn_in + n_mcmc, n)
    return dict(draws=np.array(draws).reshape(n_mcmc, n, q), state=z, logp=lp, grad=gr, acc=np.array(accs).reshape(burn_in + n_mcmc, n),
                step=step, li=lis, n_steps=lis[burn_in:].sum(axis=0).astype(np.int32))
