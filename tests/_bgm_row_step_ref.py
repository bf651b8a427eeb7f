"""NumPy restatement of the BGM HMC sampler with a step size per chain (TEST INFRASTRUCTURE): oracle/bgm.py::hmc_transition with a
step per row (``e[:, None]``) and the per-chain table update of bayesgm_amd/row_adapt.py in float32.  Everything takes the dtype of x:
float64 for the reference's own error, float32 for chain parity.  Nothing is added to oracle/."""
import numpy as np

from oracle import bgm as OB
from oracle import rng as R

from bayesgm_amd.row_adapt import S_MAX, S_MIN, row_adapt_factors


def hmc_transition(m, z, x, mask, step, n_leapfrog, it, seed, row0, lp, gr):
    """oracle.bgm.hmc_transition with a step per row -> (z, lp, gr, log_accept_ratio, accepted)."""
    n, q = z.shape
    rows = np.arange(row0, row0 + n)
    mom = R.normals(rows, it, q, R.TAG_MOM, seed).astype(z.dtype)
    u = R.uniforms(rows, it, R.TAG_HACC, seed).astype(z.dtype)
    e = np.asarray(step).astype(z.dtype)[:, None]
    h0 = -lp + (mom ** 2).sum(axis=1) / 2
    zc, pc = z.copy(), mom + e / 2 * gr
    lpc, grc = lp, gr
    for l in range(n_leapfrog):
        zc = zc + e * pc
        lpc, grc = OB.log_posterior_and_grad(m, zc, x, mask)
        pc = pc + (e if l < n_leapfrog - 1 else e / 2) * grc
    h1 = -lpc + (pc ** 2).sum(axis=1) / 2
    with np.errstate(invalid="ignore"):
        log_ratio = -(h1 - h0)
    log_ratio = np.where(np.isfinite(log_ratio), log_ratio, -np.inf)
    acc = np.log(u) < log_ratio
    return np.where(acc[:, None], zc, z), np.where(acc, lpc, lp), np.where(acc[:, None], grc, gr), log_ratio, acc


def hmc_sampler(m, x, mask, n_mcmc, burn_in, step_size, n_leapfrog, seed, target=0.75, row0=0, table=True):
    """-> dict(draws [n_mcmc, n, q], state, logp, grad, acc [burn_in + n_mcmc, n] bool, step [n] float32).  table: after the decision
    of burn-in iteration it a row's step is multiplied in float32 by up[it] if it moved, by dn[it] if not, and clamped to
    [S_MIN, S_MAX], with (up, dn) = row_adapt_factors(burn_in, target); False: the steps stay at step_size."""
    n, q = len(x), m["z_dim"]
    m = OB.cast_model(m, x.dtype)
    mask = mask.astype(x.dtype)
    z = OB.hmc_init_state(n, q, seed, row0).astype(x.dtype)
    lp, gr = OB.log_posterior_and_grad(m, z, x, mask)
    step = np.full(n, np.float32(step_size), np.float32)
    up, dn = row_adapt_factors(burn_in, target) if table else (np.zeros(0, np.float32),) * 2
    draws, accs = [], []
    for it in range(burn_in + n_mcmc):
        z, lp, gr, _, acc = hmc_transition(m, z, x, mask, step, n_leapfrog, it, seed, row0, lp, gr)
        if it < len(up):
            step = np.minimum(np.maximum(step * np.where(acc, up[it], dn[it]).astype(np.float32), np.float32(S_MIN)), np.float32(S_MAX))
            assert step.dtype == np.float32
        accs.append(acc)
        if it >= burn_in:
            draws.append(z.copy())
    return dict(draws=np.array(draws).reshape(n_mcmc, n, q), state=z, logp=lp, grad=gr, acc=np.array(accs).reshape(burn_in + n_mcmc, n),
                step=step)


# the parity cases of tests/test_gpu_bgm_row_step.py, shared with the host test of the restatement's own error
PARITY = dict(burn_in=40, n_mcmc=10, n_leapfrog=4, step_size=0.02, target=0.75, seed=77)
PARITY_CASES = [dict(q=10, p=100, n=150, nh=5), dict(q=10, p=20, n=64, nh=5), dict(q=10, p=500, n=150, nh=5),
                dict(q=10, p=61, n=2100, nh=5), dict(q=3, p=20, n=17, nh=3)]
