"""NumPy restatement of the CausalBGM HMC sampler with a number of leapfrog steps per chain and iteration (TEST INFRASTRUCTURE):
tests/_causal_hmc_ref.py::hmc_transition with L_i per row by the rule of bgm_causal_hmc_set_trajectory -- the cap of
row_adapt.leapfrog_cap from the row's current float32 step, the jitter uniform of call 1 of the accept purpose -- plus the count of
the steps taken.  Everything takes the dtype of v: float64 for the restatement's own error, float32 for chain parity; the steps, the
caps and the jitter are float32 in both.  That module is imported unchanged; nothing is added to oracle/."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_ref as REF  # noqa: E402

from oracle import causal as OC  # noqa: E402
from oracle import rng as R  # noqa: E402

from bayesgm_amd.row_adapt import S_MAX, S_MIN, leapfrog_cap, row_adapt_factors  # noqa: E402

TARGET = 0.75
# the small parity cases of the trajectory tests (host and GPU): both first-layer tilings at p = 20, L = 6 under a cap that binds at
# the adapted steps (0.12 .. 0.4: 5 .. 2 of the 6 steps; all 6 at the starting step 0.1) and moves as the step adapts
PARITY_CASES = [dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=40), dict(z_dims=[3, 3, 6, 6], p=20, binary=True, n=40)]
PARITY = dict(burn_in=15, n_keep=15, step0=0.1, n_leapfrog=6, max_trajectory=0.6, seed=1234567890123)


def parity_inputs(case):
    """(model, (x, y, v)) of a parity case: tests/test_gpu_causal.py's _model(21, ...) and _data(n, p, 22, binary), restated here so
    that the host tests need no GPU test module"""
    m = OC.init_model(21, case["z_dims"], case["p"], binary_treatment=case["binary"])
    rs = np.random.RandomState(21 + 99)
    for k in ("g", "f", "h", "e"):
        m[k] = [(W.astype(np.float32), (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W, b in m[k]]
    rs = np.random.RandomState(22)
    n = case["n"]
    v = rs.randn(n, case["p"]).astype(np.float32)
    x = rs.exponential(size=(n, 1)).astype(np.float32)
    if case["binary"]:
        x = (x > np.median(x)).astype(np.float32)
    y = (x + rs.randn(n, 1)).astype(np.float32)
    return m, (x, y, v)


def leapfrog_steps(step, n_leapfrog, max_trajectory, jitter, rows, it, seed):
    """L_i [n] int32 of iteration `it` from the rows' current float32 steps."""
    cap = leapfrog_cap(step, n_leapfrog, max_trajectory)
    if not jitter:
        return cap
    u = R.uniforms(rows, it, R.TAG_HACC, seed, call=1)
    assert u.dtype == np.float32
    k = (u * cap.astype(np.float32)).astype(np.int32)      # (float32 product, truncated)
    return (1 + np.minimum(cap - 1, k)).astype(np.int32)


def hmc_transition(m, x, y, v, z, lp, gr, step, li, it, seed, row0=0, logp_grad=None):
    """_causal_hmc_ref.hmc_transition with li [n] leapfrog steps per row -> (z, lp, gr, log_accept_ratio, accepted): row i drifts and
    kicks for l < li[i], its last half kick comes at l == li[i] - 1, and the log posterior and gradient it carries are those of the
    point after li[i] steps."""
    logp_grad = logp_grad or REF.log_posterior_and_grad
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
        lpn, grn = logp_grad(m, x, y, v, zc)
        lpc, grc = np.where(on[:, 0], lpn, lpc), np.where(on, grn, grc)
        pc = np.where(on, pc + np.where(l < li - 1, e, e / 2) * grc, pc)
    h1 = -lpc + (pc ** 2).sum(axis=1) / 2
    with np.errstate(invalid="ignore"):
        log_ratio = -(h1 - h0)
    log_ratio = np.where(np.isfinite(log_ratio), log_ratio, -np.inf)
    acc = np.log(u) < log_ratio
    return np.where(acc[:, None], zc, z), np.where(acc, lpc, lp), np.where(acc[:, None], grc, gr), log_ratio, acc


def hmc_sampler(m, data, burn_in, n_keep, step0, n_leapfrog, seed, up=None, dn=None, max_trajectory=None, jitter=False, row0=0,
                logp_grad=None):
    """_causal_hmc_ref.hmc_sampler with the trajectory rule -> its dict plus li [burn_in + n_keep, n] int32 (the steps of every
    transition) and n_steps [n] int32 (their sum over the n_keep retained transitions).  step0: a number or float32 [n].
    logp_grad: the log posterior with its gradient (None: _causal_hmc_ref's; tests/_causal_partial_ref.py's for partial rows)."""
    logp_grad = logp_grad or REF.log_posterior_and_grad
    x, y, v = data
    n, q = len(x), int(sum(m["z_dims"]))
    dt = v.dtype
    rows = np.arange(row0, row0 + n)
    z = OC.mh_init_state(n, q, seed, row0).astype(dt)
    lp, gr = logp_grad(m, x, y, v, z)
    step = (np.zeros(n, np.float32) + np.asarray(step0, np.float32)).astype(np.float32)
    up = np.zeros(0, np.float32) if up is None else np.asarray(up, np.float32)
    dn = np.zeros(0, np.float32) if dn is None else np.asarray(dn, np.float32)
    draws, accs, lis = [], [], []
    for it in range(burn_in + n_keep):
        li = leapfrog_steps(step, n_leapfrog, max_trajectory, jitter, rows, it, seed)
        z, lp, gr, _, acc = hmc_transition(m, x, y, v, z, lp, gr, step, li, it, seed, row0, logp_grad)
        if it < len(up):
            step = np.minimum(np.maximum(step * np.where(acc, up[it], dn[it]).astype(np.float32), np.float32(S_MIN)), np.float32(S_MAX))
            assert step.dtype == np.float32
        accs.append(acc)
        lis.append(li)
        if it >= burn_in:
            draws.append(z.copy())
    lis = np.array(lis, np.int32).reshape(burn_in + n_keep, n)
    return dict(draws=np.array(draws).reshape(n_keep, n, q), state=z, logp=lp, grad=gr, acc=np.array(accs).reshape(burn_in + n_keep, n),
                step=step, li=lis, n_steps=lis[burn_in:].sum(axis=0).astype(np.int32))


def parity_run(case, jitter, dt=np.float32):
    """the restatement's run of a parity case in dtype dt, adapting, cap on"""
    m, (x, y, v) = parity_inputs(case)
    P = PARITY
    up, dn = row_adapt_factors(P["burn_in"], TARGET)
    data = tuple(a.astype(dt) for a in (x, y, v))
    return hmc_sampler(OC.cast_model(m, dt), data, P["burn_in"], P["n_keep"], P["step0"], P["n_leapfrog"], P["seed"], up, dn,
                       P["max_trajectory"], jitter)


def lag1(draws):
    """lag-1 autocorrelation of every series of draws [n_keep, ...] -> float64 [...] (nan for a constant series)"""
    d = np.asarray(draws, np.float64)
    c = d - d.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (c[1:] * c[:-1]).sum(axis=0) / (c * c).sum(axis=0)


# ---- the defect and its cure: a predict_new-type panel (x and y unobserved) under a frozen step with eps x L about 2 pi --------------
DEFECT = dict(z_dims=[1, 1, 1, 7], p=20, n=16, n_leapfrog=6, step=1.05, n_keep=200, seed=777, max_trajectory=float(np.pi / 2))


def defect_inputs():
    """(model, (x, y, v)) with x = y = NaN everywhere: the rows sample p(z | v).  g's weights are scaled down so that the posterior is
    close to the standard-normal prior, whose trajectories have period 2 pi."""
    D = DEFECT
    m = OC.init_model(5, D["z_dims"], D["p"])
    m["g"] = [((0.05 * W).astype(np.float32), b.astype(np.float32)) for W, b in m["g"]]
    v = np.random.RandomState(6).randn(D["n"], D["p"]).astype(np.float32)
    nan = np.full((D["n"], 1), np.nan, np.float32)
    return m, (nan, nan.copy(), v)


def defect_run(capped, dt=np.float64):
    """the restatement's run of the defect panel (0 + n_keep transitions, frozen step) without / with the cap -> hmc_sampler's dict"""
    import _causal_partial_ref as PR
    D = DEFECT
    m, (x, y, v) = defect_inputs()
    data = tuple(a.astype(dt) for a in (x, y, v))
    return hmc_sampler(OC.cast_model(m, dt), data, 0, D["n_keep"], D["step"], D["n_leapfrog"], D["seed"],
                       max_trajectory=D["max_trajectory"] if capped else None, logp_grad=PR.log_posterior_and_grad)
