"""Per-chain proposal scale of the CausalBGM Metropolis-Hastings sampler (``row_adapt``): the schedule and the option checks.

Every chain (one per row) carries a scale of its own.  After the accept decision of burn-in iteration t the chain multiplies its
scale by ``up[t]`` if it moved and by ``dn[t]`` if it did not, and clamps it to ``[S_MIN, S_MAX]``; from iteration ``burn_in`` on the
scale is frozen, so the retained draws come from a plain Metropolis-Hastings chain.  The factors are a Robbins-Monro step on the log
scale, ``log s += gamma_t (accepted - target)`` with ``gamma_t = (t + 1) ** -kappa``: stationary exactly when the chain's acceptance
frequency equals ``target``.  They are made HERE, in float64, and rounded once to float32; the kernel only multiplies
(csrc/causal_kernels.h, ROWADAPT), so NumPy float32 reproduces every scale bit for bit and a chain stays a function of (seed, global
row, the row's data) alone -- row blocks, rank shards, launch segments and ``diagnose_rows`` leave it unchanged.

Nothing here touches the GPU.
"""
import numpy as np

S_MIN, S_MAX = 1e-4, 1e2          # clamp of a chain's scale
DEFAULT_TARGET = 0.25             # the reference's target_acceptance_rate default (base.py:821)


def row_adapt_factors(burn_in, target, kappa=0.6):
    """(up, dn): float32 [burn_in] factors of an accepted / a rejected burn-in iteration."""
    burn_in = int(burn_in)
    target = float(target)
    if burn_in < 0:
        raise ValueError("row_adapt_factors: burn_in must be >= 0; got %r" % (burn_in,))
    if not (0.0 < target < 1.0):
        raise ValueError("row_adapt_factors: target must be in (0, 1); got %r" % (target,))
    if not (0.5 < float(kappa) <= 1.0):
        raise ValueError("row_adapt_factors: kappa must be in (0.5, 1] (Robbins-Monro step sizes); got %r" % (kappa,))
    gamma = (np.arange(burn_in, dtype=np.float64) + 1.0) ** -float(kappa)
    return np.exp(gamma * (1.0 - target)).astype(np.float32), np.exp(-gamma * target).astype(np.float32)


def resolve_target(row_adapt):
    """``row_adapt`` of predict / mh_sample -> None (off) or the target acceptance rate: False / None = off, True = 0.25, a number in
    (0, 1) = that target."""
    if row_adapt is None or row_adapt is False:
        return None
    if row_adapt is True:
        return DEFAULT_TARGET
    if isinstance(row_adapt, (bool, np.bool_)):
        return DEFAULT_TARGET if row_adapt else None
    try:
        t = float(row_adapt)
    except (TypeError, ValueError):
        raise ValueError("row_adapt must be False, True (target acceptance %.2f) or a target acceptance rate in (0, 1); got %r"
                         % (DEFAULT_TARGET, row_adapt))
    if not (0.0 < t < 1.0):
        raise ValueError("row_adapt: the target acceptance rate must be in (0, 1); got %r" % (row_adapt,))
    return t


STEP_DEFAULT_TARGET = 0.75        # BGM's HMC step per chain: the target of the shared rule (bgm/base.py:805-809) and causal_hmc.DEFAULT_TARGET


def resolve_step_target(row_adapt):
    """``row_adapt`` of BGM.predict / tfp_mcmc_sampler / BgmEngine.hmc_sample (an HMC step size per chain) -> None (off) or the target
    acceptance rate: False / None = off, True = 0.75, a number in (0, 1) = that target."""
    if row_adapt is None or (isinstance(row_adapt, (bool, np.bool_)) and not row_adapt):
        return None
    if isinstance(row_adapt, (bool, np.bool_)):
        return STEP_DEFAULT_TARGET
    t = float(row_adapt) if isinstance(row_adapt, (int, float, np.integer, np.floating)) else float("nan")
    if not (0.0 < t < 1.0):
        raise ValueError("row_adapt must be False, True (target acceptance %.2f) or a target acceptance rate in (0, 1); got %r"
                         % (STEP_DEFAULT_TARGET, row_adapt))
    return t


def leapfrog_cap(step, n_leapfrog, max_trajectory):
    """Leapfrog steps a BGM chain with step size ``step`` takes under ``max_trajectory`` = T (``max_trajectory`` of BGM.predict,
    bgm_bgm_hmc_run_rows_traj): the number of l in 0 .. n_leapfrog - 1 with ``l == 0 or float32(l) * step < T``, one float32 multiply
    and one compare per l as in the kernel (csrc/bgm_rowstep_kernels.h) -- clamp(ceil(T / step), 1, n_leapfrog) without a quotient, so
    NumPy reproduces every integer.  T = None or 0: no cap, n_leapfrog.  -> int32, the shape of ``step``."""
    step = np.asarray(step, np.float32)
    L = int(n_leapfrog)
    if L < 1:
        raise ValueError("leapfrog_cap: n_leapfrog must be >= 1; got %r" % (n_leapfrog,))
    if max_trajectory is None or float(max_trajectory) == 0.0:
        return np.full(step.shape, L, np.int32)
    T = np.float32(max_trajectory)
    cap = np.ones(step.shape, np.int32)
    for l in range(1, L):
        cap += (np.float32(l) * step < T).astype(np.int32)
    return cap


def resolve_trajectory(row_adapt_target, max_trajectory=None, jitter=False, what="max_trajectory / jitter"):
    """The trajectory options of the HMC step per chain -> (max_trajectory as a float, 0.0 = no cap; jitter as 0 / 1).  ``max_trajectory``
    is None or a finite number > 0, ``jitter`` a bool; either of them needs the step per chain (``row_adapt_target`` is what
    resolve_step_target returned), since the cap is derived from the chain's own step."""
    if isinstance(jitter, (bool, np.bool_)):
        jit = int(bool(jitter))
    elif isinstance(jitter, (int, np.integer)) and int(jitter) in (0, 1):
        jit = int(jitter)
    else:
        raise ValueError("jitter must be False or True; got %r" % (jitter,))
    T = 0.0
    if max_trajectory is not None:
        ok = isinstance(max_trajectory, (int, float, np.integer, np.floating)) and not isinstance(max_trajectory, (bool, np.bool_))
        T = float(max_trajectory) if ok else float("nan")
        if not (np.isfinite(T) and T > 0.0):
            raise ValueError("max_trajectory must be None (no cap) or a finite number > 0 (the cap on step x leapfrog steps); got %r"
                             % (max_trajectory,))
    if (T > 0.0 or jit) and row_adapt_target is None:
        raise ValueError("%s needs row_adapt (the HMC step per chain): the number of leapfrog steps is derived from the chain's own "
                         "step; got row_adapt off" % (what,))
    return T, jit


def start_scale(q_sd, initial_q_sd=1.0):
    """Scale every chain starts from: ``q_sd`` if positive, else ``initial_q_sd``, else 1."""
    for s in (q_sd, initial_q_sd):
        if s is not None and float(s) > 0:
            return float(s)
    return 1.0


def check_supported(model, params):
    """The per-chain scale exists for the deterministic CausalBGM on the fp32 sampling kernels; everything else says which option is
    in the way (the C ABI answers BGM_E_UNSUPPORTED for the same paths)."""
    if model.startswith("Identifiable"):
        raise ValueError("row_adapt / adaptive_sd='row' is not available for %s: the per-chain proposal scale exists for the standard-normal "
                         "latent prior only (the conditional prior of IdentifiableCausalBGM runs on kernels without it)" % model)
    if params.get("use_bnn", False):
        raise ValueError("row_adapt / adaptive_sd='row' is not available with params['use_bnn'] = True: the Bayesian-network sampling kernels "
                         "have no per-chain proposal scale")
    prec = params.get("mh_precision", "fp32")
    if prec != "fp32":
        raise ValueError("row_adapt / adaptive_sd='row' needs params['mh_precision'] = 'fp32'; got %r (the split-precision kernels have no "
                         "per-chain proposal scale)" % (prec,))
