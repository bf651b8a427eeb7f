"""HMC latent sampler of CausalBGM (``sampler='hmc'``, ``hmc_sampler``): defaults, option checks and the row blocking of predict.

Every chain (one per row) runs Hamiltonian Monte Carlo with identity mass on log p(z | x, y, v) and carries a step size of its own,
adapted during burn-in by the table of row_adapt.py (one float32 multiply after each accept decision, towards the target acceptance
rate) and frozen afterwards.  The kernels are csrc/causal_hmc_kernels.h.  Nothing here touches the GPU.
"""
from . import row_adapt as RA

DEFAULT_TARGET = 0.75             # the target of the project's other HMC (tfp SimpleStepSizeAdaptation, bgm/base.py:709-830)
DEFAULT_STEP_SIZE = 0.1           # provisional: see README, "Results (HMC latent sampler)"
DEFAULT_N_LEAPFROG = 5
DRAW_BUDGET_BYTES = 2 << 30       # predict(sampler='hmc'): retained draws of one row block


def check_args(step_size, n_leapfrog, target):
    """step_size > 0, n_leapfrog >= 1, target None or in (0, 1); ValueError naming the option otherwise."""
    try:
        ok = float(step_size) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("step_size must be a positive number; got %r" % (step_size,))
    if isinstance(n_leapfrog, bool) or int(n_leapfrog) != n_leapfrog or int(n_leapfrog) < 1:
        raise ValueError("n_leapfrog must be an integer >= 1; got %r" % (n_leapfrog,))
    if target is not None and not (0.0 < float(target) < 1.0):
        raise ValueError("target_acceptance_rate must be in (0, 1); got %r" % (target,))


def check_supported(model, params):
    """The HMC sampler exists for the deterministic CausalBGM on the fp32 sampling kernels; everything else says which option is in
    the way (the C ABI answers BGM_E_UNSUPPORTED for the same paths)."""
    if model.startswith("Identifiable"):
        raise ValueError("sampler='hmc' / hmc_sampler is not available for %s: the gradient kernels exist for the standard-normal latent "
                         "prior only (IdentifiableCausalBGM samples under a conditional prior)" % model)
    if params.get("use_bnn", False):
        raise ValueError("sampler='hmc' / hmc_sampler is not available with params['use_bnn'] = True: the Bayesian-network sampling kernels "
                         "have no gradient path")
    prec = params.get("mh_precision", "fp32")
    if prec != "fp32":
        raise ValueError("sampler='hmc' / hmc_sampler needs params['mh_precision'] = 'fp32'; got %r (the split-precision kernels have no "
                         "gradient path)" % (prec,))


def resolve(model, params, step_size, n_leapfrog, target, adapt=True):
    """-> (step_size, n_leapfrog, target or None) with the defaults filled in, after every check above."""
    check_supported(model, params)
    step_size = DEFAULT_STEP_SIZE if step_size is None else step_size
    n_leapfrog = DEFAULT_N_LEAPFROG if n_leapfrog is None else n_leapfrog
    check_args(step_size, n_leapfrog, target)
    return float(step_size), int(n_leapfrog), (float(target) if adapt else None)


def check_predict_options(sampler, q_sd, row_adapt):
    """sampler of predict -> True for 'hmc'; row_adapt and the block-wide adaptive scale (q_sd None or <= 0) belong to 'mh'."""
    if sampler not in ("mh", "hmc"):
        raise ValueError("sampler must be 'mh' or 'hmc'; got %r" % (sampler,))
    if sampler == "mh":
        return False
    if RA.resolve_target(row_adapt) is not None:
        raise ValueError("sampler='hmc' and row_adapt exclude each other: row_adapt is the proposal scale of the MH sampler")
    if q_sd is None or not float(q_sd) > 0:
        raise ValueError("sampler='hmc' does not use q_sd; a non-positive q_sd asks for the block-wide adaptive scale of the MH sampler")
    return True


def block_rows(n_keep, q, budget_bytes=None):
    """Rows of one block of predict(sampler='hmc'): the block's retained draws [n_keep x rows x q] float32 stay within the budget;
    a multiple of 16 (whole row tiles), at least 16."""
    budget = DRAW_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
    if budget <= 0:
        raise ValueError("draw_budget_bytes must be positive; got %r" % (budget_bytes,))
    rows = budget // (4 * max(1, int(n_keep)) * max(1, int(q)))
    return max(16, rows // 16 * 16)
