"""HMC latent sampler of CausalBGM (``sampler='hmc'``, ``hmc_sampler``): defaults, option checks and the row blocking of predict.

Every chain (one per row) runs Hamiltonian Monte Carlo with identity mass on log p(z | x, y, v) and carries a step size of its own,
adapted during burn-in by the table of row_adapt.py (one float32 multiply after each accept decision, towards the target acceptance
rate) and frozen afterwards.  The kernels are csrc/causal_hmc_kernels.h.  Nothing here touches the GPU.

``mass='diag'`` (opt-in): a chain also carries a scale per coordinate, s in R^q, the metric M^-1 = diag(s^2) in the scaled form
(the step of coordinate i is eps s_i; momentum and kinetic energy are those of identity mass).  s is estimated by the chain alone
from its own burn-in draws, in the windows of ``mass_windows``, and frozen afterwards; the step table restarts its Robbins-Monro gain
at every change of the metric (``mass_schedule``).

``max_trajectory`` / ``jitter_leapfrog`` (opt-in): a chain takes only as many of the ``n_leapfrog`` steps as keep step x steps below
``max_trajectory``, and with the jitter a number uniform on 1 .. that cap per transition (``resolve_trajectory``; the cap is
row_adapt.leapfrog_cap; csrc/causal_hmc_traj_kernels.h).

``RESULT_KINDS``: one record per kind of result the kernels keep (panel ADRF, ITE, label sums, per-row curve, tails, contrasts,
choice) saying which combinations with the options are built; ``result_kind`` / ``check_result`` refuse the others from it.

``predict_individual``: the option checks, the row blocks of ``interval='quantile'`` and ``'tails'``, the size of a tail buffer
(``tail_size``), the finalisation of the per-row moments and the subgroup formula (``group_dose_response``) are at the end of the module.

``predict_dose_effect``: the contrast of every dose against a baseline dose (csrc/causal_hmc_contrast_kernels.h); its own checks are
``check_dose_effect`` and ``check_partial_panel``, everything else is predict_individual's.

``predict_best_dose``: the choice among the doses, compared per retained draw (csrc/causal_hmc_choice_kernels.h); its own checks are
``check_best_dose`` / ``check_threshold``, its finishing helpers ``choice_finalize`` and ``group_dose_choice``.

``predict_average``: the option checks, the internal row labels and the combiner of the per-draw label sums into ATE / ATT / ATC
(``combine_average_effects``) follow them.

``predict_new`` / ``partial=True``: rows whose outcome, or outcome and treatment, are not observed carry NaN there; the checks of the
pattern (``check_partial_rows``) and of predict_new's own options (``check_new``) close the module.
"""
import collections

import numpy as np

from . import _lib
from . import row_adapt as RA

DEFAULT_TARGET = 0.75             # the target of the project's other HMC (tfp SimpleStepSizeAdaptation, bgm/base.py:709-830)
DEFAULT_STEP_SIZE = 0.1           # provisional: see README, "Results (HMC latent sampler)"
DEFAULT_N_LEAPFROG = 5
DRAW_BUDGET_BYTES = 2 << 30       # predict(sampler='hmc'): retained draws of one row block
MASS_INIT_BUFFER, MASS_BASE_WINDOW, MASS_TERM_BUFFER = 75, 25, 50      # Stan's warm-up windows (init_buffer, base_window, term_buffer)
MASS_MIN_BURN_IN = 20             # below this no window is long enough to estimate a variance from
MASS_SHRINK = 5.0                 # weight (in draws) of the shrinkage target in the regularised variances (Stan's 5)
MASS_SHRINK_TARGET = 1e-3         # the target, in units of the chain's mean variance (Stan's 1e-3 presumes unit scale)
MASS_S_MIN, MASS_S_MAX = 0.05, 20.0      # clamp of a coordinate's scale relative to the chain's geometric mean


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


# ---- what exists with what: one record per kind of result the sampler computes inside its kernels -----------------------------------
# A kind is what one family of kernels keeps per retained draw.  Its record says how engine.hmc_sample is asked for it (`request`,
# and `option`, the words for that in a refusal), which engine method and kernels run it (`method`, `kernels`: the words of a
# refusal again), and which combinations are built:
#   treatment  "continuous" / "binary": the treatment type it is for; `wrong_treatment` is the refusal for the other one
#   traj       it has twins with a trajectory length per chain (max_trajectory / jitter)
#   obs        it has twins for partially observed rows (partial=True)
#   draws      it can also store the series it summarises (row_draws=True)
#   tails      it can also keep the two tails of that series (row_tails=K)
#   hole       q or None: the one combination of a built family that is not built -- a metric together with partial=True at more
#              than q latent features (check_choice_kernel)
#   late       which of "treatment" / "obs" engine.hmc_sample does not refuse before a device is touched.  They are refused once it
#              is: the other treatment type by the per-row route (ValueError, `wrong_treatment`) or by hmc_run (ValueError for the
#              effect of the other type), the pattern by the library at the first launch (BGM_E_UNSUPPORTED)
# Everything else that does not exist is a ValueError of check_result, before a device is touched.  The library refuses the same
# combinations on its own (csrc/causal_hmc_fx_host.h and the entry points); a new kind is one record here, one in
# CausalEngine._row_routes where it is a per-row kind, and its own checks.
ResultKind = collections.namedtuple("ResultKind", "name request option method kernels treatment wrong_treatment traj obs draws tails hole late")
_CONTINUOUS = "hmc_sample: %s is %s of a continuous treatment; a binary treatment has its per-row effect already (effect=EFFECT_ITE)"
RESULT_KINDS = collections.OrderedDict((k.name, k) for k in (
    ResultKind("adrf", dict(effect=_lib.EFFECT_ADRF), "effect=EFFECT_ADRF", "hmc_run", "the fused-effect kernels", "continuous", None,
               traj=True, obs=False, draws=False, tails=False, hole=None, late=("treatment", "obs")),
    ResultKind("ite", dict(effect=_lib.EFFECT_ITE), "effect=EFFECT_ITE", "hmc_run", "the fused-effect kernels", "binary", None,
               traj=True, obs=True, draws=False, tails=False, hole=None, late=("treatment",)),
    ResultKind("group_ite", dict(effect=_lib.EFFECT_GROUP_ITE), "effect=EFFECT_GROUP_ITE", "hmc_run_group_effects", "the label-sum kernels",
               "binary", "hmc_sample: effect=EFFECT_GROUP_ITE sums the treatment effect of a binary treatment; a continuous treatment has "
               "its dose-response (effect=EFFECT_ADRF)", traj=False, obs=False, draws=False, tails=False, hole=None, late=("obs",)),
    ResultKind("rows", dict(row_effects=True), "row_effects", "hmc_run_rows_effects", "the per-row kernels", "continuous",
               _CONTINUOUS % ("row_effects", "the dose-response"), traj=True, obs=True, draws=True, tails=True, hole=None, late=("treatment",)),
    # (asked for as rows with row_tails=K; the tails of the contrasts belong to the contrasts)
    ResultKind("tails", dict(row_effects=True), "row_tails", "hmc_run_rows_tails", "the tail-buffer kernels", "continuous",
               _CONTINUOUS % ("row_effects", "the dose-response"), traj=False, obs=True, draws=True, tails=True, hole=None, late=("treatment",)),
    ResultKind("contrasts", dict(row_effects=True, row_contrasts=True), "row_contrasts", "hmc_run_rows_contrasts", "the dose-contrast kernels",
               "continuous", _CONTINUOUS % ("row_contrasts", "the contrast between two doses"), traj=False, obs=True, draws=True, tails=True,
               hole=None, late=()),
    ResultKind("choice", dict(row_effects=True, row_choice=True), "row_choice", "hmc_run_rows_choice", "the dose-choice kernels",
               "continuous", _CONTINUOUS % ("row_choice", "the choice among the doses"), traj=False, obs=True, draws=True, tails=False,
               hole=11, late=()),
))
NO_TRAJECTORY = "%s (%s) have no variant with a trajectory length per chain"


def result_kind(effect, row_effects=False, row_tails=None, row_contrasts=False, row_choice=False):
    """The record of RESULT_KINDS that engine.hmc_sample's options ask for (None: the chain alone); ValueError for an effect that
    is none, and for a per-row option without row_effects or beside an effect."""
    by_effect = {_lib.EFFECT_NONE: None, _lib.EFFECT_ADRF: "adrf", _lib.EFFECT_ITE: "ite", _lib.EFFECT_GROUP_ITE: "group_ite"}
    if effect not in by_effect:
        raise ValueError("hmc_sample: effect must be EFFECT_NONE, EFFECT_ADRF, EFFECT_ITE or EFFECT_GROUP_ITE; got %r" % (effect,))
    if not row_effects:
        for name, asked in (("row_choice", row_choice), ("row_contrasts", row_contrasts)):
            if asked:
                raise ValueError("hmc_sample: %s belongs to row_effects=True" % name)
        return RESULT_KINDS.get(by_effect[effect])
    if effect != _lib.EFFECT_NONE:
        raise ValueError("hmc_sample: row_effects and effect exclude each other (the panel's ADRF is the mean of the rows' curves)")
    return RESULT_KINDS["choice" if row_choice else "contrasts" if row_contrasts else "tails" if row_tails is not None else "rows"]


def check_result(kind, binary, traj=False, row_draws=False, row_tails=None, row_contrasts=False):
    """What engine.hmc_sample refuses of a result kind (result_kind) before a device is touched, read from its record: stored
    series and tails where the kind takes none, a trajectory option without TRAJ twins, the other treatment type.  `binary` is a
    callable, asked only where the record needs the answer.  ValueError with the record's words."""
    per_row = kind is not None and kind.request.get("row_effects", False)
    if row_draws and not (kind is not None and kind.draws):
        raise ValueError("hmc_sample: row_draws belongs to row_effects=True")
    if row_tails is not None and not per_row:
        raise ValueError("hmc_sample: row_tails belongs to row_effects=True")
    if (row_tails is not None and not kind.tails) or (row_contrasts and kind.name != "contrasts"):
        raise ValueError("hmc_sample: %s is not available with row_contrasts or row_tails: %s (%s) have no variant with contrasts or "
                         "tail buffers" % (kind.option, kind.kernels, kind.method))
    # (the tails of another kind are kept by that kind's kernels, and none of those has what the tail-buffer kernels lack)
    for k in ([RESULT_KINDS["tails"]] if per_row and row_tails is not None else []) + ([kind] if kind is not None else []):
        if traj and not k.traj:
            raise ValueError("hmc_sample: max_trajectory / jitter are not available with %s: " % k.option + NO_TRAJECTORY % (k.kernels, k.method))
    if kind is not None and "treatment" not in kind.late and binary() != (kind.treatment == "binary"):
        raise ValueError(kind.wrong_treatment)


def resolve_trajectory(max_trajectory=None, jitter=False):
    """The trajectory options of the HMC sampler (``max_trajectory`` / ``jitter_leapfrog``; bgm_causal_hmc_set_trajectory) ->
    (max_trajectory as a float, 0.0 = no cap; jitter as 0 / 1).  ``max_trajectory`` is None or a finite number > 0, ``jitter`` a
    bool: the checks of row_adapt.resolve_trajectory without its row_adapt requirement, since this sampler's step is always per
    chain.  The cap itself is row_adapt.leapfrog_cap(step, n_leapfrog, max_trajectory), taken from the chain's step alone also with
    mass='diag' (the metric's scales have geometric mean 1, so the step keeps the size)."""
    return RA.resolve_trajectory(DEFAULT_TARGET, max_trajectory, jitter)


def check_trajectory(max_trajectory, jitter, hmc=True, interval=None):
    """resolve_trajectory for predict / predict_individual / predict_new: either option belongs to sampler='hmc' and has no
    tail-buffer kernel (interval='tails'); ValueError naming what is in the way, before a device is touched."""
    T, jit = resolve_trajectory(max_trajectory, jitter)
    if T > 0.0 or jit:
        if not hmc:
            raise ValueError("max_trajectory / jitter_leapfrog belong to sampler='hmc': the MH sampler has no trajectory (sampler='mh')")
        kind = RESULT_KINDS["tails" if interval == "tails" else "rows"]
        if not kind.traj:
            raise ValueError("max_trajectory / jitter_leapfrog are not available with interval='%s': %s have no variant with a "
                             "trajectory length per chain; use interval='quantile' or 'normal'" % (interval, kind.kernels))
    return T, jit


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


def check_fused(fused_effects, hmc, draw_budget_bytes):
    """fused_effects of predict: it belongs to sampler='hmc' and keeps no draws, so it has no draw budget; ValueError otherwise."""
    if not fused_effects:
        return
    if not hmc:
        raise ValueError("fused_effects=True belongs to sampler='hmc': the MH sampler always computes its effects inside the kernel")
    if draw_budget_bytes is not None:
        raise ValueError("fused_effects=True and draw_budget_bytes exclude each other: the fused route stores no draws and samples "
                         "a rank's rows in one piece")


def predict_blocks(blocks, n_keep, q, draw_budget_bytes=None, fused_effects=False):
    """The row blocks [(start, stop)] of predict(sampler='hmc') cut to block_rows(n_keep, q, draw_budget_bytes) rows each; with
    fused_effects no draws are stored and the blocks stay whole."""
    if fused_effects:
        return list(blocks)
    rows = block_rows(n_keep, q, draw_budget_bytes)
    return [(s0, min(s0 + rows, e0)) for (b0, e0) in blocks for s0 in range(b0, e0, rows)]


def check_mass(mass, hmc=True, adapt=True, burn_in=None):
    """mass of predict / hmc_sampler -> None ('identity' or None) or 'diag'; ValueError for anything else, for 'diag' without the HMC
    sampler, without step adaptation, or with a burn-in too short for one window."""
    if mass is None or mass == "identity":
        return None
    if mass != "diag":
        raise ValueError("mass must be 'identity' or 'diag'; got %r" % (mass,))
    if not hmc:
        raise ValueError("mass='diag' belongs to sampler='hmc': the MH sampler has no metric (its per-chain scale is row_adapt)")
    if adapt is None or adapt is False:
        raise ValueError("mass='diag' needs adapt=True: a change of the metric without re-adapting the step leaves the step of the old metric")
    if burn_in is not None and not mass_windows(burn_in)[1]:
        raise ValueError("mass='diag' needs burn_in >= %d (no estimation window fits); got burn_in = %r" % (MASS_MIN_BURN_IN, burn_in))
    return "diag"


def mass_windows(burn_in):
    """(start, [end_1, ..., end_k]): the metric is estimated from the draws of [start, end_1), [end_1, end_2), ... and updated at
    every end.  An initial buffer of 75 iterations, windows of 25, 50, 100, ... and a terminal buffer of 50; a window whose successor
    would not fit before the terminal buffer is stretched to it.  When 75 + 25 + 50 > burn_in: 15 % / 75 % / 10 % of burn_in with one
    window.  burn_in < 20: no windows."""
    burn_in = int(burn_in)
    if burn_in < MASS_MIN_BURN_IN:
        return max(burn_in, 0), []
    if MASS_INIT_BUFFER + MASS_BASE_WINDOW + MASS_TERM_BUFFER > burn_in:
        return burn_in * 15 // 100, [burn_in - burn_in * 10 // 100]
    start, last = MASS_INIT_BUFFER, burn_in - MASS_TERM_BUFFER
    ends, size, end = [], MASS_BASE_WINDOW, MASS_INIT_BUFFER
    while end < last:
        end += size
        size *= 2
        if end + size > last:
            end = last
        ends.append(end)
    return start, ends


def check_windows(windows, burn_in):
    """(start, ends) -> (int, [int]) with 1 <= start < end_1 < ... < end_k <= burn_in; ValueError otherwise."""
    try:
        start, ends = int(windows[0]), [int(e) for e in windows[1]]
    except (TypeError, ValueError, IndexError):
        raise ValueError("mass_windows must be (start, [end_1, ..., end_k]); got %r" % (windows,))
    marks = [start] + ends
    if not ends or start < 1 or ends[-1] > int(burn_in) or any(b <= a for a, b in zip(marks[:-1], marks[1:])):
        raise ValueError("mass_windows needs 1 <= start < end_1 < ... < end_k <= burn_in (= %d); got %r" % (int(burn_in), windows))
    return start, ends


def mass_schedule(burn_in, target, windows=None):
    """((start, ends), (up, dn)): the windows (``windows`` or mass_windows(burn_in)) and the step table of the whole burn-in, the
    concatenation of row_adapt_factors(len, target) over [0, start), every window and [end_k, burn_in): the Robbins-Monro gain
    restarts whenever the metric changes.  ValueError naming burn_in when no window fits."""
    burn_in = int(burn_in)
    if windows is None:
        windows = mass_windows(burn_in)
        if not windows[1]:
            raise ValueError("mass='diag' needs burn_in >= %d (no estimation window fits); got burn_in = %r" % (MASS_MIN_BURN_IN, burn_in))
    start, ends = check_windows(windows, burn_in)
    marks = [0, start] + ends + [burn_in]
    parts = [RA.row_adapt_factors(b - a, target) for a, b in zip(marks[:-1], marks[1:])]
    return (start, ends), (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def mass_update(W, state, scale, ref, s1, s2):
    """The update of a chain's metric at the end of a window of W draws, as the device does it (csrc/causal_hmc_kernels.h,
    causal_hmc_mass_update_kernel), in NumPy float64 on [n x q] arrays -> (scale float32, ref, s1, s2).  With d = z - ref summed
    into s1 and d^2 into s2: var_i = max(s2_i / W - (s1_i / W)^2, 0), shrunk towards 1e-3 of the chain's mean variance vbar with the
    weight of 5 draws, var_r_i = (W var_i + 5e-3 vbar) / (W + 5); s_i = sqrt(var_i) over the geometric mean of the chain, clamped to [0.05, 20]: only the shape, the step keeps the
    scale.  A chain whose vbar is zero or not finite keeps its scales; W = 0 only resets.  Then ref = state, s1 = s2 = 0."""
    scale = np.array(scale, np.float32)
    if W > 0:
        with np.errstate(all="ignore"):
            mean = np.asarray(s1, np.float64) / W
            var = np.maximum(np.asarray(s2, np.float64) / W - mean * mean, 0.0)
            vbar = var.mean(axis=1, keepdims=True)
            t = np.sqrt((W * var + MASS_SHRINK * MASS_SHRINK_TARGET * vbar) / (W + MASS_SHRINK))
            new = np.clip(t / np.exp(np.log(t).mean(axis=1, keepdims=True)), MASS_S_MIN, MASS_S_MAX).astype(np.float32)
        ok = (np.isfinite(vbar) & (vbar > 0))[:, 0]
        scale[ok] = new[ok]
    return scale, np.array(state, np.float32), np.zeros_like(scale), np.zeros_like(scale)


# ---- predict_individual: the dose-response of every row (csrc/causal_hmc_rowfx_kernels.h) ----------------------------------------
INTERVALS = ("normal", "quantile", "tails")


def check_interval(interval):
    """interval of predict_individual / predict_new: one of INTERVALS; ValueError otherwise."""
    if interval not in INTERVALS:
        raise ValueError("interval must be 'normal' or 'quantile'; got %r (or 'tails': the bounds of 'quantile' from the two tail buffers "
                         "of every series, kept inside the sampler)" % (interval,))


def tail_size(alpha, m):
    """K of interval='tails': how many of the smallest and of the largest of m retained values the two bounds read.  With q = alpha / 2
    and 1 - alpha / 2, vi = q * (m - 1) in double, i0 = floor(vi) clamped to [0, m - 1] and i1 = min(i0 + 1, m - 1) -- the arithmetic
    of bgm_row_mean_quantiles, restated operation for operation and never as a closed form (0.55 * 100 is 55.00000000000001 in double) -- the
    lower bound reads the i1 + 1 smallest values and the upper one the m - i0 largest: K = min(m, max(i1_lo + 1, m - i0_hi)).
    K = m (few draws or a wide alpha) keeps everything."""
    m = int(m)
    if m < 1:
        raise ValueError("tail_size: m must be >= 1; got %r" % (m,))
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("tail_size: alpha must be in [0, 1]; got %r" % (alpha,))

    def idx(q):
        vi = q * float(m - 1)
        i0 = min(max(int(np.floor(vi)), 0), m - 1)
        return i0, min(i0 + 1, m - 1)
    (_, i1_lo), (i0_hi, _) = idx(alpha / 2), idx(1 - alpha / 2)
    return min(m, max(i1_lo + 1, m - i0_hi))


def check_individual(binary, x_values, interval, draw_budget_bytes):
    """The options of predict_individual that are its own: a continuous treatment, x_values, interval 'normal', 'quantile' or
    'tails', and a draw budget only where something of size n_keep or K is stored; ValueError otherwise."""
    if binary:
        raise ValueError("predict_individual is the dose-response of every row under a continuous treatment; a binary treatment has "
                         "its per-row effect already: predict's ITE")
    if x_values is None:
        raise ValueError("predict_individual needs x_values: the doses at which every row's outcome is evaluated")
    check_interval(interval)
    if interval != "normal" and draw_budget_bytes is not None and int(draw_budget_bytes) <= 0:
        raise ValueError("draw_budget_bytes must be positive; got %r" % (draw_budget_bytes,))
    if interval == "normal" and draw_budget_bytes is not None:
        raise ValueError("interval='normal' and draw_budget_bytes exclude each other: the moments store no draws and this rank's rows "
                         "are sampled in one piece")


def check_dose_effect(binary, x_values, baseline, interval, draw_budget_bytes):
    """The options of predict_dose_effect that are its own: a continuous treatment, x_values, a finite scalar baseline, and
    interval / draw_budget_bytes by predict_individual's rules -> baseline as a float; ValueError otherwise."""
    if binary:
        raise ValueError("predict_dose_effect is the contrast between two doses of a continuous treatment; a binary treatment has "
                         "its per-row effect already: predict's ITE")
    if x_values is None:
        raise ValueError("predict_dose_effect needs x_values: the doses whose outcome is compared with the baseline's")
    try:
        b = float(baseline) if np.ndim(baseline) == 0 and not isinstance(baseline, (bool, str)) else float("nan")
    except (TypeError, ValueError):
        b = float("nan")
    if not np.isfinite(b):
        raise ValueError("baseline must be a finite scalar, the dose every other dose is compared with; got %r" % (baseline,))
    check_individual(False, x_values, interval, draw_budget_bytes)
    return b


def individual_block_rows(n_keep, n_doses, budget_bytes=None):
    """Rows of one block of predict_individual(interval='quantile'): the block's outcome draws [rows x n_doses x n_keep] float32
    stay within the budget; a multiple of 16 (whole row tiles), at least 16."""
    return block_rows(n_keep, n_doses, budget_bytes)


def tails_block_rows(k_tail, n_doses, budget_bytes=None):
    """Rows of one block of predict_individual(interval='tails'): the block's tail buffers [2 x k_tail x n_doses x rows] float32 stay
    within the budget, rows = budget // (8 * k_tail * n_doses); a multiple of 16 (whole row tiles), at least 16."""
    return block_rows(2 * int(k_tail), n_doses, budget_bytes)


def individual_blocks(blocks, n_keep, n_doses, interval, draw_budget_bytes=None, k_tail=None):
    """The row blocks [(start, stop)] of predict_individual: whole for interval='normal' (nothing of size n_keep is stored), cut to
    individual_block_rows rows each for 'quantile' and to tails_block_rows(k_tail, n_doses) rows each for 'tails'."""
    if interval == "normal":
        return list(blocks)
    if interval == "tails":
        rows = tails_block_rows(k_tail, n_doses, draw_budget_bytes)
    else:
        rows = individual_block_rows(n_keep, n_doses, draw_budget_bytes)
    return [(s0, min(s0 + rows, e0)) for (b0, e0) in blocks for s0 in range(b0, e0, rows)]


def row_moments_finalize(ref, s1, s2, m):
    """The shifted sums of m retained values (ref = the first value, s1 = sum of y - ref, s2 = sum of (y - ref)^2; NumPy arrays or
    torch tensors of one shape) -> (mean, sd) in float64: mean = ref + s1 / m, var = (s2 - s1^2 / m) / (m - 1), clamped at 0 so that
    a constant series gives sd 0 and no NaN.  m = 1 has no spread: sd 0."""
    ref, s1, s2 = ((a.double() if hasattr(a, "double") else np.asarray(a, np.float64)) for a in (ref, s1, s2))
    m = int(m)
    mean = ref + s1 / m
    if m < 2:
        return mean, mean * 0.0
    var = (s2 - s1 * s1 / m) / (m - 1)
    var = var * (var > 0)
    return mean, var ** 0.5


def group_dose_response(mean, sd, groups):
    """Subgroup curves from the rows' (mean, sd) [n, n_doses] and int labels [n] -> {label: (mean_g [n_doses], sd_g [n_doses])},
    float64: mean_g = mean over the group's rows of mean_ik, sd_g = sqrt(sum_i sd_ik^2) / m_g.  The sd is exact, not an
    approximation: given the fitted networks the posterior factorises over rows, and the chains and noise streams are keyed per row,
    so the rows' values are independent and the variance of their average is the sum of their variances over m_g^2."""
    mean, sd = np.asarray(mean, np.float64), np.asarray(sd, np.float64)
    labels = np.asarray(groups)
    if labels.shape != (mean.shape[0],) or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("groups must be integer labels of shape [n] = (%d,); got %s of shape %r" % (mean.shape[0], labels.dtype, labels.shape))
    out = {}
    for g in np.unique(labels):
        rows = labels == g
        m_g = int(rows.sum())
        out[int(g)] = (mean[rows].sum(axis=0) / m_g, np.sqrt((sd[rows] ** 2).sum(axis=0)) / m_g)
    return out


# ---- predict_best_dose: the choice among the doses, compared per retained draw (csrc/causal_hmc_choice_kernels.h) -----------------
def check_threshold(threshold):
    """None, or a finite scalar -> None or float; ValueError otherwise."""
    if threshold is None:
        return None
    try:
        t = float(threshold) if np.ndim(threshold) == 0 and not isinstance(threshold, (bool, str)) else float("nan")
    except (TypeError, ValueError):
        t = float("nan")
    if not np.isfinite(t):
        raise ValueError("threshold must be None or a finite scalar, the outcome a dose is asked to exceed; got %r" % (threshold,))
    return t


def check_best_dose(binary, x_values, threshold):
    """The options of predict_best_dose that are its own: a continuous treatment, x_values and a finite threshold (or None) ->
    threshold as a float or None; ValueError otherwise."""
    if binary:
        raise ValueError("predict_best_dose is the choice among the doses of a continuous treatment; a binary treatment has "
                         "its per-row effect already: predict's ITE")
    if x_values is None:
        raise ValueError("predict_best_dose needs x_values: the doses among which every row's best is looked for")
    return check_threshold(threshold)


def check_choice_kernel(q, metric, partial):
    """The one combination the dose-choice kernels are not built for (csrc/causal_hmc_choice_api.hip; RESULT_KINDS["choice"].hole): a
    metric together with partially observed rows at more than 11 latent features, where that instantiation would need scratch
    memory.  ValueError."""
    hole = RESULT_KINDS["choice"].hole
    if metric and partial and int(q) > hole:
        raise ValueError("the dose choice is not available with a metric (mass='diag' / mass_scale) together with partial=True at more "
                         "than %d latent features (here %d): that kernel cannot be had without scratch memory and is not built; use "
                         "mass='identity', or fully observed rows" % (hole, int(q)))


def choice_finalize(best_count, best_ref, best_s1, mean, n_keep, maximize=True):
    """The sampler's per-row choice planes -> (prob_best [n, n_doses], expected_best [n], regret [n, n_doses]), float64 NumPy.
    best_count [n, n_doses] = the retained draws at which dose k was the row's best, (best_ref, best_s1) [n] the shifted sum of the
    best outcome (ref = that of draw 0, s1 = sum of best - ref), mean [n, n_doses] the posterior mean of every dose, n_keep the
    number of retained draws.  prob_best = best_count / n_keep; expected_best = ref + s1 / n_keep; regret_k = expected_best -
    mean_k (mean_k - expected_best when minimising): what is lost in expectation by giving dose k instead of the draw's best.
    It is not clipped: both terms are float32 sums, so a value may be negative by their rounding and by nothing else."""
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    count, ref, s1, mean = (np.asarray(to_np(a), np.float64) for a in (best_count, best_ref, best_s1, mean))
    m = int(n_keep)
    if m < 1:
        raise ValueError("choice_finalize: n_keep must be at least 1; got %r" % (n_keep,))
    if count.shape != mean.shape or count.ndim != 2 or ref.shape != (count.shape[0],) or s1.shape != ref.shape:
        raise ValueError("choice_finalize: best_count and mean [n, n_doses], best_ref and best_s1 [n]; got %r, %r, %r, %r" %
                         (count.shape, mean.shape, ref.shape, s1.shape))
    expected = ref + s1 / m
    regret = expected[:, None] - mean if maximize else mean - expected[:, None]
    return count / m, expected, regret


def group_dose_choice(choice, prob_best, groups):
    """Subgroup summaries of the choice: choice [n] (dose index per row), prob_best [n, n_doses] and int labels [n] ->
    {label: (share [n_doses], mean_prob [n_doses])}, float64: the share of the group's rows whose choice is dose k, and the mean
    over the group's rows of prob_best."""
    prob = np.asarray(prob_best, np.float64)
    choice = np.asarray(choice)
    labels = np.asarray(groups)
    if labels.shape != (prob.shape[0],) or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("groups must be integer labels of shape [n] = (%d,); got %s of shape %r" % (prob.shape[0], labels.dtype, labels.shape))
    out = {}
    for g in np.unique(labels):
        rows = labels == g
        m_g = int(rows.sum())
        out[int(g)] = (np.bincount(choice[rows].astype(np.int64), minlength=prob.shape[1])[:prob.shape[1]] / float(m_g),
                       prob[rows].sum(axis=0) / m_g)
    return out


# ---- predict_average: ATE / ATT / ATC and subgroup effects of a binary treatment (csrc/causal_hmc_gfx_kernels.h) ------------------
ESTIMANDS = ("ate", "att", "atc")
MAX_GROUPS = 32                   # 2 * MAX_GROUPS internal labels (group, arm): the 64 labels of bgm_causal_hmc_run_group_effects


def check_average(binary, estimand, groups, n):
    """The options of predict_average that are its own: a binary treatment, an estimand of ESTIMANDS, groups None or integer labels
    [n] with at most MAX_GROUPS distinct values; ValueError naming the option otherwise.
    -> (group_labels [n_groups] sorted distinct labels, or None without groups; group_index [n] int64 in [0, n_groups))."""
    if not binary:
        raise ValueError("predict_average is the average effect of a binary treatment (ATE / ATT / ATC); a continuous treatment has "
                         "its dose-response: predict's ADRF")
    if estimand not in ESTIMANDS:
        raise ValueError("estimand must be 'ate', 'att' or 'atc'; got %r" % (estimand,))
    if groups is None:
        return None, np.zeros(int(n), np.int64)
    labels = np.asarray(groups)
    if labels.shape != (int(n),) or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("groups must be integer labels of shape [n] = (%d,); got %s of shape %r" % (int(n), labels.dtype, labels.shape))
    distinct, index = np.unique(labels, return_inverse=True)
    if len(distinct) > MAX_GROUPS:
        raise ValueError("groups: at most %d distinct labels; got %d" % (MAX_GROUPS, len(distinct)))
    return distinct, index.reshape(-1).astype(np.int64)


def average_labels(group_index, x):
    """The row label of the kernels: 2 * group + arm, arm = 1 for a treated row (x_i = 1) -> int32 [n]"""
    arm = (np.asarray(x, np.float64).reshape(-1) > 0.5).astype(np.int64)
    return (2 * np.asarray(group_index, np.int64) + arm).astype(np.int32)


def average_counts(labels, n_groups):
    """Rows per (group, arm) -> float64 [n_groups, 2]"""
    return np.bincount(np.asarray(labels, np.int64), minlength=2 * int(n_groups)).astype(np.float64).reshape(int(n_groups), 2)


def combine_average_effects(sums, counts):
    """Per-draw label sums S[g, arm, d] of the individual treatment effect (arm 1 = the treated rows) and row counts n[g, arm] ->
    dict(ate, att, atc), each float64 [n_groups, n_draws]:
        ATE_g,d = (S_g0 + S_g1) / (n_g0 + n_g1),   ATT_g,d = S_g1 / n_g1,   ATC_g,d = S_g0 / n_g0.
    An estimand whose denominator is zero is nan for that group.  Sums and counts are additive over row shards: add the shards'
    arrays (an all-reduce) before calling."""
    S, cnt = np.asarray(sums, np.float64), np.asarray(counts, np.float64)
    if S.ndim != 3 or S.shape[1] != 2 or cnt.shape != S.shape[:2]:
        raise ValueError("combine_average_effects: sums [n_groups, 2, n_draws] and counts [n_groups, 2]; got %r and %r" % (S.shape, cnt.shape))

    def ratio(num, den):
        out = np.full(num.shape, np.nan)
        ok = den > 0
        out[ok] = num[ok] / den[ok][:, None]
        return out
    return dict(ate=ratio(S[:, 0] + S[:, 1], cnt[:, 0] + cnt[:, 1]), att=ratio(S[:, 1], cnt[:, 1]), atc=ratio(S[:, 0], cnt[:, 0]))


def average_summary(series, alpha):
    """Per-draw averages [n_groups, n_draws] -> (effect [n_groups], interval [n_groups, 2]): the mean over the draws and the
    alpha / 2 and 1 - alpha / 2 quantiles with linear interpolation between order statistics (NumPy's default, the rule of
    bgm_row_mean_quantiles that predict applies to the ADRF), in float64; nan rows stay nan."""
    series = np.asarray(series, np.float64)
    effect = np.full(series.shape[0], np.nan)
    bounds = np.full((series.shape[0], 2), np.nan)
    ok = ~np.isnan(series).any(axis=1)
    if ok.any():
        effect[ok] = series[ok].mean(axis=1)
        bounds[ok] = np.quantile(series[ok], [alpha / 2, 1 - alpha / 2], axis=1).T
    return effect, bounds


def check_average_estimand(estimand, effect, group_labels):
    """The estimand asked for must exist in every group; ValueError naming estimand and the groups without its rows otherwise."""
    bad = np.flatnonzero(np.isnan(np.asarray(effect, np.float64)))
    if len(bad):
        which = "the panel" if group_labels is None else "groups %r" % ([int(group_labels[i]) for i in bad],)
        raise ValueError("estimand=%r is undefined for %s: no %s rows to average over" %
                         (estimand, which, {"ate": "", "att": "treated", "atc": "control"}[estimand]))


# ---- predict_new / partial=True: rows whose outcome, or outcome and treatment, are not observed (csrc/causal_hmc_obs_kernels.h) -----
def check_partial_rows(x, y):
    """The observation pattern of partial=True is carried by NaN in x / y (NumPy arrays or torch tensors [n]).  A row may lack its
    outcome, or its outcome and its treatment; a row with y observed and x not has no defined target, because the outcome net f
    needs the treatment: ValueError naming the first such row."""
    bad = (x != x) & (y == y)
    if bool(bad.any()):
        row = int(bad.nonzero()[0].reshape(-1)[0])
        raise ValueError("partial=True: row %d has its outcome y observed and its treatment x not (NaN); the outcome term f(z, x) "
                         "needs the treatment -- drop y (NaN) or give x" % row)


def check_partial_panel(data_x, data_y, data_v):
    """partial=True of predict_dose_effect, before a device is touched -> (x [n], y [n], v [n, p]) float32 with NaN in x / y where
    a row does not observe them: the pattern rule of check_partial_rows and, as in check_new, no NaN among the covariates."""
    x, y = np.asarray(data_x, np.float32).reshape(-1), np.asarray(data_y, np.float32).reshape(-1)
    v = np.asarray(data_v, np.float32)
    if np.isnan(v).any():
        raise ValueError("partial=True: data_v holds NaN in row %d; missing covariates are not modelled (only the treatment and the "
                         "outcome may be unobserved)" % int(np.flatnonzero(np.isnan(v).reshape(len(v), -1).any(axis=1))[0]))
    check_partial_rows(x, y)
    return x, y, v


def check_new(binary, data_v, data_x, x_values, interval, draw_budget_bytes):
    """The options of predict_new that are its own, before a device is touched -> (v [n, p], x [n], y [n]) float32, x NaN where
    the treatment is not known (data_x None: everywhere) and y NaN everywhere.  ValueError for NaN in data_v (missing covariates
    are not modelled), for a continuous treatment without x_values, for a binary data_x with values other than 0, 1 or NaN, for a
    data_x whose length is not data_v's, for an interval that is neither 'normal' nor 'quantile', and for a draw budget that is
    not positive or, with a continuous treatment and interval='normal', has nothing to bound."""
    v = np.asarray(data_v, np.float32)
    if v.ndim != 2:
        raise ValueError("predict_new: data_v must be [n, p]; got shape %r" % (v.shape,))
    if np.isnan(v).any():
        raise ValueError("predict_new: data_v holds NaN in row %d; missing covariates are not modelled (only the treatment and the "
                         "outcome may be unobserved)" % int(np.flatnonzero(np.isnan(v).any(axis=1))[0]))
    n = v.shape[0]
    check_interval(interval)
    if binary and interval == "tails":
        raise ValueError("predict_new: interval='tails' belongs to the dose-response of a continuous treatment; a binary treatment goes "
                         "the ITE route (one value per row and draw): use interval='quantile'")
    if draw_budget_bytes is not None and int(draw_budget_bytes) <= 0:
        raise ValueError("draw_budget_bytes must be positive; got %r" % (draw_budget_bytes,))
    if not binary:
        if x_values is None:
            raise ValueError("predict_new needs x_values for a continuous treatment: the doses at which every row's outcome is evaluated")
        check_individual(False, x_values, interval, draw_budget_bytes)
    if data_x is None:
        x = np.full(n, np.nan, np.float32)
    else:
        x = np.asarray(data_x, np.float32).reshape(-1)
        if x.shape[0] != n:
            raise ValueError("predict_new: data_x has %d rows, data_v %d" % (x.shape[0], n))
        if binary and not np.all(np.isnan(x) | (x == 0.0) | (x == 1.0)):
            raise ValueError("predict_new: a binary treatment takes data_x in {0, 1} or NaN (not known); got %r in row %d" %
                             (float(x[~(np.isnan(x) | (x == 0.0) | (x == 1.0))][0]), int(np.flatnonzero(~(np.isnan(x) | (x == 0.0) | (x == 1.0)))[0])))
    return v, x, np.full(n, np.nan, np.float32)
