"""Run-time diagnostics: the second optimum of the EGM warm start of CausalBGM.fit, and the mixing of the latent MCMC chains
(`chain_diagnostics`: split R-hat and effective sample size per sampled latent, computed on the GPU; `MixingWarning`).

Sixteen end-to-end runs of the published tutorial setting (eight of the product, eight of the NumPy oracle: DESIGN_HISTORY.md section 2c,
profiles/r03_accuracy/, profiles/r03_oracle_anchor/) end in one of two places.  Eleven land where the reference's published run
landed: late `l2_loss_z` 0.22 - 0.25 (published 0.247), panel `MSE_v` 0.964 - 0.976, MH acceptance 0.097 - 0.101.  Five land in a
second optimum of the warm start -- late `l2_loss_z` 0.35 - 0.44, `MSE_v` 0.975 - 0.999 at EVERY evaluation, acceptance 0.11 - 0.12
-- in which the dose-response curve can be anything (ADRF RMSE 0.016 - 0.030 for four of them, 0.53 for product seed 99: a curve
shifted by +0.65).  Both statistics are printed by `fit` (the reference prints the same lines); this module turns them into ONE
`warnings.warn` so that a run of the drop-in does not return such a curve silently.  The reference itself gives no warning.
"""
import warnings

import numpy as np

MIN_EGM_ITER = 10000        # warm starts shorter than this are not diagnosed (the sixteen runs used the reference's 30 000)
L2Z_LATE_MAX = 0.33     # median l2_loss_z of the EGM log lines of the last third of the warm start: main optimum <= 0.253, second >= 0.351
MSE_V_MAX = 0.975       # panel MSE_v of a fit evaluation (standardised V): second optimum >= 0.9753 at every evaluation


class SecondOptimumWarning(RuntimeWarning):
    pass


def late_l2_loss_z(iters, values, n_iter):
    """Median of the logged l2_loss_z over the last third of the warm start (iterations >= 2/3 n_iter); nan without such lines."""
    it = np.asarray(iters, float)
    v = np.asarray(values, float)
    sel = it >= (2.0 / 3.0) * float(n_iter)
    return float(np.median(v[sel])) if sel.any() else float("nan")


def second_optimum_message(l2z_late, mse_v, v_var=1.0):
    """The warning text when BOTH symptoms are present, else None.  `v_var`: mean per-column variance of the panel's V -- the threshold
    on MSE_v was calibrated on standardised covariates (variance 1), so the statistic compared is MSE_v / v_var, the fraction of V's
    variance the generator leaves unexplained; a panel whose V carries no usable variance (v_var <= 0) is not diagnosed."""
    if l2z_late is None or not np.isfinite(l2z_late) or mse_v is None or not np.isfinite(mse_v):
        return None
    if v_var is None or not np.isfinite(v_var) or v_var <= 0:
        return None
    mse_v = mse_v / v_var
    if l2z_late > L2Z_LATE_MAX and mse_v > MSE_V_MAX:
        return ("CausalBGM.fit: the EGM warm start may have ended in its second optimum (late l2_loss_z %.3f > %.2f and panel "
                "MSE_v / var(V) %.4f > %.3f; thresholds calibrated on sixteen runs of the reference's Hirano-Imbens tutorial, where runs "
                "that reproduce the published trace show l2_loss_z <= 0.25 and MSE_v <= 0.976 -- on data with weakly informative "
                "covariates a high MSE_v alone is normal).  On the tutorial data the estimated dose-response curve / treatment effects "
                "were unreliable in this state (one of five such runs returned an ADRF shifted by +0.65).  Remedy: re-run with another "
                "random_seed (or a longer egm_n_iter) and compare the same two log lines; params['second_optimum_check'] = False "
                "silences this check." % (l2z_late, L2Z_LATE_MAX, mse_v, MSE_V_MAX))
    return None


def warn_if_second_optimum(l2z_late, mse_v, already=False, v_var=1.0):
    """Emit the warning once; returns True when it was (or had been) emitted."""
    if already:
        return True
    msg = second_optimum_message(l2z_late, mse_v, v_var)
    if msg is None:
        return False
    warnings.warn(msg, SecondOptimumWarning, stacklevel=3)
    return True


_NOTICED = set()


def notice_once(key, message):
    """One line on stderr, once per process: a default of this build that differs from the reference as written was taken implicitly."""
    import sys
    if key in _NOTICED:
        return
    _NOTICED.add(key)
    print("bayesgm_amd: " + message, file=sys.stderr)


# ---------------------------------------------------------------------------------------------------------------------
# MCMC chain diagnostics (bgm_chain_diagnostics, csrc/chain_diag_kernels.h)
# ---------------------------------------------------------------------------------------------------------------------
# Conventions, not calibrated on this model: Stan and ArviZ flag a quantity whose split R-hat exceeds 1.01 or whose effective
# sample size is below 100 per chain; a run is reported when more than MIXING_MAX_SHARE of its non-constant series are flagged.
RHAT_MAX = 1.01
ESS_MIN = 100.0
MIXING_MAX_SHARE = 0.01

FLAG_CONSTANT, FLAG_TRUNCATED, FLAG_NONFINITE = 1, 2, 4
MAX_LAG_LIMIT = 1024         # limits of the kernel
MAX_CHAINS = 8
MIN_DRAWS = 8
_UPLOAD_BYTES = 1 << 30      # host input: rows are uploaded in blocks of at most this many bytes of draws


class MixingWarning(RuntimeWarning):
    pass


class ChainDiagnostics(object):
    """Per-series statistics of MCMC draws, NumPy arrays of shape (n, q): `mean`, `sd`, `rhat` (split R-hat), `ess`, `mcse`
    (sd / sqrt(ess)), `moves` (number of t with x[t] != x[t-1], over all chains) and `flags` (int32; bit 0: constant series,
    bit 1: the autocorrelation sum was truncated at max_lag -- the ESS is an upper bound, bit 2: a non-finite draw).  `rows`: the
    row indices of the panel the n rows stand for (set by `CausalBGM.predict(diagnose_rows=...)`), else None."""

    FIELDS = ("mean", "sd", "rhat", "ess", "mcse", "moves")

    def __init__(self, mean, sd, rhat, ess, mcse, moves, flags, n_chains, n_draws, max_lag, rows=None):
        self.mean, self.sd, self.rhat, self.ess, self.mcse, self.moves, self.flags = mean, sd, rhat, ess, mcse, moves, flags
        self.n_chains, self.n_draws, self.max_lag, self.rows = n_chains, n_draws, max_lag, rows

    def summary(self):
        """Small dict over all series: minimum and 1 % / 50 % quantiles of the ESS and maximum / 99 % quantile of R-hat over the
        non-constant finite series, and the shares of constant, truncated, `rhat > RHAT_MAX` and `ess < ESS_MIN` series (the
        last two among the non-constant ones; `share_flagged`: either)."""
        flags = self.flags.reshape(-1)
        total = max(1, flags.shape[0])
        live = (flags & (FLAG_CONSTANT | FLAG_NONFINITE)) == 0
        ess, rhat = self.ess.reshape(-1)[live], self.rhat.reshape(-1)[live]
        k = max(1, ess.shape[0])
        nan = float("nan")
        some = ess.shape[0] > 0
        bad_rhat, bad_ess = rhat > RHAT_MAX, ess < ESS_MIN
        return dict(
            n_series=int(flags.shape[0]), n_chains=int(self.n_chains), n_draws=int(self.n_draws),
            ess_min=float(ess.min()) if some else nan, ess_q01=float(np.quantile(ess, 0.01)) if some else nan,
            ess_median=float(np.median(ess)) if some else nan,
            rhat_max=float(rhat.max()) if some else nan, rhat_q99=float(np.quantile(rhat, 0.99)) if some else nan,
            share_constant=float(((flags & FLAG_CONSTANT) != 0).sum()) / total,
            share_truncated=float(((flags & FLAG_TRUNCATED) != 0).sum()) / total,
            share_nonfinite=float(((flags & FLAG_NONFINITE) != 0).sum()) / total,
            share_rhat_above=float(bad_rhat.sum()) / k, share_ess_below=float(bad_ess.sum()) / k,
            share_flagged=float((bad_rhat | bad_ess).sum()) / k)


def mixing_message(summary, where="MCMC"):
    """The warning text when more than MIXING_MAX_SHARE of the non-constant series miss a threshold, else None."""
    if not (summary["share_flagged"] > MIXING_MAX_SHARE):
        return None
    return ("%s: %.1f %% of the %d sampled series have not mixed by the usual conventions (split R-hat > %.2f: %.1f %%, effective "
            "sample size < %.0f: %.1f %%; ESS min %.1f, 1 %% quantile %.1f, median %.1f of %d draws; R-hat max %.3f; constant series "
            "%.1f %%).  Posterior intervals read the tails of these chains.  Remedies: a smaller q_sd or the adaptive scale, more "
            "iterations; params['mixing_check'] = False silences this check."
            % (where, 100 * summary["share_flagged"], summary["n_series"], RHAT_MAX, 100 * summary["share_rhat_above"], ESS_MIN,
               100 * summary["share_ess_below"], summary["ess_min"], summary["ess_q01"], summary["ess_median"],
               summary["n_chains"] * summary["n_draws"], summary["rhat_max"], 100 * summary["share_constant"]))


def warn_if_not_mixed(diag, params=None, where="MCMC"):
    """One MixingWarning when `diag.summary()` misses the thresholds, unless params['mixing_check'] is False; True when emitted."""
    if params is not None and not params.get("mixing_check", True):
        return False
    msg = mixing_message(diag.summary(), where)
    if msg is None:
        return False
    warnings.warn(msg, MixingWarning, stacklevel=3)
    return True


def _diag_device(lib, h, t, n_chains, n_draws, n_series, max_lag):
    """(out [6, n_series] float64, flags [n_series] int32) device tensors of one bgm_chain_diagnostics call on the contiguous
    float32 device tensor t."""
    import ctypes as C

    import torch
    from . import _lib
    dev = t.device
    ws_bytes = C.c_int64()
    _lib.check(lib.bgm_chain_diagnostics_workspace(h, n_chains, n_draws, n_series, max_lag, C.byref(ws_bytes)),
               "bgm_chain_diagnostics_workspace")
    ws = torch.empty(max(1, (ws_bytes.value + 7) // 8), dtype=torch.float64, device=dev)
    out = torch.empty((6, n_series), dtype=torch.float64, device=dev)
    flags = torch.empty(n_series, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.bgm_chain_diagnostics(h, C.c_void_p(t.data_ptr()), n_chains, n_draws, n_series, max_lag, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(flags.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel() * 8, stream),
               "bgm_chain_diagnostics")
    return out, flags


def chain_diagnostics(draws, max_lag=256, device=None):
    """Split R-hat and effective sample size of every sampled latent: the Stan / ArviZ "mean" forms without rank normalisation
    (definitions: include/bgm_hip.h, bgm_chain_diagnostics), float64 sums over the float32 draws in one GPU pass.

    draws: NumPy array or torch tensor of shape (n_keep, n, q) -- what `metropolis_hastings_sampler` / `tfp_mcmc_sampler`
    return -- or (n_chains, n_keep, n, q) for independent runs of the same rows; also a list of (n_keep, n, q) arrays, which is
    stacked.  Device tensors are used in place; host arrays are uploaded in row blocks, so an input larger than the free device
    memory works.  max_lag: the largest autocorrelation lag summed (1 .. 1024, clamped to n_keep / 2 - 1).  Returns a
    `ChainDiagnostics`.  Runs on the current HIP device (or `device`); there is no CPU path."""
    import torch
    from . import _lib
    from .latent_dims import _handle
    if isinstance(draws, (list, tuple)):
        if len(draws) == 0:
            raise ValueError("chain_diagnostics: empty list of draws")
        if any(tuple(d.shape) != tuple(draws[0].shape) or len(d.shape) != 3 for d in draws):
            raise ValueError("chain_diagnostics: a list of draws must hold arrays of one shape (n_keep, n, q)")
        draws = torch.stack(list(draws)) if isinstance(draws[0], torch.Tensor) else np.stack([np.asarray(d) for d in draws])
    elif not isinstance(draws, torch.Tensor):
        draws = np.asarray(draws)
    if draws.ndim == 3:
        draws = draws[None]
    if draws.ndim != 4:
        raise ValueError("chain_diagnostics: draws must have shape (n_keep, n, q) or (n_chains, n_keep, n, q), got %s" % (tuple(draws.shape),))
    n_chains, n_draws, n, q = (int(k) for k in draws.shape)
    if n_draws < MIN_DRAWS:
        raise ValueError("chain_diagnostics: %d draws per chain, at least %d are needed" % (n_draws, MIN_DRAWS))
    if not 1 <= n_chains <= MAX_CHAINS:
        raise ValueError("chain_diagnostics: %d chains, 1 .. %d are supported" % (n_chains, MAX_CHAINS))
    max_lag = int(max_lag)
    if not 1 <= max_lag <= MAX_LAG_LIMIT:
        raise ValueError("chain_diagnostics: max_lag = %d outside 1 .. %d" % (max_lag, MAX_LAG_LIMIT))
    if n < 1 or q < 1:
        raise ValueError("chain_diagnostics: draws of shape %s hold no series" % (tuple(draws.shape),))
    if not torch.cuda.is_available():
        raise RuntimeError("bayesgm_amd: chain_diagnostics runs on a HIP device; none is available (there is no CPU path)")
    on_device = isinstance(draws, torch.Tensor) and draws.is_cuda
    if on_device:
        dev = draws.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    h = _handle(dev.index if dev.index is not None else torch.cuda.current_device())
    with torch.cuda.device(dev):
        if on_device:
            t = draws.to(torch.float32).contiguous()
            out, flags = _diag_device(lib, h, t, n_chains, n_draws, n * q, max_lag)
            out, flags = out.cpu().numpy(), flags.cpu().numpy()
        else:
            host = draws if isinstance(draws, torch.Tensor) else torch.from_numpy(draws)
            rows = max(1, min(n, _UPLOAD_BYTES // max(1, 4 * n_chains * n_draws * q)))
            outs, fl = [], []
            for r0 in range(0, n, rows):
                t = host[:, :, r0:r0 + rows, :].to(torch.float32).contiguous().to(dev)
                o, f = _diag_device(lib, h, t, n_chains, n_draws, t.shape[2] * q, max_lag)
                outs.append(o.cpu().numpy())
                fl.append(f.cpu().numpy())
            out, flags = np.concatenate(outs, axis=1), np.concatenate(fl)
    fields = [out[i].reshape(n, q) for i in range(6)]
    return ChainDiagnostics(*fields, flags=flags.reshape(n, q), n_chains=n_chains, n_draws=n_draws,
                            max_lag=min(max_lag, n_draws // 2 - 1))
