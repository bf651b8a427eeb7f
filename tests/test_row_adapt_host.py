"""The per-chain proposal scale of the MH sampler without a device: the factor table, the rule on the NumPy oracle
(tests/_row_adapt_ref.py) and the option checks of the class surface.

Bounds.  The adapted chains must accept within target +/- 0.05 in the retained phase: 0.05 is the reference's own `tolerance`
default for its block-wide rule (base.py:821).  The table identity up^target * dn^(1 - target) = 1 holds exactly before the rounding
to float32; each factor carries a relative rounding error <= 2^-24 and its logarithm is weighted by target resp. 1 - target, so the
product is within 2^-24 (target + 1 - target) = 2^-24 of 1, and 2^-23 leaves room for the float64 evaluation of the check itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _row_adapt_ref import (S_MAX, S_MIN, concentrated_model, concentrated_panel, random_panel,  # noqa: E402
                            row_adapt_sampler)
from bayesgm_amd import row_adapt as RA  # noqa: E402
from oracle import causal as OC  # noqa: E402

Z_DIMS, P, N, BURN, KEEP, TARGET = [3, 3, 3, 1], 50, 128, 1000, 1000, 0.25


@pytest.mark.parametrize("burn_in,target,kappa", [(1000, 0.25, 0.6), (5000, 0.25, 0.6), (37, 0.4, 0.75), (1, 0.1, 1.0), (0, 0.25, 0.6)])
def test_factor_table(burn_in, target, kappa):
    up, dn = RA.row_adapt_factors(burn_in, target, kappa)
    assert up.dtype == np.float32 and dn.dtype == np.float32 and up.shape == dn.shape == (burn_in,)
    assert np.all(up > 1) and np.all(dn < 1) and np.all(dn > 0)
    # stationary at the target: target * log up + (1 - target) * log dn = 0
    prod = up.astype(np.float64) ** target * dn.astype(np.float64) ** (1 - target)
    assert np.all(np.abs(prod - 1.0) <= 2.0 ** -23), np.abs(prod - 1.0).max()
    # monotone to 1
    assert np.all(np.diff(up) <= 0) and np.all(np.diff(dn) >= 0)
    if burn_in >= 1000:
        assert up[-1] - 1 < 0.02 and 1 - dn[-1] < 0.01
    # the first step is a whole unit of the log scale
    if burn_in:
        assert up[0] == np.float32(np.exp(1 - target)) and dn[0] == np.float32(np.exp(-target))
    assert np.float32(RA.S_MIN) == S_MIN and np.float32(RA.S_MAX) == S_MAX


def test_factor_table_arguments():
    for bad in (dict(burn_in=-1, target=0.25), dict(burn_in=10, target=0.0), dict(burn_in=10, target=1.0),
                dict(burn_in=10, target=0.25, kappa=0.5), dict(burn_in=10, target=0.25, kappa=1.5)):
        with pytest.raises(ValueError):
            RA.row_adapt_factors(**bad)


def _check_panel(m, data, what):
    up, dn = RA.row_adapt_factors(BURN, TARGET)
    fixed = row_adapt_sampler(m, data, BURN, KEEP, 1.0, 11, up[:0], dn[:0])
    adapt = row_adapt_sampler(m, data, BURN, KEEP, 1.0, 11, up, dn)
    assert np.all(fixed["scale"] == 1.0)
    rate_f, rate_a = fixed["acc"][BURN:].mean(), adapt["acc"][BURN:].mean()
    per_row = adapt["acc"][BURN:].mean(axis=0)
    const_f = (fixed["acc"][BURN:].sum(axis=0) == 0).mean()
    const_a = (adapt["acc"][BURN:].sum(axis=0) == 0).mean()
    s = adapt["scale"]
    print("%s: retained acceptance fixed %.4f, per row %.4f; per-row move rate q05 / median / q95 %.3f / %.3f / %.3f; final scale "
          "q05 / median / q95 %.4f / %.4f / %.4f; rows that never move: fixed %.3f, per row %.3f"
          % (what, rate_f, rate_a, *np.quantile(per_row, [0.05, 0.5, 0.95]), *np.quantile(s, [0.05, 0.5, 0.95]), const_f, const_a))
    assert abs(rate_a - TARGET) <= 0.05, rate_a
    # no constant series: every chain moved in the retained phase, i.e. every latent of every row takes more than one value
    assert const_a == 0.0
    assert np.all(np.ptp(adapt["draws"], axis=0) > 0)
    assert np.all(s > S_MIN) and np.all(s < S_MAX) and s.dtype == np.float32
    return rate_f, const_f, adapt


def test_rule_on_random_weights_panel():
    m = OC.init_model(0, Z_DIMS, P)
    rate_f, const_f, _ = _check_panel(m, random_panel(N, P, 1), "random weights, unrelated data")
    assert rate_f < TARGET - 0.05          # the fixed scale 1 is outside the band the rule reaches


def test_rule_on_concentrated_panel():
    m = concentrated_model(0, Z_DIMS, P)
    rate_f, const_f, _ = _check_panel(m, concentrated_panel(m, N, 1), "concentrated posterior")
    assert rate_f < 0.02 and const_f > 0.1          # fixed scale 1: hardly a move, and chains that never move


def test_scale_depends_on_the_row_alone():
    """rows [32, 64) sampled alone with row0 = 32 give the scales and draws of the same rows of the whole panel"""
    m = OC.init_model(2, Z_DIMS, P)
    x, y, v = random_panel(96, P, 3)
    up, dn = RA.row_adapt_factors(60, TARGET)
    full = row_adapt_sampler(m, (x, y, v), 60, 20, 0.7, 5, up, dn)
    part = row_adapt_sampler(m, (x[32:64], y[32:64], v[32:64]), 60, 20, 0.7, 5, up, dn, row0=32)
    assert np.array_equal(full["scale"][32:64], part["scale"]) and np.array_equal(full["draws"][:, 32:64], part["draws"])


def test_resolve_target_and_start_scale():
    assert RA.resolve_target(False) is None and RA.resolve_target(None) is None
    assert RA.resolve_target(True) == 0.25 and RA.resolve_target(np.bool_(True)) == 0.25 and RA.resolve_target(0.4) == 0.4
    for bad in (0.0, 1.0, -0.2, 1.5, "row", 2):
        with pytest.raises(ValueError, match="row_adapt"):
            RA.resolve_target(bad)
    assert RA.start_scale(0.3) == 0.3 and RA.start_scale(None) == 1.0 and RA.start_scale(-1.0, 0.5) == 0.5 and RA.start_scale(0, None) == 1.0


def _bare(cls, **params):
    """an instance without a device: the option checks run before anything touches the engine"""
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def test_class_surface_refuses_unsupported_combinations():
    from bayesgm_amd.models.causalbgm import CausalBGM
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    data = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))
    ok = _bare(CausalBGM)
    assert ok._row_adapt_target(False) is None and ok._row_adapt_target(True) == 0.25 and ok._row_adapt_target(0.3) == 0.3
    assert CausalBGM.mh_row_scale_ is None
    for bad in (0.0, 1.0, 7):
        with pytest.raises(ValueError, match="row_adapt"):
            ok.predict(data, x_values=[0.0], row_adapt=bad)
    # a call without row adaptation does not keep the scales of an earlier one (here it stops at its next argument check)
    ok.mh_row_scale_ = np.ones(4, np.float32)
    with pytest.raises(ValueError, match="x_values"):
        ok.predict(data)
    assert ok.mh_row_scale_ is None
    with pytest.raises(ValueError, match="adaptive_sd"):
        ok.metropolis_hastings_sampler(data, adaptive_sd="rows")
    with pytest.raises(ValueError, match="target"):
        ok.metropolis_hastings_sampler(data, adaptive_sd="row", target_acceptance_rate=1.2)
    for prec in ("bf16x3", "f16x3"):
        m = _bare(CausalBGM)
        m._p["mh_precision"] = prec
        with pytest.raises(ValueError, match="mh_precision"):
            m.predict(data, x_values=[0.0], row_adapt=True)
        with pytest.raises(ValueError, match="mh_precision"):
            m.metropolis_hastings_sampler(data, adaptive_sd="row")
    for cls, word in ((IdentifiableCausalBGM, "IdentifiableCausalBGM"), (IdentifiableCausalBGMBayes, "IdentifiableCausalBGM")):
        m = _bare(cls, n_segments=3)
        with pytest.raises(ValueError, match=word):
            m.predict(data, x_values=[0.0], row_adapt=True)
        with pytest.raises(ValueError, match=word):
            m.metropolis_hastings_sampler(data, adaptive_sd="row")
    m = _bare(CausalBGMBayes)
    m._p["use_bnn"] = True
    with pytest.raises(ValueError, match="use_bnn"):
        m.predict(data, x_values=[0.0], row_adapt=0.3)
    with pytest.raises(ValueError, match="use_bnn"):
        m.metropolis_hastings_sampler(data, adaptive_sd="row")


def test_abi_declares_the_setter():
    from bayesgm_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bgm_hip.h")).read()
    assert "bgm_causal_set_row_scale(bgm_handle *h, float *scale_dev, const float *up_dev, const float *dn_dev," in header
    assert len(_lib.SYMBOLS["bgm_causal_set_row_scale"][1]) == 7
