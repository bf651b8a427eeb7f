"""Chain diagnostics without a GPU: known answers of the float64 NumPy restatement (tests/_chain_diag_ref.py) that the GPU tests
compare the kernel with, the summary / warning path on host arrays, and the ABI of the two new entry points."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _chain_diag_ref import FLAG_CONSTANT, FLAG_NONFINITE, FLAG_TRUNCATED, ar1, chain_diag_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DRAWS = 3000
N_SERIES = 512


def _band(values, expected):
    """mean of `values` and the band expected +- 4 standard errors of that mean"""
    se = values.std(ddof=1) / np.sqrt(values.shape[0])
    print("mean %.1f, sd over series %.1f, standard error %.2f, expected %.1f" % (values.mean(), values.std(ddof=1), se, expected))
    return values.mean(), expected - 4 * se, expected + 4 * se


def test_iid_series_have_ess_near_the_number_of_draws():
    r = chain_diag_ref(ar1(np.random.RandomState(1), N_DRAWS, N_SERIES, 0.0))
    # measured at this seed: mean ESS 2935.4 (sd over the series 180.3, standard error 8.0): 2.2 % below the 3000 draws
    mean, lo, hi = _band(r["ess"], 2935.4)
    assert lo <= mean <= hi
    assert abs(mean / N_DRAWS - 1.0) < 0.03
    assert np.all(r["flags"] == 0)
    assert np.all(np.abs(r["rhat"] - 1.0) < 0.01)
    assert np.all(r["moves"] == N_DRAWS - 1)
    np.testing.assert_allclose(r["mcse"], r["sd"] / np.sqrt(r["ess"]), rtol=1e-15)


def test_ar1_series_have_ess_near_a_third_of_the_draws():
    r = chain_diag_ref(ar1(np.random.RandomState(2), N_DRAWS, N_SERIES, 0.5))
    # asymptotic ESS: n (1 - phi) / (1 + phi) = 1000; measured at this seed: mean 990.4 (sd over the series 89.1, s.e. 3.9)
    mean, lo, hi = _band(r["ess"], 990.4)
    assert lo <= mean <= hi
    assert abs(mean / (N_DRAWS / 3.0) - 1.0) < 0.05
    assert np.all(r["flags"] == 0)


def test_shifted_second_half_and_constant_series():
    rs = np.random.RandomState(3)
    x = ar1(rs, 1000, 4, 0.3)
    x[500:, 1] += 3.0                      # second half shifted by 3 sd
    x[:, 2] = 1.25                         # constant
    x[17, 3] = np.nan
    r = chain_diag_ref(x)
    assert r["rhat"][0] < 1.05
    assert r["rhat"][1] > 1.5
    assert r["flags"][2] == FLAG_CONSTANT and r["moves"][2] == 0 and r["sd"][2] == 0 and r["mean"][2] == 1.25
    assert np.isnan([r["rhat"][2], r["ess"][2], r["mcse"][2]]).all()
    assert r["flags"][3] == FLAG_NONFINITE
    assert np.isnan([r[k][3] for k in ("mean", "sd", "rhat", "ess", "mcse", "moves")]).all()
    assert r["flags"][0] == 0 and r["flags"][1] & FLAG_CONSTANT == 0


def test_truncation_flag_and_more_chains():
    rs = np.random.RandomState(4)
    x = ar1(rs, 400, 3, 0.99, n_chains=3)
    r4 = chain_diag_ref(x, max_lag=4)
    assert np.all(r4["flags"] == FLAG_TRUNCATED)          # phi = 0.99: the pairs are far from zero at lag 4
    r = chain_diag_ref(x, max_lag=1024)                   # clamped to 400 / 2 - 1
    assert np.all(r["ess"] < r4["ess"])
    sticky = np.repeat(ar1(rs, 50, 2, 0.0), 8, axis=0)    # every value held for 8 iterations
    rr = chain_diag_ref(sticky)
    assert np.all(rr["moves"] == 49)
    assert np.all(rr["ess"] < 400 / 4)


def test_summary_and_mixing_warning_on_host_arrays():
    from bayesgm_amd import diagnostics as dg
    rs = np.random.RandomState(5)
    good = chain_diag_ref(ar1(rs, 3000, 40, 0.3))
    sticky = chain_diag_ref(np.repeat(ar1(rs, 60, 40, 0.0), 50, axis=0))         # about 60 moves in 3000 draws

    def as_diag(r):
        f = {k: r[k].reshape(-1, 4) for k in dg.ChainDiagnostics.FIELDS}
        return dg.ChainDiagnostics(flags=r["flags"].reshape(-1, 4), n_chains=1, n_draws=3000, max_lag=256, **f)
    s = as_diag(good).summary()
    assert s["share_flagged"] == 0.0 and s["share_constant"] == 0.0 and s["ess_min"] > 100 and s["rhat_max"] < 1.01
    assert s["ess_min"] <= s["ess_q01"] <= s["ess_median"] and s["rhat_q99"] <= s["rhat_max"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert dg.warn_if_not_mixed(as_diag(good), {}) is False
        assert dg.warn_if_not_mixed(as_diag(sticky), {"mixing_check": False}) is False
    assert as_diag(sticky).summary()["share_ess_below"] > 0.5
    with pytest.warns(dg.MixingWarning, match="effective"):
        assert dg.warn_if_not_mixed(as_diag(sticky), {}) is True
    assert issubclass(dg.MixingWarning, RuntimeWarning)


def test_chain_diagnostics_rejects_wrong_shapes():
    from bayesgm_amd.diagnostics import chain_diagnostics
    for bad in (np.zeros((10, 3)), np.zeros((4, 5, 2)), np.zeros((9, 100, 4, 2)), np.zeros((2, 3, 4, 5, 6)), []):
        with pytest.raises(ValueError):
            chain_diagnostics(bad)
    with pytest.raises(ValueError):
        chain_diagnostics(np.zeros((100, 5, 2)), max_lag=2000)
    with pytest.raises(ValueError):
        chain_diagnostics([np.zeros((100, 5, 2)), np.zeros((100, 6, 2))])


def test_entry_points_are_bound_declared_and_exported():
    from bayesgm_amd import _lib
    names = ("bgm_chain_diagnostics", "bgm_chain_diagnostics_workspace")
    src = open(os.path.join(ROOT, "include", "bgm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(bgm_[a-z_0-9]+)\s*\(", src))
    lib = _lib.load()
    for n in names:
        assert n in _lib.SYMBOLS, "ctypes binding misses " + n
        assert n in declared, "include/bgm_hip.h does not declare " + n
        assert hasattr(lib, n), "libbgm_hip.so does not export " + n
    assert len(_lib.SYMBOLS["bgm_chain_diagnostics"][1]) == 11
    assert len(_lib.SYMBOLS["bgm_chain_diagnostics_workspace"][1]) == 6
