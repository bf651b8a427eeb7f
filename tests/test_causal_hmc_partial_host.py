"""Partially observed rows (predict_new, partial=True) on the CPU: the refusals of the class surface and of the engine-level
pattern check, the three classes without the HMC sampler, the masks of the NumPy restatement (a missing term contributes exactly 0
to value and gradient) and the share condition the GPU chain test rests on.  No device is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_ref as REF  # noqa: E402
import _causal_partial_ref as PR  # noqa: E402
from oracle import causal as OC  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402
from bayesgm_amd.row_adapt import row_adapt_factors  # noqa: E402

V = np.zeros((4, 5), np.float32)
NAN = float("nan")
# the inputs of tests/test_gpu_causal_hmc_partial.py::test_chains_match_the_float32_restatement
CHAIN_CASES = [dict(z_dims=[1, 1, 1, 7], p=20, binary=False), dict(z_dims=[3, 3, 6, 6], p=20, binary=True)]
CHAIN_BURN_MASS = 20              # the shortest burn-in with an estimation window (causal_hmc.MASS_MIN_BURN_IN)
CHAIN_N, CHAIN_BURN, CHAIN_KEEP, CHAIN_L, CHAIN_STEP0, CHAIN_SEED, TARGET = 113, 10, 10, 3, 0.1, 1234567890123, 0.75


def chain_inputs(case):
    """(model, (x, y, v)) of a chain case: the model and the panel of tests/test_gpu_causal.py's helpers (restated here, so that this
    module needs no GPU test module), with the three patterns mixed inside every tile"""
    m = OC.init_model(21, case["z_dims"], case["p"], binary_treatment=case["binary"])
    rs = np.random.RandomState(21 + 99)
    for k in ("g", "f", "h", "e"):
        m[k] = [(W.astype(np.float32), (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W, b in m[k]]
    rs = np.random.RandomState(22)
    v = rs.randn(CHAIN_N, case["p"]).astype(np.float32)
    x = rs.exponential(size=(CHAIN_N, 1)).astype(np.float32)
    if case["binary"]:
        x = (x > np.median(x)).astype(np.float32)
    y = (x + rs.randn(CHAIN_N, 1)).astype(np.float32)
    x, y = PR.mixed_panel(x, y, 23)
    return m, (x, y, v)


def _bare(cls, binary=False, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=binary, **params)
    obj.params = obj._p
    return obj


def _error(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


def test_predict_new_refusals():
    from bayesgm_amd.models.causalbgm import CausalBGM
    cont, binr = _bare(CausalBGM), _bare(CausalBGM, True)
    bad_v = V.copy()
    bad_v[2, 1] = NAN
    msg = _error(cont.predict_new, bad_v, x_values=[0.0])
    assert "data_v holds NaN in row 2" in msg and "missing covariates" in msg
    assert "data_v holds NaN" in _error(binr.predict_new, bad_v)
    assert "x_values" in _error(cont.predict_new, V) and "x_values" in _error(cont.predict_new, V, np.zeros(4))
    msg = _error(binr.predict_new, V, [0.0, 1.0, 0.5, NAN])
    assert "0, 1" in msg and "0.5" in msg and "row 2" in msg
    assert "data_x has 3 rows" in _error(binr.predict_new, V, [0.0, 1.0, NAN])
    assert "interval must be 'normal' or 'quantile'" in _error(cont.predict_new, V, x_values=[0.0], interval="hpd")
    assert "draw_budget_bytes must be positive" in _error(binr.predict_new, V, draw_budget_bytes=0)
    msg = _error(cont.predict_new, V, x_values=[0.0], draw_budget_bytes=1 << 20)
    assert "interval='normal'" in msg and "draw_budget_bytes" in msg
    # every refusal of the HMC sampler, through the same calls as predict(sampler='hmc'): word for word, before the method's own
    data = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), V)
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(mass="dense"), "mass must be"),
                     (dict(mass="diag", burn_in=10), "burn_in >= 20")):
        msg = _error(cont.predict_new, bad_v, **kw)
        assert word in msg and msg == _error(cont.predict, data, x_values=[0.0], sampler="hmc", **kw)
    split = _bare(CausalBGM)
    split._p["mh_precision"] = "f16x3"
    assert "mh_precision" in _error(split.predict_new, V, x_values=[0.0])
    # what passes the checks: x NaN where the treatment is not known, y NaN everywhere
    v, x, y = HM.check_new(True, V, [0.0, 1.0, NAN, 1.0], None, "normal", None)
    assert v.dtype == x.dtype == y.dtype == np.float32 and np.isnan(y).all() and np.array_equal(np.isnan(x), [False, False, True, False])
    v, x, y = HM.check_new(False, V, None, [0.5], "quantile", 1 << 20)
    assert np.isnan(x).all() and np.isnan(y).all() and x.shape == y.shape == (4,)


def test_a_row_with_its_outcome_and_without_its_treatment_is_refused():
    import torch
    x = np.array([0.3, NAN, NAN, 1.0], np.float32)
    y = np.array([0.1, NAN, 0.7, NAN], np.float32)
    for a, b in ((x, y), (torch.from_numpy(x), torch.from_numpy(y))):
        with pytest.raises(ValueError, match=r"row 2 has its outcome y observed and its treatment x not"):
            HM.check_partial_rows(a, b)
        HM.check_partial_rows(a[[0, 1, 3]], b[[0, 1, 3]])          # all observed, both missing, y missing: fine
    from bayesgm_amd.models.causalbgm import CausalBGM
    msg = _error(_bare(CausalBGM).hmc_sampler, (x, y, V), partial=True)
    assert "row 2" in msg and "treatment" in msg
    from bayesgm_amd.engine import CausalEngine
    import inspect
    for name in ("logpost_grad", "hmc_run", "hmc_sample", "hmc_run_rows_effects"):
        assert inspect.signature(getattr(CausalEngine, name)).parameters["partial"].default is False, name
    assert inspect.signature(CausalBGM.hmc_sampler).parameters["partial"].default is False


def test_the_other_classes_refuse_predict_new_by_name():
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    for cls, params in ((IdentifiableCausalBGM, dict(n_segments=3)), (IdentifiableCausalBGMBayes, dict(n_segments=3)), (CausalBGMBayes, dict())):
        msg = _error(_bare(cls, **params).predict_new, V, x_values=[0.0])
        assert "predict_new is not available for %s" % cls.__name__ in msg and "HMC" in msg
        assert msg == _error(_bare(cls, True, **params).predict_new, V, [0.0, 1.0, NAN, 1.0])


def test_abi_declares_the_entry_point():
    from bayesgm_amd import _lib
    import ctypes as C
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    name = "bgm_causal_hmc_set_partial"
    assert "BGM_API int %s(bgm_handle *h, int32_t on);" % name in header
    assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_int32])
    assert '"causal_hmc_obs_api.hip"' in open(os.path.join(root, "bayesgm_amd", "csrc", "build.py")).read()
    assert name in open(os.path.join(root, "ABI_MAP.md")).read()


@pytest.mark.parametrize("case", CHAIN_CASES)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_missing_term_contributes_exactly_zero(case, dt):
    m, (x, y, v) = chain_inputs(case)
    z = np.random.RandomState(3).randn(CHAIN_N, sum(case["z_dims"])).astype(dt)
    has_x, has_y = PR.patterns(x, y)
    assert has_y.sum() > 20 and (has_x & ~has_y).sum() > 20 and (~has_x).sum() > 20 and not np.any(has_y & ~has_x)
    T = PR.log_posterior_terms(m, x, y, v, z)
    for key, has in (("x", has_x), ("y", has_y)):
        nll, dz = T[key]
        assert nll.dtype == dz.dtype == dt
        assert np.all(nll[~has] == 0) and np.all(dz[~has] == 0), key
        assert np.all(np.abs(dz[has]).max(axis=1) > 0) and np.all(np.isfinite(nll)) and np.all(np.isfinite(dz)), key
    lp, gr = PR.log_posterior_and_grad(m, x, y, v, z)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(gr))
    # the observed rows are those of the restatement without masks, bit for bit; so is a fully observed panel
    xf, yf = np.where(np.isnan(x), 0.25, x).astype(np.float32), np.where(np.isnan(y), -0.5, y).astype(np.float32)
    lp0, gr0 = REF.log_posterior_and_grad(m, xf, yf, v, z)
    assert np.array_equal(lp[has_y], lp0[has_y]) and np.array_equal(gr[has_y], gr0[has_y])
    lp1, gr1 = PR.log_posterior_and_grad(m, xf, yf, v, z)
    assert np.array_equal(lp1, lp0) and np.array_equal(gr1, gr0)
    # leaving a term out is the analytic statement: log p(z | x, v) = log p(z | x, y, v) + nll_y, and so for the gradient (float64)
    if dt is np.float64:
        sel = has_x & ~has_y
        nll_y, dz_y = PR.log_posterior_terms(m, xf, yf, v, z)["y"]
        assert np.allclose(lp[sel], lp0[sel] + nll_y[sel], rtol=1e-12, atol=1e-12)
        assert np.allclose(gr[sel], gr0[sel] + dz_y[sel], rtol=1e-10, atol=1e-12)


def chain_runs(case, mass, dt=np.float32):
    """the restatement's run of a chain case in dtype dt, with the estimated metric (mass='diag': CHAIN_BURN_MASS iterations of
    burn-in, the windows of causal_hmc.mass_windows) or without"""
    m, data = chain_inputs(case)
    m, data = OC.cast_model(m, dt), tuple(t.astype(dt) for t in data)
    if mass:
        (start, ends), (up, dn) = HM.mass_schedule(CHAIN_BURN_MASS, TARGET)
        return PR.hmc_mass_sampler(m, data, CHAIN_BURN_MASS, CHAIN_KEEP, CHAIN_STEP0, CHAIN_L, CHAIN_SEED, up, dn, windows=(start, ends))
    up, dn = row_adapt_factors(CHAIN_BURN, TARGET)
    return PR.hmc_sampler(m, data, CHAIN_BURN, CHAIN_KEEP, CHAIN_STEP0, CHAIN_L, CHAIN_SEED, up, dn)


@pytest.mark.parametrize("mass", [False, True], ids=["identity", "diag"])
@pytest.mark.parametrize("case", CHAIN_CASES)
def test_float32_restatement_keeps_the_share_against_its_float64_twin(case, mass):
    """The GPU chain test asks for >= 97 % of the rows within 1e-4 of the float32 restatement; that bar rests on the float32
    restatement itself staying with its float64 twin on >= 98.5 % of the rows of the same inputs (tests/test_gpu_causal_hmc.py)."""
    a, b = chain_runs(case, mass), chain_runs(case, mass, np.float64)
    assert a["draws"].dtype == np.float32 and b["draws"].dtype == np.float64
    row_ok = np.all(np.abs(a["draws"][-1] - b["draws"][-1]) <= 1e-4, axis=1)
    print("float32 restatement rows equal to the float64 one: %.4f; acceptance %.3f" % (row_ok.mean(), a["acc"].mean()))
    assert row_ok.mean() >= 0.985
    assert 0.2 < a["acc"].mean() < 1.0 and np.ptp(a["step"]) > 0
    assert np.all(np.isfinite(a["draws"])) and np.array_equal(a["step"][row_ok], b["step"][row_ok])
