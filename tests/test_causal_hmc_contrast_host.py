"""predict_dose_effect / hmc_sample(row_contrasts=True) on the CPU: every refusal comes before a device is touched, the other classes
refuse the method with their HMC refusal, the entry point is declared, and the float32 shifted sums of a contrast series, restated
in NumPy, stay inside the two bounds that tests/test_gpu_causal_hmc_contrast.py applies to the kernel's planes
(tests/_causal_hmc_contrast_ref.py).  No device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bgm_impute_ref as IR  # noqa: E402
import _causal_hmc_contrast_ref as CR  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

DATA = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))


def _bare(cls, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def _error(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


def test_the_entry_point_is_declared():
    from bayesgm_amd import _lib
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    name = "bgm_causal_hmc_run_row_contrasts"
    assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
    tails, con = _lib.SYMBOLS["bgm_causal_hmc_run_row_tails"], _lib.SYMBOLS[name]
    # row_moments, + row_cmoments, contrast_draws, contrast_tails, k_tail, stream
    assert con[0] is C.c_int and con[1] == tails[1][:-4] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert "float *row_moments_dev, float *row_cmoments_dev,\n" in header
    assert "float *contrast_draws_dev, float *contrast_tails_dev, int32_t k_tail, void *stream);" in header
    assert "replaces: nothing in causalbgm/base.py" in header.split(name)[0].rsplit("/*", 1)[1]
    src = open(os.path.join(root, "bayesgm_amd", "csrc", "build.py")).read()
    assert '"causal_hmc_contrast_api.hip"' in src
    from bayesgm_amd.engine import CausalEngine
    assert callable(CausalEngine.hmc_run_rows_contrasts)


def test_hmc_sample_refuses_before_a_device_is_touched():
    """an engine without a handle or a device: anything past the option checks would raise AttributeError, not ValueError"""
    from bayesgm_amd.engine import CausalEngine
    eng = object.__new__(CausalEngine)
    eng.binary = False
    x, y, v = DATA
    run = (x, y, v, 5, 5, 0.1, 2, 7)
    assert "row_contrasts belongs to row_effects=True" in _error(eng.hmc_sample, *run, row_contrasts=True)
    for kw in (dict(max_trajectory=0.5), dict(jitter=True)):
        msg = _error(eng.hmc_sample, *run, row_effects=True, x_values=[0.0, 1.0], row_contrasts=True, **kw)
        assert "max_trajectory / jitter are not available with row_contrasts" in msg
    eng.binary = True
    msg = _error(eng.hmc_sample, *run, row_effects=True, x_values=[0.0, 1.0], row_contrasts=True)
    assert "binary" in msg and "EFFECT_ITE" in msg
    with pytest.raises(AttributeError):      # and with the option off the same call does go on to the device
        eng.hmc_sample(*run, row_effects=True, x_values=[0.0, 1.0])


def test_predict_dose_effect_refuses_before_a_device_is_touched():
    from bayesgm_amd.models.causalbgm import CausalBGM
    ok = _bare(CausalBGM)
    for bad in (None, float("nan"), float("inf"), [0.0], np.zeros(2), "a", True):
        assert "baseline must be a finite scalar" in _error(ok.predict_dose_effect, DATA, [1.0], bad)
    assert "predict_dose_effect needs x_values" in _error(ok.predict_dose_effect, DATA, None, 0.0)
    msg = _error(ok.predict_dose_effect, DATA, [1.0], 0.0, interval="hpd")
    assert "interval must be 'normal' or 'quantile'; got 'hpd'" in msg and "'tails'" in msg
    msg = _error(ok.predict_dose_effect, DATA, [1.0], 0.0, draw_budget_bytes=1 << 20)
    assert "interval='normal'" in msg and "draw_budget_bytes" in msg
    for interval in ("quantile", "tails"):
        assert "draw_budget_bytes must be positive" in _error(ok.predict_dose_effect, DATA, [1.0], 0.0, interval=interval, draw_budget_bytes=0)
    assert "groups must be integer labels" in _error(ok.predict_dose_effect, DATA, [1.0], 0.0, groups=np.zeros(3, np.int64))
    binary = _bare(CausalBGM)
    binary._p["binary_treatment"] = True
    msg = _error(binary.predict_dose_effect, DATA, [1.0], 0.0)
    assert "binary" in msg and "predict's ITE" in msg
    # partial=True: the pattern rules, on the host
    x, y, v = (a.copy() for a in DATA)
    x[2] = np.nan
    assert "row 2 has its outcome y observed and its treatment x not" in _error(ok.predict_dose_effect, (x, y, v), [1.0], 0.0, partial=True)
    v[1, 3] = np.nan
    assert "data_v holds NaN in row 1" in _error(ok.predict_dose_effect, (DATA[0], DATA[1], v), [1.0], 0.0, partial=True)
    # the method does not take the trajectory options
    with pytest.raises(TypeError):
        ok.predict_dose_effect(DATA, [1.0], 0.0, max_trajectory=1.0)
    # the refusals of the HMC sampler come first and stay word for word
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(mass="dense"), "mass must be"),
                     (dict(mass="diag", burn_in=10), "burn_in >= 20")):
        msg = _error(ok.predict_dose_effect, DATA, [1.0], 0.0, **kw)
        assert word in msg and msg == _error(ok.predict, DATA, x_values=[0.0], sampler="hmc", **kw)
    # the attributes of an earlier call do not survive a refused one
    ok.dose_effect_sd_ = ok.group_dose_effect_ = ok.dose_effect_curve_ = "stale"
    _error(ok.predict_dose_effect, DATA, [1.0], None)
    assert ok.dose_effect_sd_ is None and ok.group_dose_effect_ is None and ok.dose_effect_curve_ is None


def test_the_other_classes_refuse_the_method():
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    for cls, params, word in ((IdentifiableCausalBGM, dict(n_segments=3), "IdentifiableCausalBGM"),
                              (CausalBGMBayes, dict(), "not available for CausalBGMBayes"),
                              (IdentifiableCausalBGMBayes, dict(n_segments=3), "IdentifiableCausalBGMBayes")):
        m = _bare(cls, **params)
        want = _error(m.predict, DATA, x_values=[0.0], sampler="hmc")
        assert word in want and _error(m.predict_dose_effect, DATA, [1.0], 0.0) == want
        assert _error(m.predict_dose_effect, DATA, [1.0], 0.0, interval="tails", partial=True) == want
    bnn = _bare(CausalBGMBayes)
    bnn._p["use_bnn"] = True
    msg = _error(bnn.predict_dose_effect, DATA, [1.0], 0.0)
    assert "use_bnn" in msg and msg == _error(bnn.predict, DATA, x_values=[0.0], sampler="hmc")


def test_check_dose_effect_and_the_row_blocks():
    assert HM.check_dose_effect(False, [1.0], np.float32(0.5), "tails", None) == 0.5
    assert HM.check_dose_effect(False, [1.0], 2, "normal", None) == 2.0 and HM.check_dose_effect(False, 1.0, np.array(0.25), "quantile", 64) == 0.25
    # 20 doses and the baseline: the blocks of predict_individual at 21 doses
    shard = [(0, 2000000)]
    assert HM.individual_blocks(shard, 3000, 21, "normal") == shard
    assert HM.individual_blocks(shard, 3000, 21, "tails", k_tail=16)[0] == (0, (2 << 30) // (8 * 16 * 21) // 16 * 16)
    x, y, v = HM.check_partial_panel(np.array([[np.nan], [1.0]]), np.array([[np.nan], [np.nan]]), np.zeros((2, 3)))
    assert x.shape == y.shape == (2,) and x.dtype == y.dtype == v.dtype == np.float32 and np.isnan(x[0]) and x[1] == 1.0


@pytest.mark.parametrize("m", [20, 400])
def test_float32_shifted_sums_of_a_contrast_series_stay_inside_both_bounds(m):
    """the kernel's accumulation restated in NumPy float32 (tests/_bgm_impute_ref.py, moments_f32) on synthetic contrast series, the
    baseline's own column of exact zeros and a chain that repeats its values included, against float64 on the same float32 values"""
    rs = np.random.RandomState(100 + m)
    for ties in (False, True):
        c = CR.synthetic_contrasts(rs, 64, 6, m, ties)
        assert c.dtype == np.float32 and not c[:, 0].any() and c[:, 1:].any()
        ref, s1, s2 = IR.moments_f32(np.moveaxis(c, -1, 0))
        mean, sd = HM.row_moments_finalize(ref, s1, s2, m)
        assert not mean[:, 0].any() and not sd[:, 0].any()                    # dose 0: exactly zero, no NaN
        r_mean, r_var, inside = CR.worst_ratios(mean, sd, c)
        print("m = %d%s: worst |mean - ref| / bound %.3g, worst |var - ref| / bound %.3g, gamma_m %.3g" %
              (m, " ties" if ties else "", r_mean, r_var, IR.gamma(m)))
        assert inside
        # the bounds are not vacuous: sums that drop the last term are outside one of them somewhere
        ref_b, s1_b, s2_b = IR.moments_f32(np.moveaxis(c[..., :-1], -1, 0))
        mean_b, sd_b = HM.row_moments_finalize(ref_b, s1_b, s2_b, m)
        assert not CR.worst_ratios(mean_b, sd_b, c)[2]
