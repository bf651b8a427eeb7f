"""The imputation inside the BGM sampler (BGM.predict(fused_predict=True), bgm_bgm_hmc_run_rows_impute), host side: the refusals that
come before any device work, the binding, and the proof on the CPU that the GPU test's inputs stay inside the two bounds of
tests/_bgm_impute_ref.py -- the float32 restatement of the kernel's sequential sums over float32 predictive values of the chains of
the NumPy sampler, against float64 on the same latents.  No measured tolerance enters.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bgm_impute_ref as IR  # noqa: E402
from _bgm_traj_ref import hmc_sampler  # noqa: E402

from oracle import bgm as OB  # noqa: E402


def _model(seed, q, p, n_hidden):      # (test_gpu_bgm._model; that module cannot be imported without the built library)
    m = OB.init_model(seed, q, p, g_units=(64,) * n_hidden)
    rs = np.random.RandomState(seed + 7)
    g = m["g"]
    g["bn"].update(gamma=(1 + 0.1 * rs.randn(q)).astype(np.float32), beta=(0.1 * rs.randn(q)).astype(np.float32),
                   mean=(0.2 * rs.randn(q)).astype(np.float32), var=(0.5 + rs.rand(q)).astype(np.float32))
    g["trunk"] = [(W, (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W, b in g["trunk"]]
    g["mean"] = (g["mean"][0], (0.1 * rs.randn(p)).astype(np.float32))
    g["var"] = (g["var"][0], (0.1 * rs.randn(p)).astype(np.float32))
    return m


def _data(n, p, seed, miss):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, p).astype(np.float32)
    x[rs.rand(n, p) < miss] = np.nan
    x[0, :] = np.nan
    if n > 1:
        x[1, :] = rs.randn(p)
    return x


def test_the_four_refusals_name_the_option_before_any_device_work():
    from bayesgm_amd.models.bgm import BGM
    from bayesgm_amd.models.bgm_bnn import BGMBayes
    x = np.zeros((4, 5), np.float32)
    model = object.__new__(BGM)               # no engine, no device: the refusal comes before either is touched
    model.params = dict(hmc_precision="fp32")
    with pytest.raises(ValueError, match="fused_predict.*row_adapt"):
        model.predict(x, fused_predict=True)
    with pytest.raises(ValueError, match="fused_predict.*return_samples"):
        model.predict(x, row_adapt=True, fused_predict=True, return_samples=True)
    model.params = dict(hmc_precision="f16x3")
    with pytest.raises(ValueError, match="fused_predict.*hmc_precision"):
        model.predict(x, row_adapt=True, fused_predict=True)
    with pytest.raises(ValueError, match="fused_predict"):
        model.predict(x, row_adapt=True, fused_predict="yes")
    bayes = object.__new__(BGMBayes)
    with pytest.raises(ValueError, match="fused_predict.*use_bnn"):
        bayes.predict(x, fused_predict=True)
    with pytest.raises(ValueError, match="use_bnn"):      # (and row_adapt is still refused first)
        bayes.predict(x, row_adapt=True, fused_predict=True)


def test_the_entry_point_is_bound_and_declared():
    import ctypes as C
    from bayesgm_amd import _lib
    res, args = _lib.SYMBOLS["bgm_bgm_hmc_run_rows_impute"]
    traj = _lib.SYMBOLS["bgm_bgm_hmc_run_rows_traj"][1]
    # bgm_bgm_hmc_run_rows_traj's arguments, then moments_dev, cells_dev, slot_dev, k_slots, n_keep, add_noise, and the stream
    assert res is C.c_int and args[:len(traj) - 1] == traj[:-1]
    assert args[len(traj) - 1:] == [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    assert "BGM_API int bgm_bgm_hmc_run_rows_impute(" in header
    from bayesgm_amd.csrc import build
    assert "bgm_impute_api.hip" in build.SOURCES


def test_engine_refuses_impute_without_row_adapt_before_any_device_work():
    from bayesgm_amd.engine import BgmEngine
    eng = object.__new__(BgmEngine)
    with pytest.raises(ValueError, match="impute.*row_adapt"):
        eng.hmc_sample(np.zeros((4, 5), np.float32), 4, 4, impute=True)


@pytest.mark.parametrize("keep", [IR.KEEP, IR.KEEP_LONG])
def test_float32_sequential_sums_stay_inside_both_bounds_on_the_test_inputs(keep):
    """The chains of the NumPy sampler on the p = 20, n = 17 case of the GPU test, decoded in float32 (what the kernel sums) and in
    float64 (the reference): the restatement of the kernel's sums is inside the mean and the variance bound at every missing cell."""
    c = IR.LONG
    m = _model(11, c["q"], c["p"], c["nh"])
    x = _data(c["n"], c["p"], 12, IR.MISS)
    obs, clean = OB.obs_mask_of(x)
    draws = hmc_sampler(m, clean, obs, keep, IR.BURN, 0.1, IR.LEAP, 77, 0.75)["draws"]
    assert draws.shape == (keep, c["n"], c["q"])
    x32 = OB.predict_on_posteriors(m, draws.astype(np.float32), seed=77, burn_in=IR.BURN).astype(np.float32)
    x64 = OB.predict_on_posteriors(OB.cast_model(m, np.float64), draws.astype(np.float64), seed=77, burn_in=IR.BURN)
    assert np.abs(x32 - x64).max() <= IR.VALUE_BAR
    mean_ref, var_ref, mean_bound, var_bound = IR.reference(x64)
    mean, var = IR.mean_var(*IR.moments_f32(x32), keep)
    miss = ~obs
    r_mean = (np.abs(mean - mean_ref) / mean_bound)[miss].max()
    r_var = (np.abs(var - var_ref) / var_bound)[miss].max()
    print("k = %d: worst |mean - ref| / bound %.3g, worst |var - ref| / bound %.3g, gamma_k %.3g" % (keep, r_mean, r_var, IR.gamma(keep)))
    assert r_mean <= 1.0 and r_var <= 1.0
    # and the bounds are not vacuous: a sum that drops one term is outside the variance bound somewhere
    mean_bad, var_bad = IR.mean_var(*IR.moments_f32(x32[:-1]), keep)
    assert (np.abs(var_bad - var_ref) > var_bound)[miss].any() or (np.abs(mean_bad - mean_ref) > mean_bound)[miss].any()
