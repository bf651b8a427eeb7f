"""predict_best_dose / hmc_sample(row_choice=True) on the CPU: the NumPy restatement of the kernel's counts
(tests/_causal_hmc_choice_ref.py) against brute force on small arrays with forced ties, the finishing helpers of causal_hmc.py,
every refusal before a device is touched, the other classes' refusal of the method, and the declaration of the entry point.  No
device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_choice_ref as CH  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

DATA = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _bare(cls, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def _error(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


def _brute(y, maximize, threshold):
    """loops, no argmax: counts of the best dose (lowest index on ties), of y > threshold, and the float32 sequential sums"""
    n, nd, m = y.shape
    best, above = np.zeros((n, nd), np.int64), np.zeros((n, nd), np.int64)
    ref, s1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(n):
        for d in range(m):
            k_best, v_best = -1, None
            for k in range(nd):
                val = y[i, k, d]
                if val > np.float32(threshold):
                    above[i, k] += 1
                if np.isnan(val):
                    continue
                if v_best is None or (val > v_best if maximize else val < v_best):
                    k_best, v_best = k, val
            if k_best < 0:
                continue
            best[i, k_best] += 1
            if d == 0:
                ref[i] = v_best
            else:
                s1[i] = np.float32(s1[i] + np.float32(v_best - ref[i]))
    return best, above, ref, s1


@pytest.mark.parametrize("maximize", [True, False], ids=["max", "min"])
def test_the_restatement_against_brute_force_with_forced_ties(maximize):
    rs = np.random.RandomState(7)
    n, nd, m = 9, 18, 23
    y = rs.randn(n, nd, m).astype(np.float32)
    y[:4] = np.round(y[:4] * 2) / 2                                      # a coarse grid: ties at the extremes everywhere
    top = y.max(axis=1) + 1 if maximize else y.min(axis=1) - 1
    for k in (2, 7, 13, 17):                                             # one value beyond every other, at four indices in rows 4, 5
        y[4:6, k] = top[4:6]
    y[6, :, 3] = np.nan                                                  # a draw of NaNs counts nothing
    y[7, 5, :] = np.nan                                                  # a dose of NaNs never wins
    thr = float(np.nanmedian(y))
    best, above, ref, s1 = _brute(y, maximize, thr)
    assert np.array_equal(CH.best_count(y, maximize), best) and np.array_equal(CH.above_count(y, thr), above)
    assert best[4:6, 2].sum() == 2 * m and not best[4:6, [7, 13, 17]].any()      # the lowest index won every tie
    assert best[6].sum() == m - 1 and not best[7, 5] and (np.delete(best, 6, 0).sum(axis=1) == m).all()
    rows = [i for i in range(n) if i != 6]                               # (the NaN draw of row 6 is outside what best_moments restates)
    r_ref, r_s1 = CH.best_moments(y[rows], maximize)
    assert np.array_equal(r_ref, ref[rows]) and np.array_equal(r_s1, s1[rows])
    idx = CH.best_index(y, maximize)
    assert idx[6, 3] == -1 and (np.delete(idx, 6, 0) >= 0).all()
    one = y[:, :1]
    assert np.array_equal(CH.best_count(one, maximize)[rows], np.full((n - 1, 1), m))


def test_choice_finalize():
    rs = np.random.RandomState(3)
    n, nd, m = 6, 5, 40
    y = rs.randn(n, nd, m).astype(np.float32)
    for maximize in (True, False):
        count = CH.best_count(y, maximize)
        ref, s1 = CH.best_moments(y, maximize)
        mean = y.astype(np.float64).mean(axis=-1)
        prob, expected, regret = HM.choice_finalize(count, ref, s1, mean, m, maximize)
        assert prob.dtype == expected.dtype == regret.dtype == np.float64 and prob.shape == regret.shape == (n, nd) and expected.shape == (n,)
        assert np.array_equal(prob, count / float(m)) and np.allclose(prob.sum(axis=1), 1.0, rtol=0, atol=1e-15)
        exact = CH.best_value(y, maximize).astype(np.float64).mean(axis=1)
        assert (np.abs(expected - exact) <= CH.best_mean_bound(y, maximize)).all()
        want = expected[:, None] - mean if maximize else mean - expected[:, None]
        assert np.array_equal(regret, want) and (regret >= -CH.best_mean_bound(y, maximize)[:, None] - 1e-15).all()
        choice = np.argmax(mean if maximize else -mean, axis=1)
        assert np.array_equal(np.argmin(regret, axis=1), choice)
    import torch
    t = HM.choice_finalize(torch.from_numpy(count), torch.from_numpy(ref), torch.from_numpy(s1), torch.from_numpy(mean), m, False)
    assert all(np.array_equal(a, b) for a, b in zip(t, (prob, expected, regret)))
    assert "n_keep must be at least 1" in _error(HM.choice_finalize, count, ref, s1, mean, 0)
    assert "best_count and mean [n, n_doses]" in _error(HM.choice_finalize, count[:, :3], ref, s1, mean, m)
    assert "best_ref and best_s1 [n]" in _error(HM.choice_finalize, count, ref[:2], s1, mean, m)


def test_group_dose_choice():
    choice = np.array([0, 2, 2, 1, 2, 0])
    prob = np.array([[.5, .2, .3], [.1, .1, .8], [0, .4, .6], [.2, .7, .1], [.3, .3, .4], [1, 0, 0]])
    groups = np.array([4, 4, 4, -1, -1, -1])
    out = HM.group_dose_choice(choice, prob, groups)
    assert sorted(out) == [-1, 4]
    assert np.array_equal(out[4][0], np.array([1, 0, 2]) / 3.0) and np.array_equal(out[4][1], prob[:3].sum(axis=0) / 3)
    assert np.array_equal(out[-1][0], np.array([1, 1, 1]) / 3.0) and np.array_equal(out[-1][1], prob[3:].sum(axis=0) / 3)
    assert out[4][0].dtype == out[4][1].dtype == np.float64
    for bad in (np.zeros(5, np.int64), np.zeros(6), np.zeros((6, 1), np.int64)):
        assert "groups must be integer labels of shape [n] = (6,)" in _error(HM.group_dose_choice, choice, prob, bad)


def test_check_choice_kernel():
    for q, metric, partial in ((11, True, True), (19, False, True), (19, True, False), (19, False, False)):
        HM.check_choice_kernel(q, metric, partial)
    for q in (12, 18, 19):
        assert "(here %d)" % q in _error(HM.check_choice_kernel, q, True, True)


def test_check_best_dose():
    assert HM.check_best_dose(False, [1.0], None) is None and HM.check_best_dose(False, 1.0, np.float32(0.5)) == 0.5
    assert HM.check_best_dose(False, [1.0], 2) == 2.0 and isinstance(HM.check_best_dose(False, [1.0], 2), float)
    for bad in (float("nan"), float("inf"), -float("inf"), [0.0], np.zeros(2), "a", True):
        assert "threshold must be None or a finite scalar" in _error(HM.check_best_dose, False, [1.0], bad)
    assert "predict_best_dose needs x_values" in _error(HM.check_best_dose, False, None, None)
    msg = _error(HM.check_best_dose, True, [1.0], None)
    assert "binary" in msg and "predict's ITE" in msg


def test_the_entry_point_is_declared():
    from bayesgm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bgm_hip.h")).read()
    name = "bgm_causal_hmc_run_row_choice"
    assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
    rows, cho = _lib.SYMBOLS["bgm_causal_hmc_run_row_effects"], _lib.SYMBOLS[name]
    # the arguments of bgm_causal_hmc_run_row_effects, then best_count, best_moments, above_count, threshold, maximize, stream
    assert cho[0] is C.c_int and cho[1] == rows[1][:-1] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p]
    assert "uint32_t *best_count_dev, float *best_moments_dev, uint32_t *above_count_dev, float threshold,\n" in header
    assert "int32_t maximize, void *stream);" in header
    assert "replaces: nothing in causalbgm/base.py" in header.split("BGM_API int " + name)[0].rsplit("/*", 1)[1]
    assert '"causal_hmc_choice_api.hip"' in open(os.path.join(ROOT, "bayesgm_amd", "csrc", "build.py")).read()
    abi = open(os.path.join(ROOT, "ABI_MAP.md")).read()
    assert name in abi and "causal_hmc_choice_api.hip" in abi
    from bayesgm_amd.engine import CausalEngine
    assert callable(CausalEngine.hmc_run_rows_choice)


def test_hmc_sample_refuses_before_a_device_is_touched():
    """an engine without a handle or a device: anything past the option checks would raise AttributeError, not ValueError"""
    from bayesgm_amd.engine import CausalEngine
    eng = object.__new__(CausalEngine)
    eng.binary = False
    x, y, v = DATA
    run = (x, y, v, 5, 5, 0.1, 2, 7)
    rows = dict(row_effects=True, x_values=[0.0, 1.0], row_choice=True)
    assert "row_choice belongs to row_effects=True" in _error(eng.hmc_sample, *run, row_choice=True)
    for kw in (dict(row_contrasts=True), dict(row_tails=2)):
        assert "row_choice is not available with row_contrasts or row_tails" in _error(eng.hmc_sample, *run, **rows, **kw)
    for kw in (dict(max_trajectory=0.5), dict(jitter=True)):
        assert "max_trajectory / jitter are not available with row_choice" in _error(eng.hmc_sample, *run, **rows, **kw)
    for bad in (float("inf"), -float("inf"), float("nan"), "a"):
        assert "threshold must be None or a finite scalar" in _error(eng.hmc_sample, *run, threshold=bad, **rows)
    assert "threshold belongs to row_choice=True" in _error(eng.hmc_sample, *run, row_effects=True, x_values=[0.0], threshold=0.0)
    eng.binary = True
    msg = _error(eng.hmc_sample, *run, **rows)
    assert "binary" in msg and "EFFECT_ITE" in msg
    eng.binary = False
    # the one combination whose kernel is not built: a metric with partially observed rows at the KT1 = 2 shapes (q + 1 > 12)
    eng.q = 12
    for kw in (dict(mass="diag"), dict(mass_scale=np.ones((4, 12), np.float32))):
        msg = _error(eng.hmc_sample, *run, partial=True, **rows, **kw)
        assert "more than 11 latent features (here 12)" in msg and "mass='identity'" in msg
    eng.q = 11
    with pytest.raises(AttributeError):      # q + 1 = 12 is a KT1 = 1 shape: the call goes on to the device
        eng.hmc_sample(x, y, v, 40, 5, 0.1, 2, 7, partial=True, mass="diag", **rows)
    with pytest.raises(AttributeError):      # and with the option off the same call does go on to the device
        eng.hmc_sample(*run, row_effects=True, x_values=[0.0, 1.0])


def test_predict_best_dose_refuses_before_a_device_is_touched():
    from bayesgm_amd.models.causalbgm import CausalBGM
    ok = _bare(CausalBGM)
    assert "predict_best_dose needs x_values" in _error(ok.predict_best_dose, DATA, None)
    for bad in (float("nan"), float("inf"), -float("inf"), [0.0], "a"):
        assert "threshold must be None or a finite scalar" in _error(ok.predict_best_dose, DATA, [1.0], threshold=bad)
    assert "groups must be integer labels" in _error(ok.predict_best_dose, DATA, [1.0], groups=np.zeros(3, np.int64))
    binary = _bare(CausalBGM)
    binary._p["binary_treatment"] = True
    msg = _error(binary.predict_best_dose, DATA, [1.0])
    assert "binary" in msg and "predict's ITE" in msg
    x, y, v = (a.copy() for a in DATA)
    x[2] = np.nan
    assert "row 2 has its outcome y observed and its treatment x not" in _error(ok.predict_best_dose, (x, y, v), [1.0], partial=True)
    v[1, 3] = np.nan
    assert "data_v holds NaN in row 1" in _error(ok.predict_best_dose, (DATA[0], DATA[1], v), [1.0], partial=True)
    for kw in (dict(max_trajectory=1.0), dict(jitter_leapfrog=True), dict(alpha=0.1), dict(interval="tails")):      # not taken
        with pytest.raises(TypeError):
            ok.predict_best_dose(DATA, [1.0], **kw)
    wide = _bare(CausalBGM, z_dims=[3, 3, 6, 6])
    msg = _error(wide.predict_best_dose, DATA, [1.0], partial=True, mass="diag")
    assert "more than 11 latent features (here 18)" in msg and "not built" in msg
    narrow = _bare(CausalBGM, z_dims=[1, 1, 1, 7])
    narrow.engine = None
    with pytest.raises(Exception) as e:      # q = 10 has the kernel: the call goes past the option checks
        narrow.predict_best_dose(DATA, [1.0], partial=True, mass="diag", verbose=0)
    assert not isinstance(e.value, ValueError)
    # the refusals of the HMC sampler come first and stay word for word
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(mass="dense"), "mass must be"),
                     (dict(mass="diag", burn_in=10), "burn_in >= 20")):
        msg = _error(ok.predict_best_dose, DATA, [1.0], **kw)
        assert word in msg and msg == _error(ok.predict, DATA, x_values=[0.0], sampler="hmc", **kw)
    # the attributes of an earlier call do not survive a refused one
    ok.dose_regret_ = ok.dose_exceed_prob_ = ok.dose_choice_curve_ = ok.group_dose_choice_ = "stale"
    _error(ok.predict_best_dose, DATA, None)
    assert ok.dose_regret_ is None and ok.dose_exceed_prob_ is None and ok.dose_choice_curve_ is None and ok.group_dose_choice_ is None
    import inspect
    sig = inspect.signature(CausalBGM.predict_best_dose)
    assert sig.parameters["sample_y"].default is False and sig.parameters["maximize"].default is True
    assert "INDEPENDENT predictive noise" in CausalBGM.predict_best_dose.__doc__


def test_the_other_classes_refuse_the_method():
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    for cls, params, word in ((IdentifiableCausalBGM, dict(n_segments=3), "IdentifiableCausalBGM"),
                              (CausalBGMBayes, dict(), "not available for CausalBGMBayes"),
                              (IdentifiableCausalBGMBayes, dict(n_segments=3), "IdentifiableCausalBGMBayes")):
        m = _bare(cls, **params)
        want = _error(m.predict, DATA, x_values=[0.0], sampler="hmc")
        assert word in want and _error(m.predict_best_dose, DATA, [1.0]) == want
        assert _error(m.predict_best_dose, DATA, [1.0], maximize=False, threshold=0.0, partial=True) == want
    bnn = _bare(CausalBGMBayes)
    bnn._p["use_bnn"] = True
    msg = _error(bnn.predict_best_dose, DATA, [1.0])
    assert "use_bnn" in msg and msg == _error(bnn.predict, DATA, x_values=[0.0], sampler="hmc")
