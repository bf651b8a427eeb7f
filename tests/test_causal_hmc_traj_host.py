"""The trajectory options of the CausalBGM HMC sampler (max_trajectory / jitter_leapfrog, bgm_causal_hmc_set_trajectory), everything
that needs no GPU: the restatement's own error, the option checks, the class-level refusals made before a device is touched, the
ABI declaration and the cap rule at its edges."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_traj_ref as TR  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402
from bayesgm_amd import row_adapt as RA  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
V = np.zeros((4, 3), np.float32)


def _bare(cls, binary=False, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=binary, **params)
    obj.params = obj._p
    return obj


def _error(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


@pytest.mark.parametrize("case", TR.PARITY_CASES, ids=lambda c: "q%d" % sum(c["z_dims"]))
@pytest.mark.parametrize("jitter", [False, True])
def test_float32_restatement_keeps_the_share_against_its_float64_twin(case, jitter):
    """The GPU bar (>= 97 % of the rows within 1e-4 of the float32 restatement, n_steps equal on those rows) rests on the float32
    restatement itself following its float64 twin: 15 + 15 transitions, L = 6, adapting, the cap on.  Measured: 100 % of the rows and
    every step count equal on the four cases."""
    a, b = TR.parity_run(case, jitter, np.float32), TR.parity_run(case, jitter, np.float64)
    ok = np.all(np.abs(a["draws"][-1] - b["draws"][-1]) <= 1e-4, axis=1)
    same = a["n_steps"] == b["n_steps"]
    print("rows equal %.4f, n_steps equal %.4f, L_i %d .. %d, mean L_i %.3f" % (ok.mean(), same.mean(), a["li"].min(), a["li"].max(), a["li"].mean()))
    assert ok.mean() >= 0.985 and same.mean() >= ok.mean() - 1e-12
    assert np.array_equal(a["step"][ok], b["step"][ok])
    # the options are live on these cases: the cap binds, moves with the step, and the jitter spreads L_i below it
    cap = RA.leapfrog_cap(a["step"], TR.PARITY["n_leapfrog"], TR.PARITY["max_trajectory"])
    assert a["li"][-1].max() < TR.PARITY["n_leapfrog"] and len(np.unique(a["li"])) > 2
    assert np.all(a["li"][-1] <= cap) and (jitter or np.array_equal(a["li"][-1], cap))
    assert np.all(a["n_steps"] >= TR.PARITY["n_keep"]) and np.all(a["n_steps"] < TR.PARITY["n_keep"] * TR.PARITY["n_leapfrog"])


def test_the_restatement_with_the_options_off_is_the_existing_one():
    import _causal_hmc_ref as REF
    case, P = TR.PARITY_CASES[0], TR.PARITY
    m, data = TR.parity_inputs(case)
    up, dn = RA.row_adapt_factors(P["burn_in"], TR.TARGET)
    a = TR.hmc_sampler(m, data, P["burn_in"], 5, P["step0"], 3, P["seed"], up, dn)
    b = REF.hmc_sampler(m, data, P["burn_in"], 5, P["step0"], 3, P["seed"], up, dn)
    for k in ("draws", "state", "logp", "grad", "acc", "step"):
        assert np.array_equal(a[k], b[k]), k
    assert np.all(a["li"] == 3) and np.all(a["n_steps"] == 15)


def test_the_restatement_alone_shows_the_defect_and_its_cure():
    """The panel of the GPU test (x and y unobserved, frozen step 1.05, L = 6: eps x L = 6.3, about 2 pi): float64 and float32
    restatement agree to the digits the GPU test compares, and the cap of pi / 2 (2 steps) takes the lag-1 autocorrelation from
    about +0.91 to about -0.17."""
    plain, capped = TR.defect_run(False), TR.defect_run(True)
    a, b = np.median(TR.lag1(plain["draws"])), np.median(TR.lag1(capped["draws"]))
    print("median lag-1 autocorrelation: uncapped %+.4f, max_trajectory = pi / 2 %+.4f" % (a, b))
    assert a > 0.85 and b < 0.0
    assert np.all(plain["n_steps"] == 6 * TR.DEFECT["n_keep"]) and np.all(capped["n_steps"] == 2 * TR.DEFECT["n_keep"])
    for run, ref in ((plain, a), (capped, b)):
        assert run["acc"].mean() > 0.5
    assert "%.3f" % np.median(TR.lag1(TR.defect_run(True, np.float32)["draws"])) == "%.3f" % b


def test_resolve_trajectory():
    assert HM.resolve_trajectory() == (0.0, 0) and HM.resolve_trajectory(None, False) == (0.0, 0)
    assert HM.resolve_trajectory(1.5, True) == (1.5, 1) and HM.resolve_trajectory(np.float32(2.0), np.bool_(False)) == (2.0, 0)
    assert HM.resolve_trajectory(3, 1) == (3.0, 1)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1.0", True, [1.0]):
        assert "max_trajectory must be None" in _error(HM.resolve_trajectory, bad), bad
    for bad in (2, -1, "yes", 0.5, None):
        assert "jitter must be False or True" in _error(HM.resolve_trajectory, 1.0, bad), bad
    # no row_adapt requirement: this sampler's step is always per chain (row_adapt's own resolver keeps it)
    assert "needs row_adapt" in _error(RA.resolve_trajectory, None, 1.0)
    assert HM.check_trajectory(None, False, hmc=False) == (0.0, 0) and HM.check_trajectory(None, False, True, "tails") == (0.0, 0)
    assert "sampler='hmc'" in _error(HM.check_trajectory, 1.0, False, False)
    assert "interval='tails'" in _error(HM.check_trajectory, None, True, True, "tails")


def test_class_refusals_before_a_device_is_touched():
    from bayesgm_amd.models.causalbgm import CausalBGM
    cont, binr = _bare(CausalBGM), _bare(CausalBGM, True)
    data = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), V)
    for kw in (dict(max_trajectory=1.0), dict(jitter_leapfrog=True)):
        msg = _error(cont.predict, data, x_values=[0.0], sampler="mh", **kw)
        assert "max_trajectory / jitter_leapfrog belong to sampler='hmc'" in msg
        assert msg == _error(cont.predict, data, x_values=[0.0], **kw) == _error(binr.predict, data, **kw)
        msg = _error(cont.predict_individual, data, [0.0], interval="tails", **kw)
        assert "interval='tails'" in msg and "max_trajectory / jitter_leapfrog" in msg
        assert msg == _error(cont.predict_new, V, x_values=[0.0], interval="tails", **kw)
    for method, args in ((cont.predict, (data,)), (cont.predict_individual, (data, [0.0])), (cont.predict_new, (V,)), (cont.hmc_sampler, (data,))):
        kw = dict(x_values=[0.0]) if method in (cont.predict, cont.predict_new) else {}
        kw.update(dict(sampler="hmc") if method == cont.predict else {})
        assert "max_trajectory must be None" in _error(method, *args, max_trajectory=-1.0, **kw), method
        assert "jitter must be False or True" in _error(method, *args, jitter_leapfrog=2, **kw), method
    for name in ("predict", "predict_individual", "predict_new", "hmc_sampler"):
        par = inspect.signature(getattr(CausalBGM, name)).parameters
        assert par["max_trajectory"].default is None and par["jitter_leapfrog"].default is False, name
    assert "max_trajectory" not in inspect.signature(CausalBGM.predict_average).parameters
    assert CausalBGM.hmc_row_leapfrog_ is None


def test_the_other_classes_keep_refusing_as_they_do():
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    data = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), V)
    for cls, params in ((IdentifiableCausalBGM, dict(n_segments=3)), (CausalBGMBayes, dict())):
        assert "max_trajectory" not in inspect.signature(cls.predict).parameters, cls
        assert "sampler='hmc'" in _error(_bare(cls, **params).predict, data, x_values=[0.0], sampler="hmc")


def test_engine_signatures():
    from bayesgm_amd.engine import CausalEngine
    par = inspect.signature(CausalEngine.hmc_sample).parameters
    assert par["max_trajectory"].default is None and par["jitter"].default is False
    par = inspect.signature(CausalEngine.set_hmc_trajectory).parameters
    assert [par[k].default for k in ("max_trajectory", "jitter", "n_steps")] == [None, False, None]


def test_abi_declares_the_entry_point():
    from bayesgm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bgm_hip.h")).read()
    name = "bgm_causal_hmc_set_trajectory"
    assert "BGM_API int %s(bgm_handle *h, float max_trajectory, int32_t jitter, int32_t *n_steps_dev);" % name in header
    assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_float, C.c_int32, C.c_void_p])
    row = [line for line in open(os.path.join(ROOT, "ABI_MAP.md")) if line.startswith("| `%s` |" % name)]
    assert len(row) == 1 and "causal_hmc_traj_api.hip" in row[0] and "set_hmc_trajectory" in row[0]
    assert "causal_hmc_traj_api.hip" in open(os.path.join(ROOT, "bayesgm_amd", "csrc", "build.py")).read()


def test_leapfrog_cap_edges():
    f = np.float32
    L = 6
    # eps >= T: one step, whatever L
    assert RA.leapfrog_cap(f(0.5), L, 0.5) == 1 and RA.leapfrog_cap(f(0.7), L, 0.5) == 1 and RA.leapfrog_cap(f(0.5), 1, 0.5) == 1
    # eps x (L - 1) < T: all L
    assert RA.leapfrog_cap(f(0.05), L, 0.26) == L and RA.leapfrog_cap(f(0.05), L, 1e9) == L
    # an exact tie in float32 (0.25 x 2 = 0.5, no rounding): l x eps < T is strict, so l = 2 is not counted
    assert RA.leapfrog_cap(f(0.25), L, 0.5) == 2 and RA.leapfrog_cap(f(0.25), L, np.nextafter(f(0.5), f(1))) == 3
    # no cap
    assert RA.leapfrog_cap(f(3.0), L, None) == L and RA.leapfrog_cap(f(3.0), L, 0.0) == L
    # the cases of the GPU tests: 0.05 -> 3 and 0.03 -> 5 of L = 6 under T = 0.13, with the products away from T
    caps = RA.leapfrog_cap(np.array([0.05, 0.03], f), L, 0.13)
    assert caps.dtype == np.int32 and caps.tolist() == [3, 5]
    for eps, l in ((0.05, 2), (0.05, 3), (0.03, 4), (0.03, 5)):
        assert abs(float(f(l) * f(eps)) - 0.13) > 5e-3
    # the defect panel: step 1.05 under pi / 2 takes 2 of 6 steps
    assert RA.leapfrog_cap(f(TR.DEFECT["step"]), TR.DEFECT["n_leapfrog"], TR.DEFECT["max_trajectory"]) == 2
