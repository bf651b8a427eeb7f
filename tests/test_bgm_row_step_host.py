"""BGM HMC with a step size per chain, on the CPU: how the option is resolved and refused, that the entry point exists in the header,
the ctypes table and the built library, and the NumPy restatement (tests/_bgm_row_step_ref.py) in float32 against float64 on the GPU
tests' parity cases -- the reference alone must stay inside the bars the kernels are held to."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bgm_row_step_ref import PARITY, PARITY_CASES, hmc_sampler  # noqa: E402
from test_gpu_bgm import _data, _model  # noqa: E402

from oracle import bgm as OB  # noqa: E402

from bayesgm_amd import _lib, causal_hmc, row_adapt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_resolution():
    f = row_adapt.resolve_step_target
    assert f(False) is None and f(None) is None and f(np.bool_(False)) is None
    assert f(True) == 0.75 == causal_hmc.DEFAULT_TARGET and f(np.bool_(True)) == 0.75
    assert f(0.6) == 0.6 and f(np.float32(0.5)) == 0.5
    for bad in (0, 1, 0.0, 1.0, -0.2, 1.5, float("nan"), "0.8", "row", [0.5]):
        with pytest.raises(ValueError, match="row_adapt"):
            f(bad)
    # the proposal-scale option of the MH sampler keeps its own default
    assert row_adapt.resolve_target(True) == 0.25


def test_bayesian_generator_refuses_the_option_without_a_device():
    from bayesgm_amd.models.bgm_bnn import BGMBayes
    model = object.__new__(BGMBayes)          # no engine, no device: the refusal comes before either is touched
    x = np.zeros((4, 5), np.float32)
    for call in (model.predict, model.tfp_mcmc_sampler):
        for opt in (True, 0.8):
            with pytest.raises(ValueError, match="use_bnn"):
                call(x, row_adapt=opt)


def test_entry_point_is_declared_bound_and_exported():
    from bayesgm_amd.csrc.build import build
    build(force=False, verbose=False)
    name = "bgm_bgm_hmc_run_rows"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgm_hip.h")).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in _lib.SYMBOLS
    assert hasattr(_lib.load(), name)
    assert "bgm_bvn_hmc_run_rows" not in header        # the Bayesian generator has no such entry


@pytest.mark.parametrize("case", [c for c in PARITY_CASES if c["n"] <= 150], ids=lambda c: "p%d-n%d-q%d" % (c["p"], c["n"], c["q"]))
def test_restatement_float32_stays_inside_the_gpu_bars_against_float64(case):
    """Measured at 40 + 10 transitions: 100 % of the rows within 2e-3 at the last draw and every step bit-equal on all four cases
    (at 200 + 20: >= 99.3 % on both counts)."""
    m = _model(11, case["q"], case["p"], case["nh"])
    x = _data(case["n"], case["p"], 12)
    obs, clean = OB.obs_mask_of(x)
    a = (PARITY["n_mcmc"], PARITY["burn_in"], PARITY["step_size"], PARITY["n_leapfrog"], PARITY["seed"], PARITY["target"])
    r32 = hmc_sampler(m, clean, obs, *a)
    r64 = hmc_sampler(m, clean.astype(np.float64), obs, *a)
    assert r32["draws"].dtype == np.float32 and r64["draws"].dtype == np.float64 and r64["step"].dtype == np.float32
    close = np.all(np.abs(r32["draws"][-1] - r64["draws"][-1]) <= 2e-3, axis=1).mean()
    same = (r32["step"] == r64["step"]).mean()
    print("p=%d n=%d: rows within 2e-3 %.4f, steps bit-equal %.4f" % (case["p"], case["n"], close, same))
    assert close >= 0.99 and same >= 0.99, (close, same)
    # the rule moved the steps, and apart
    assert r64["step"].min() > np.float32(PARITY["step_size"]) and len(np.unique(r64["step"])) > 1
