"""BGM HMC with a number of leapfrog steps per chain, on the CPU: how the options are resolved and refused, that the entry point exists
in the header, the ctypes table and the built library, the cap rule at its edges, and the NumPy restatement (tests/_bgm_traj_ref.py) in
float32 against float64 on the GPU tests' parity cases -- the reference alone must stay inside the bars the kernels are held to."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bgm_traj_ref import PARITY_CASES, TRAJ_PARITY, hmc_sampler  # noqa: E402
from test_gpu_bgm import _data, _model  # noqa: E402

from oracle import bgm as OB  # noqa: E402

from bayesgm_amd import _lib, row_adapt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_resolution():
    f = row_adapt.resolve_trajectory
    assert f(None) == (0.0, 0) and f(0.75) == (0.0, 0) and f(None, None, False) == (0.0, 0)
    assert f(0.75, 0.4) == (0.4, 0) and f(0.75, None, True) == (0.0, 1) and f(0.6, np.float32(0.5), np.bool_(True)) == (0.5, 1)
    assert f(0.75, 2, 1) == (2.0, 1)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "0.4", [0.4], True):
        with pytest.raises(ValueError, match="max_trajectory"):
            f(0.75, bad)
    for bad in (2, -1, 0.5, "yes", None):
        with pytest.raises(ValueError, match="jitter"):
            f(0.75, None, bad)
    # either option needs the step per chain, and says so
    for kw in (dict(max_trajectory=0.4), dict(jitter=True), dict(max_trajectory=0.4, jitter=True)):
        with pytest.raises(ValueError, match="row_adapt"):
            f(None, **kw)


def test_classes_refuse_the_options_without_row_adapt_or_a_device():
    from bayesgm_amd.models.bgm import BGM
    from bayesgm_amd.models.bgm_bnn import BGMBayes
    x = np.zeros((4, 5), np.float32)
    model = object.__new__(BGM)               # no engine, no device: the refusal comes before either is touched
    for call in (model.predict, model.tfp_mcmc_sampler):
        for kw in (dict(max_trajectory=0.4), dict(jitter_leapfrog=True), dict(row_adapt=False, max_trajectory=1.0, jitter_leapfrog=True)):
            with pytest.raises(ValueError, match="row_adapt"):
                call(x, **kw)
        with pytest.raises(ValueError, match="max_trajectory"):
            call(x, row_adapt=True, max_trajectory=-1.0)
    bayes = object.__new__(BGMBayes)
    for call in (bayes.predict, bayes.tfp_mcmc_sampler):
        for kw in (dict(max_trajectory=0.4), dict(jitter_leapfrog=True)):
            with pytest.raises(ValueError, match="use_bnn"):
                call(x, **kw)


def test_entry_point_is_declared_bound_and_exported():
    from bayesgm_amd.csrc.build import build
    build(force=False, verbose=False)
    name = "bgm_bgm_hmc_run_rows_traj"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgm_hip.h")).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == 11
    assert hasattr(_lib.load(), name)
    assert "bgm_bvn_hmc_run_rows_traj" not in header        # the Bayesian generator has no such entry
    assert name in open(os.path.join(ROOT, "ABI_MAP.md")).read()


def test_leapfrog_cap_at_the_edges():
    f = row_adapt.leapfrog_cap
    L = 10
    # no cap
    assert f(np.float32(0.6), L, None) == L and f(np.float32(0.6), L, 0) == L
    # eps >= T: one step; eps * (L - 1) < T: all of them
    assert np.array_equal(f(np.array([0.5, 0.7, 100.0], np.float32), L, 0.5), [1, 1, 1])
    assert np.array_equal(f(np.array([0.05, 1e-4], np.float32), L, 0.5), [L, L])
    assert f(np.float32(0.5) / 9 * np.float32(1.0001), L, 0.5) == L - 1
    # l * eps == T exactly (powers of two: the float32 product is exact): the compare is strict, l itself is not taken
    assert f(np.float32(0.125), L, 0.5) == 4 and f(np.float32(0.125), L, 0.5 + 1e-6) == 5
    assert f(np.float32(0.25), 2, 0.25) == 1 and f(np.float32(0.25), 1, 1e-9) == 1
    # the rule is the float32 product, not a quotient: 3 * 0.1f rounds to 0.3f, so under T = 0.3f step 3 is not taken, where the exact
    # quotient 0.3f / 0.1f = 3.00000007 would take it
    e, T = np.float32(0.1), np.float32(0.3)
    assert np.float32(3) * e == T and np.ceil(np.float64(T) / np.float64(e)) == 4 and f(e, L, T) == 3
    # clamp(ceil(T / eps), 1, L) wherever no product lies within a rounding error of T
    rs = np.random.RandomState(0)
    eps = rs.uniform(0.01, 2.0, 2000).astype(np.float32)
    T = np.float32(np.pi / 2)
    want = np.clip(np.ceil(np.float64(T) / eps.astype(np.float64)), 1, L).astype(np.int32)
    clear = np.all(np.abs(np.arange(1, L)[:, None] * eps.astype(np.float64)[None] - np.float64(T)) > 1e-6, axis=0)
    got = f(eps, L, T)
    assert got.dtype == np.int32 and got.shape == eps.shape and clear.mean() > 0.99 and np.array_equal(got[clear], want[clear])
    assert set(got) == set(range(1, L + 1))
    # the frozen steps of the GPU tests: 0.10 < 0.12 <= 0.15, and 4 x 0.03f == 0.12f exactly
    assert np.array_equal(f(np.array([0.05, 0.03], np.float32), 6, 0.12), [3, 4])
    assert f(np.float32(0.6283), 10, np.pi / 2) == 3
    with pytest.raises(ValueError, match="n_leapfrog"):
        f(eps, 0, T)


@pytest.mark.parametrize("jitter", [False, True], ids=["cap", "cap-jitter"])
@pytest.mark.parametrize("case", [c for c in PARITY_CASES if c["n"] <= 150], ids=lambda c: "p%d-n%d-q%d" % (c["p"], c["n"], c["q"]))
def test_restatement_float32_stays_inside_the_gpu_bars_against_float64(case, jitter):
    """Measured at 40 + 10 transitions, L = 6, max_trajectory = 0.4: 100 % of the rows within 2e-3 at the last draw, every step and
    every L_i equal on all four cases, without and with jitter."""
    m = _model(11, case["q"], case["p"], case["nh"])
    x = _data(case["n"], case["p"], 12)
    obs, clean = OB.obs_mask_of(x)
    P = TRAJ_PARITY
    a = (P["n_mcmc"], P["burn_in"], P["step_size"], P["n_leapfrog"], P["seed"], P["target"], P["max_trajectory"], jitter)
    r32 = hmc_sampler(m, clean, obs, *a)
    r64 = hmc_sampler(m, clean.astype(np.float64), obs, *a)
    assert r32["draws"].dtype == np.float32 and r64["draws"].dtype == np.float64 and r64["step"].dtype == np.float32
    close = np.all(np.abs(r32["draws"][-1] - r64["draws"][-1]) <= 2e-3, axis=1).mean()
    same = (r32["step"] == r64["step"]).mean()
    same_li = np.all(r32["li"] == r64["li"], axis=0).mean()
    kept = r64["li"][P["burn_in"]:]
    print("p=%d n=%d jitter=%d: rows within 2e-3 %.4f, steps bit-equal %.4f, rows with every L_i equal %.4f, retained L_i %d .. %d"
          % (case["p"], case["n"], jitter, close, same, same_li, kept.min(), kept.max()))
    assert close >= 0.99 and same >= 0.99 and same_li >= 0.99, (close, same, same_li)
    # the cap comes to bind at another iteration for every row, so rows of one 16-row tile take different numbers of steps in one transition
    li = r64["li"]
    assert len(np.unique(li)) > 1 and any((li[:, t:t + 16].max(axis=1) != li[:, t:t + 16].min(axis=1)).any() for t in range(0, case["n"], 16))
    assert kept.min() >= 1 and kept.max() <= P["n_leapfrog"]
    assert np.array_equal(r64["n_steps"], kept.sum(axis=0))
    if not jitter:      # frozen steps: a retained cap is the cap of the final step
        assert np.all(kept == row_adapt.leapfrog_cap(r64["step"], P["n_leapfrog"], P["max_trajectory"])[None])
