"""The diagonal metric of the CausalBGM HMC sampler on the CPU: the window schedule and the step table (bayesgm_amd/causal_hmc.py), the
NumPy restatement (tests/_causal_hmc_mass_ref.py) against the identity-mass one, the update rule on synthetic moments, the option
checks of the class surface and the ABI.  No device is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _causal_hmc_mass_ref import accumulate, hmc_mass_sampler, update  # noqa: E402
from _causal_hmc_ref import hmc_sampler  # noqa: E402
from oracle import causal as OC  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402
from bayesgm_amd.row_adapt import row_adapt_factors  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2. the schedule
# ---------------------------------------------------------------------------------------------------------------------
def test_mass_windows():
    assert HM.mass_windows(1000) == (75, [100, 150, 250, 450, 950])
    assert HM.mass_windows(5000) == (75, [100, 150, 250, 450, 850, 1650, 4950])
    assert HM.mass_windows(100) == (15, [90])                      # 15 % / 75 % / 10 %
    assert HM.mass_windows(150) == (75, [100]) and HM.mass_windows(149) == (22, [135])
    assert HM.mass_windows(20) == (3, [18])
    for burn in list(range(20, 400)) + [1000, 2500, 5000, 12345]:
        start, ends = HM.mass_windows(burn)
        marks = [start] + ends
        assert ends and start >= 1 and all(b > a for a, b in zip(marks[:-1], marks[1:])) and ends[-1] <= burn, burn
        if burn >= 150:      # the terminal buffer is kept, and every window but the last is twice its predecessor
            assert start == 75 and ends[-1] == burn - 50
            sizes = np.diff(marks)
            assert sizes[0] == 25 or len(sizes) == 1
            assert all(b == 2 * a for a, b in zip(sizes[:-2], sizes[1:-1])) and (len(sizes) == 1 or sizes[-1] >= 2 * sizes[-2])
    for burn in (0, 1, 19):
        assert HM.mass_windows(burn)[1] == []
        with pytest.raises(ValueError, match="burn_in"):
            HM.mass_schedule(burn, 0.75)
        with pytest.raises(ValueError, match="burn_in"):
            HM.check_mass("diag", True, True, burn)


@pytest.mark.parametrize("burn,windows", [(1000, None), (100, None), (20, None), (36, (6, [12, 20, 30])), (20, (6, [12, 20]))])
def test_mass_schedule_restarts_the_gain_in_every_phase(burn, windows):
    (start, ends), (up, dn) = HM.mass_schedule(burn, 0.75, windows)
    assert (start, ends) == (HM.mass_windows(burn) if windows is None else (windows[0], list(windows[1])))
    assert up.dtype == dn.dtype == np.float32 and len(up) == len(dn) == burn
    marks = [0, start] + ends + [burn]
    for a, b in zip(marks[:-1], marks[1:]):
        u, d = row_adapt_factors(b - a, 0.75)
        assert np.array_equal(up[a:b], u) and np.array_equal(dn[a:b], d), (a, b)
    for bad in ((0, [5]), (5, []), (5, [5]), (5, [9, 8]), (5, [burn + 1]), 7):
        with pytest.raises(ValueError, match="mass_windows"):
            HM.mass_schedule(burn, 0.75, bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the restatement with s = 1 is the identity-mass restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_with_unit_scales_is_the_identity_mass_sampler():
    z_dims, p, n = [1, 1, 1, 7], 20, 24
    m = OC.cast_model(OC.init_model(1, z_dims, p), np.float32)
    rs = np.random.RandomState(2)
    v = rs.randn(n, p).astype(np.float32)
    x = rs.exponential(size=(n, 1)).astype(np.float32)
    y = (x + rs.randn(n, 1)).astype(np.float32)
    up, dn = row_adapt_factors(10, 0.75)
    ref = hmc_sampler(m, (x, y, v), 10, 5, 0.1, 3, 77, up, dn)
    one = hmc_mass_sampler(m, (x, y, v), 10, 5, 0.1, 3, 77, up, dn, scale=np.ones((n, 10), np.float32))
    for k in ("draws", "state", "logp", "grad", "acc", "step"):
        assert np.array_equal(ref[k], one[k]), k
    assert ref["draws"].dtype == np.float32 and np.ptp(ref["step"]) > 0 and 0 < ref["acc"].mean() < 1
    # a metric changes the chain, and the windows change the metric
    two = hmc_mass_sampler(m, (x, y, v), 10, 5, 0.1, 3, 77, up, dn, scale=np.full((n, 10), 2.0, np.float32))
    assert not np.array_equal(two["draws"], ref["draws"])
    (start, ends), (up, dn) = HM.mass_schedule(20, 0.75, (4, [10, 16]))
    ad = hmc_mass_sampler(m, (x, y, v), 20, 3, 0.1, 3, 77, up, dn, windows=(start, ends))
    assert ad["scale"].dtype == np.float32 and (np.ptp(ad["scale"], axis=1) > 0).mean() > 0.5
    assert np.abs(np.log(ad["scale"].astype(np.float64)).mean(axis=1)).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 4. the update rule on synthetic moments
# ---------------------------------------------------------------------------------------------------------------------
W_SYN, Q_SYN = 2000, 10
SIGMA = np.logspace(-2, 0, Q_SYN)


def _synthetic_moments(seed=5, n=6):
    """n chains of W_SYN iid draws of N(mu, diag(SIGMA^2)), |mu| up to 3, accumulated in float32 in the kernel's order from the
    chain's first state -> (s1, s2, last state), [n x q] each"""
    rs = np.random.RandomState(seed)
    mu = rs.uniform(-3, 3, (n, Q_SYN))
    ref = (mu + SIGMA * rs.randn(n, Q_SYN)).astype(np.float32)
    s1 = s2 = np.zeros((n, Q_SYN), np.float32)
    for _ in range(W_SYN):
        z = (mu + SIGMA * rs.randn(n, Q_SYN)).astype(np.float32)
        s1, s2 = accumulate(z, ref, s1, s2)
    return s1, s2, z


def test_update_rule_on_synthetic_moments():
    """The rule on W = 2000 iid draws of N(mu, diag(sigma^2)), sd spread over 0.01 .. 1, |mu| up to 3, q = 10, accumulated in float32 in
    the kernel's order.  s_i / (sigma_i / geomean(sigma)) is within 10 % for every coordinate: about six standard errors of an sd
    estimate from 2000 draws (6 / sqrt(2 W) = 9.5 %).  The shrinkage (5 draws' weight on 1e-3 of the chain's mean variance) moves the
    smallest sd by 0.2 % here; with the whole mean variance as its target it would move it by a factor 2.2 and this bar could not
    hold.  Both statements of the rule (causal_hmc.mass_update, vectorised; the restatement, row by row) agree to 1e-6; the geometric
    mean of s is 1 to 1e-5; a chain with all moments zero, or with a moment that is not finite, keeps its scales; W = 0 only resets."""
    s1, s2, z = _synthetic_moments()
    prev = np.full_like(s1, 3.0)
    s, ref, n1, n2 = HM.mass_update(W_SYN, z, prev, z * 0, s1, s2)
    s_row, ref_row, _, _ = update(W_SYN, z, prev, z * 0, s1, s2)
    assert s.dtype == np.float32 and np.abs(s / s_row - 1).max() <= 1e-6
    assert np.array_equal(ref, z) and np.array_equal(ref_row, z) and not n1.any() and not n2.any()
    assert np.abs(np.exp(np.log(s.astype(np.float64)).mean(axis=1)) - 1).max() <= 1e-5
    ratio = s / (SIGMA / np.exp(np.log(SIGMA).mean()))
    print("s / (sigma / geomean(sigma)): min %.4f, max %.4f" % (ratio.min(), ratio.max()))
    assert np.abs(ratio - 1).max() <= 0.10, (ratio.min(), ratio.max())
    # a coordinate that never moved is held at the clamp by the shrinkage, not at zero
    t1, t2 = s1.copy(), s2.copy()
    t1[0, 4] = t2[0, 4] = 0.0
    s0 = HM.mass_update(W_SYN, z, prev, z * 0, t1, t2)[0][0]
    assert s0[4] == np.float32(0.05) and np.all(s0 > 0) and np.array_equal(s0, update(W_SYN, z, prev, z * 0, t1, t2)[0][0])
    # a chain that never moved keeps its scales; a chain whose moments are not finite does too
    s1[1] = s2[1] = 0.0
    s2[2, 3] = np.inf
    s, _, _, _ = HM.mass_update(W_SYN, z, prev, z * 0, s1, s2)
    s_row, _, _, _ = update(W_SYN, z, prev, z * 0, s1, s2)
    assert np.all(s[1] == 3.0) and np.all(s[2] == 3.0) and np.all(s[0] != 3.0) and np.array_equal(s[1:3], s_row[1:3])
    # W = 0 only resets
    s, ref, n1, n2 = HM.mass_update(0, z, prev, z * 0, s1, s2)
    assert np.array_equal(s, prev) and np.array_equal(ref, z) and not n1.any() and not n2.any()
    assert np.array_equal(update(0, z, prev, z * 0, s1, s2)[0], prev)


def test_update_rule_recovers_sigma_over_its_geometric_mean():
    """The bar on its own, for every chain of the synthetic panel and from unit scales: s_i / (sigma_i / geomean(sigma)) within 10 %
    for every coordinate, sd spread over 0.01 .. 1, W = 2000 (measured 0.956 .. 1.035; 0.836 .. 1.916 with the whole mean variance
    as the shrinkage target)."""
    s1, s2, z = _synthetic_moments()
    s, _, _, _ = HM.mass_update(W_SYN, z, np.ones_like(s1), z * 0, s1, s2)
    ratio = s / (SIGMA / np.exp(np.log(SIGMA).mean()))
    print("s / (sigma / geomean(sigma)): min %.4f, max %.4f" % (ratio.min(), ratio.max()))
    assert np.abs(ratio - 1).max() <= 0.10, (ratio.min(), ratio.max())


# ---------------------------------------------------------------------------------------------------------------------
# 5. option checks: every ValueError is raised before anything touches the engine
# ---------------------------------------------------------------------------------------------------------------------
def _bare(cls, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def test_mass_option_checks_need_no_device():
    from bayesgm_amd.models.causalbgm import CausalBGM
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    data = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))
    assert CausalBGM.hmc_row_mass_ is None
    ok = _bare(CausalBGM)
    # an unknown mass
    for call in (lambda: ok.hmc_sampler(data, mass="dense"), lambda: ok.predict(data, x_values=[0.0], sampler="hmc", mass="dense"),
                 lambda: ok.predict(data, x_values=[0.0], mass=1.0)):
        with pytest.raises(ValueError, match="mass must be"):
            call()
    # 'diag' belongs to the HMC sampler
    with pytest.raises(ValueError, match="mass='diag' belongs to sampler='hmc'"):
        ok.predict(data, x_values=[0.0], mass="diag")
    with pytest.raises(ValueError, match="mass='diag' belongs to sampler='hmc'"):
        ok.predict(data, x_values=[0.0], sampler="mh", mass="diag", row_adapt=True)
    # a metric change without a step re-adaptation
    with pytest.raises(ValueError, match="adapt=True"):
        ok.hmc_sampler(data, mass="diag", adapt=False)
    # a burn-in without room for a window
    with pytest.raises(ValueError, match="burn_in"):
        ok.hmc_sampler(data, mass="diag", burn_in=19)
    with pytest.raises(ValueError, match="burn_in"):
        ok.predict(data, x_values=[0.0], sampler="hmc", mass="diag", burn_in=10)
    # good options go on to the next argument check; 'identity' and None are the call without the argument
    for mass in ("diag", "identity", None):
        with pytest.raises(ValueError, match="x_values"):
            ok.predict(data, sampler="hmc", mass=mass)
    with pytest.raises(ValueError, match="x_values"):
        ok.predict(data, mass="identity")
    # the existing refusals come first, word for word
    with pytest.raises(ValueError, match="n_leapfrog"):
        ok.hmc_sampler(data, mass="diag", n_leapfrog=0)
    with pytest.raises(ValueError, match="row_adapt"):
        ok.predict(data, x_values=[0.0], sampler="hmc", mass="diag", row_adapt=True)
    m = _bare(CausalBGM)
    m._p["mh_precision"] = "f16x3"
    with pytest.raises(ValueError, match="mh_precision"):
        m.predict(data, x_values=[0.0], sampler="hmc", mass="diag")
    for cls in (IdentifiableCausalBGM, IdentifiableCausalBGMBayes):
        m = _bare(cls, n_segments=3)
        with pytest.raises(ValueError, match=r"not available for Identifiable\w+: the gradient kernels exist for the standard-normal"):
            m.predict(data, x_values=[0.0], sampler="hmc", mass="diag")
        with pytest.raises(ValueError, match=r"not available for Identifiable\w+: the gradient kernels exist for the standard-normal"):
            m.hmc_sampler(data, mass="diag")
        with pytest.raises(ValueError, match="mass='diag' belongs to sampler='hmc'"):
            m.predict(data, x_values=[0.0], mass="diag")
    m = _bare(CausalBGMBayes)
    m._p["use_bnn"] = True
    with pytest.raises(ValueError, match=r"params\['use_bnn'\] = True: the Bayesian-network sampling kernels have no gradient path"):
        m.predict(data, x_values=[0.0], sampler="hmc", mass="diag")
    with pytest.raises(ValueError, match=r"params\['use_bnn'\] = True: the Bayesian-network sampling kernels have no gradient path"):
        m.hmc_sampler(data, mass="diag")


# ---------------------------------------------------------------------------------------------------------------------
# 6. ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_mass_entry_points():
    from bayesgm_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bgm_hip.h")).read()
    for name, n_args in (("bgm_causal_hmc_set_mass", 6), ("bgm_causal_hmc_mass_update", 9)):
        assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
        assert len(_lib.SYMBOLS[name][1]) == n_args
    assert len(_lib.SYMBOLS["bgm_causal_hmc_run"][1]) == 25      # the run keeps its signature
