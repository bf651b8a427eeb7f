"""The HMC latent sampler of CausalBGM on the CPU: the NumPy restatement (tests/_causal_hmc_ref.py) against finite differences and
oracle.fit, the integrator's reversibility and order, and the option checks of the class surface.  No device is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _causal_hmc_ref import hmc_sampler, leapfrog, log_posterior_and_grad  # noqa: E402
from oracle import causal as OC  # noqa: E402
from oracle import fit as OF  # noqa: E402
from oracle.nets import mlp_forward_cache  # noqa: E402

Z_DIMS, P = [1, 1, 1, 7], 20
FIXED = dict(sigma_v=0.8, sigma_x=1.3, sigma_y=0.5)


def _model(seed, binary=False, **kw):
    m = OC.init_model(seed, Z_DIMS, P, binary_treatment=binary, **kw)
    rs = np.random.RandomState(seed + 99)
    for k in ("g", "f", "h", "e"):      # non-zero biases
        m[k] = [(W.astype(np.float64), 0.1 * rs.randn(*b.shape)) for W, b in m[k]]
    return m


def _data(n, seed, binary=False):
    rs = np.random.RandomState(seed)
    v = rs.randn(n, P)
    x = rs.exponential(size=(n, 1))
    if binary:
        x = (x > np.median(x)).astype(np.float64)
    return x, x + rs.randn(n, 1), v


def _near_kink(m, x, z, tol):
    """rows with a hidden pre-activation of g, h or f within tol of zero: the log posterior is not differentiable at zero"""
    z0, z1, z2 = OC.split_z(m, z)
    bad = np.zeros(len(z), bool)
    for net, inp in ((m["g"], z), (m["h"], np.concatenate([z0, z2], -1)), (m["f"], np.concatenate([z0, z1, x], -1))):
        for pre in mlp_forward_cache(net, inp)[1][1][:-1]:
            bad |= (np.abs(pre) < tol).any(axis=1)
    return bad


@pytest.mark.parametrize("binary,fixed", [(False, False), (True, False), (False, True)])
def test_gradient_against_central_differences(binary, fixed):
    """h = 1e-5, agreement within 1e-6 max(1, |g|) per element; rows with a pre-activation within 1e-4 of zero are left out, at most 1 %
    of them.  Every row has about 800 hidden units, so about one row in eight has such a unit: the panel is 10 rows whose latents
    (seed 7) have none, and the cap holds with nothing left out."""
    n, h = 10, 1e-5
    m = _model(1, binary, **(FIXED if fixed else {}))
    x, y, v = _data(n, 2, binary)
    z = np.random.RandomState(7).randn(n, sum(Z_DIMS))
    out = _near_kink(m, x, z, 1e-4)
    assert out.mean() <= 0.01, out.mean()
    lp, g = log_posterior_and_grad(m, x, y, v, z)
    assert lp.dtype == np.float64 and np.array_equal(lp, OC.log_posterior(m, x, y, v, z))
    fd = np.empty_like(z)
    for k in range(z.shape[1]):
        zp, zm = z.copy(), z.copy()
        zp[:, k] += h
        zm[:, k] -= h
        fd[:, k] = (OC.log_posterior(m, x, y, v, zp) - OC.log_posterior(m, x, y, v, zm)) / (2 * h)
    err = np.abs(g - fd)[~out] / np.maximum(1.0, np.abs(g))[~out]
    print("worst |grad - central difference| / max(1, |grad|): %.3g" % err.max())
    assert err.max() <= 1e-6


@pytest.mark.parametrize("binary,fixed", [(False, False), (True, False), (False, True)])
def test_gradient_against_oracle_fit(binary, fixed):
    """the same gradient is -B times the dz of oracle.fit.z_loss_and_grad (batch-mean negative log joint), 1e-12 relative in float64"""
    n = 37
    m = _model(3, binary, **(FIXED if fixed else {}))
    x, y, v = _data(n, 4, binary)
    z = np.random.RandomState(5).randn(n, sum(Z_DIMS))
    lp, g = log_posterior_and_grad(m, x, y, v, z)
    loss, dz = OF.z_loss_and_grad(m, z, x, y, v)
    assert np.abs(g + n * dz).max() <= 1e-12 * np.abs(g).max()
    assert abs(loss + lp.mean()) <= 1e-12 * abs(loss)
    # and the dtype follows z
    m32 = OC.cast_model(m, np.float32)
    lp32, g32 = log_posterior_and_grad(m32, *(a.astype(np.float32) for a in (x, y, v, z)))
    assert lp32.dtype == np.float32 and g32.dtype == np.float32
    assert np.abs(g32 - g).max() <= 1e-3 * np.abs(g).max()


def _setup(n=24):
    m = _model(1)
    x, y, v = _data(n, 2)
    z = np.random.RandomState(3).randn(n, sum(Z_DIMS))
    mom = np.random.RandomState(4).randn(n, sum(Z_DIMS))
    lp, gr = log_posterior_and_grad(m, x, y, v, z)
    return m, x, y, v, z, mom, lp, gr


def test_leapfrog_is_reversible():
    m, x, y, v, z, mom, lp, gr = _setup()
    step = np.full(len(z), 0.01)
    zc, pc, lpc, grc = leapfrog(m, x, y, v, z, mom, gr, step, 5)
    assert np.abs(zc - z).max() > 1e-2
    zb, pb, lpb, _ = leapfrog(m, x, y, v, zc, -pc, grc, step, 5)
    assert np.abs(zb - z).max() <= 1e-10 and np.abs(pb + mom).max() <= 1e-10 and np.abs(lpb - lp).max() <= 1e-10 * np.abs(lp).max()


def test_energy_error_is_second_order():
    """The same trajectory length with the step halved: |H1 - H0| shrinks by 4.  The log posterior is piecewise smooth (LeakyReLU), and
    a trajectory that crosses a kink loses the order: at a step of 3e-4 over 4 steps no row of this panel does (measured: ratios
    3.9987 .. 4.04; at 1e-3 the median is 4.0 but single rows are off)."""
    m, x, y, v, z, mom, lp, gr = _setup()
    h0 = -lp + (mom ** 2).sum(axis=1) / 2
    dh = []
    for step, L in ((3e-4, 4), (1.5e-4, 8)):
        zc, pc, lpc, _ = leapfrog(m, x, y, v, z, mom, gr, np.full(len(z), step), L)
        dh.append(np.abs(-lpc + (pc ** 2).sum(axis=1) / 2 - h0))
    ratio = dh[0] / dh[1]
    print("energy error ratio min / median / max: %.4f / %.4f / %.4f" % (ratio.min(), np.median(ratio), ratio.max()))
    assert np.all(ratio > 3.0) and np.all(ratio < 5.0)


def test_sampler_restatement_adapts_and_is_row_local():
    """the float32 restatement: steps move towards the target, and rows [8, 24) alone with row0 = 8 reproduce their chains (the BLAS
    products of NumPy depend on the batch in their last bits, so the draws are compared within 1e-4; the decisions, hence the steps, are
    the same)"""
    from bayesgm_amd.row_adapt import row_adapt_factors
    m = OC.cast_model(_model(1), np.float32)
    x, y, v = (a.astype(np.float32) for a in _data(24, 2))
    up, dn = row_adapt_factors(10, 0.75)
    full = hmc_sampler(m, (x, y, v), 10, 5, 0.1, 3, 77, up, dn)
    part = hmc_sampler(m, (x[8:], y[8:], v[8:]), 10, 5, 0.1, 3, 77, up, dn, row0=8)
    assert full["draws"].shape == (5, 24, 10) and full["draws"].dtype == np.float32 and full["step"].dtype == np.float32
    assert np.abs(full["draws"][:, 8:] - part["draws"]).max() <= 1e-4 and np.array_equal(full["step"][8:], part["step"])
    assert np.ptp(full["step"]) > 0
    fixed = hmc_sampler(m, (x, y, v), 10, 5, 0.1, 3, 77, None, None)
    ones = np.ones(10, np.float32)
    same = hmc_sampler(m, (x, y, v), 10, 5, 0.1, 3, 77, ones, ones)
    assert np.array_equal(fixed["draws"], same["draws"]) and np.all(fixed["step"] == np.float32(0.1))


# ---------------------------------------------------------------------------------------------------------------------
# option checks: every ValueError is raised before anything touches the engine
# ---------------------------------------------------------------------------------------------------------------------
def _bare(cls, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def test_option_checks_need_no_device():
    from bayesgm_amd import causal_hmc as HM
    from bayesgm_amd.models.causalbgm import CausalBGM
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    data = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))
    assert HM.DEFAULT_TARGET == 0.75 and CausalBGM.hmc_row_step_ is None
    ok = _bare(CausalBGM)
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(n_leapfrog=2.5), "n_leapfrog"), (dict(step_size=0.0), "step_size"),
                     (dict(step_size=-0.1), "step_size"), (dict(target_acceptance_rate=0.0), "target_acceptance_rate"),
                     (dict(target_acceptance_rate=1.0), "target_acceptance_rate")):
        with pytest.raises(ValueError, match=word):
            ok.hmc_sampler(data, **kw)
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(row_adapt=True), "row_adapt"),
                     (dict(q_sd=None), "q_sd"), (dict(q_sd=-1.0), "q_sd")):
        with pytest.raises(ValueError, match=word):
            ok.predict(data, x_values=[0.0], sampler="hmc", **kw)
    with pytest.raises(ValueError, match="sampler"):
        ok.predict(data, x_values=[0.0], sampler="nuts")
    with pytest.raises(ValueError, match="x_values"):          # 'hmc' with good options goes on to the next argument check
        ok.predict(data, sampler="hmc")
    for prec in ("bf16x3", "f16x3"):
        m = _bare(CausalBGM)
        m._p["mh_precision"] = prec
        with pytest.raises(ValueError, match="mh_precision"):
            m.predict(data, x_values=[0.0], sampler="hmc")
        with pytest.raises(ValueError, match="mh_precision"):
            m.hmc_sampler(data)
    for cls in (IdentifiableCausalBGM, IdentifiableCausalBGMBayes):
        m = _bare(cls, n_segments=3)
        with pytest.raises(ValueError, match="IdentifiableCausalBGM"):
            m.predict(data, x_values=[0.0], sampler="hmc")
        with pytest.raises(ValueError, match="IdentifiableCausalBGM"):
            m.hmc_sampler(data)
    m = _bare(CausalBGMBayes)
    m._p["use_bnn"] = True
    with pytest.raises(ValueError, match="use_bnn"):
        m.predict(data, x_values=[0.0], sampler="hmc")
    with pytest.raises(ValueError, match="use_bnn"):
        m.hmc_sampler(data)
    # the row blocks of predict(sampler='hmc'): whole tiles within the budget
    assert HM.block_rows(3000, 10) == (2 << 30) // (4 * 3000 * 10) // 16 * 16
    assert HM.block_rows(100, 10, 4 * 100 * 10 * 40) == 32 and HM.block_rows(100, 10, 1) == 16
    with pytest.raises(ValueError, match="draw_budget_bytes"):
        HM.block_rows(100, 10, 0)


def test_abi_declares_the_entry_points():
    from bayesgm_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bgm_hip.h")).read()
    for name in ("bgm_causal_logpost_grad", "bgm_causal_hmc_run"):
        assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["bgm_causal_hmc_run"][1]) == 25 and len(_lib.SYMBOLS["bgm_causal_logpost_grad"][1]) == 9
