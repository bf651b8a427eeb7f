"""The diagonal metric of the CausalBGM HMC sampler on the GPU (csrc/causal_hmc_mass_kernels.h, bgm_causal_hmc_set_mass /
bgm_causal_hmc_mass_update) against the NumPy restatement (tests/_causal_hmc_mass_ref.py), and the properties that make it usable.

Bars:
  identity              mass_scale = 1 is the identity-mass kernel bit for bit on every output
  chains                those of tests/test_gpu_causal_hmc.py::test_chain_and_step_match_restatement: last draw within 1e-4 of the
                        float32 restatement on >= 97 % of the rows, steps bit-equal on those rows, acc_count[it] off by at most the
                        number of other rows; adapted scales within 1e-3 relative on those rows
  moments               |device - float64 sum of the kept draws| <= 1e-5 x (sum of |terms|): 40 float32 additions of bounded terms
  update                1e-6 relative against the rule in float64 from the device's own moments, 1e-3 from the draws
  same posterior        posterior means within 5 combined MCSE on >= 95 % of the series (test_same_target_as_row_adaptive_mh)
everything else is bit-identity."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _causal_hmc_mass_ref import hmc_mass_sampler  # noqa: E402
from _row_adapt_ref import concentrated_model, concentrated_panel  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
CASES = [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=200),         # the list of tests/test_gpu_causal_hmc.py
         dict(z_dims=[3, 3, 6, 6], p=100, binary=True, n=150),
         dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=40),
         dict(z_dims=[1, 1, 1, 7], p=50, binary=False, n=60),
         dict(z_dims=[2, 2, 2, 6], p=150, binary=True, n=50),
         dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=1),           # a single row
         dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=17)]          # a partial second tile
KEYS = ("draws", "state", "logp", "grad", "acc_count", "row_step")
WINDOWS = (6, [12, 20, 30])       # the tiny schedule: burn-in 36


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _rule64(W, s1, s2):
    """the update rule in NumPy float64 from [n x q] moments -> s [n x q] float64 (no chain of these tests has zero variance)"""
    mean = s1.astype(np.float64) / W
    var = np.maximum(s2.astype(np.float64) / W - mean * mean, 0.0)
    t = np.sqrt((W * var + 5e-3 * var.mean(axis=1, keepdims=True)) / (W + 5.0))
    return np.clip(t / np.exp(np.log(t).mean(axis=1, keepdims=True)), 0.05, 20.0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. unit scales are identity mass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[6]])
def test_unit_scales_are_identity_mass(torch, case):
    burn, keep, L, step0, seed = 12, 10, 3, 0.1, 99
    m = _model(31, case["z_dims"], case["p"], case["binary"])
    n, q = case["n"], sum(case["z_dims"])
    x, y, v = _data(n, case["p"], 32, case["binary"])
    eng = _engine(m)
    kw = dict(want_draws=True, adapt=TARGET)
    plain = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, **kw)
    assert "mass_scale" not in plain
    ones = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, mass_scale=torch.ones(n, q), **kw)
    for k in KEYS:
        assert torch.equal(plain[k], ones[k]), k
    assert torch.equal(ones["mass_scale"], torch.ones(n, q, device=ones["mass_scale"].device))
    twos = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, mass_scale=np.full((n, q), 2.0, np.float32), **kw)
    assert not torch.equal(twos["draws"], plain["draws"])          # the metric kernel reads its scales
    again = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, **kw)      # the setter was cleared: the plain call is unchanged
    for k in KEYS:
        assert torch.equal(plain[k], again[k]), k
    assert bool(torch.isfinite(plain["draws"]).all()) and int(plain["acc_count"].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the transition with a given metric against the float32 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES[:5])
def test_chain_with_a_given_metric_matches_restatement(torch, case):
    from bayesgm_amd.row_adapt import row_adapt_factors
    burn, keep, L, step0, seed = 15, 15, 3, 0.1, 1234567890123
    m = _model(21, case["z_dims"], case["p"], case["binary"])
    n, q = case["n"], sum(case["z_dims"])
    x, y, v = _data(n, case["p"], 22, case["binary"])
    scale = np.random.RandomState(23).uniform(0.3, 3.0, (n, q)).astype(np.float32)
    out = _engine(m).hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, chunk=7, adapt=TARGET, mass_scale=scale)
    draws, acc, step = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy().astype(np.int64), out["row_step"].cpu().numpy()
    up, dn = row_adapt_factors(burn, TARGET)
    ref = hmc_mass_sampler(m, (x, y, v), burn, keep, step0, L, seed, up, dn, scale=scale)
    assert draws.shape == ref["draws"].shape == (keep, n, q)
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    print("rows equal to the restatement: %.4f; acceptance %.3f; step q05 / median / q95 %.4f / %.4f / %.4f"
          % (row_ok.mean(), acc.sum() / float(acc.size * n), *np.quantile(step, [0.05, 0.5, 0.95])))
    assert row_ok.mean() >= 0.97, row_ok.mean()
    assert step.dtype == np.float32 and np.array_equal(step[row_ok], ref["step"][row_ok])
    assert np.ptp(step) > 0
    assert np.abs(acc - ref["acc"].sum(axis=1)).max() <= int((~row_ok).sum())
    assert np.array_equal(out["state"].cpu().numpy(), draws[-1]) and np.array_equal(out["mass_scale"].cpu().numpy(), scale)


# ---------------------------------------------------------------------------------------------------------------------
# 3. moments and update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[2], CASES[1]])
def test_moments_and_update(torch, case):
    """one window of 40 iterations run as RETAINED iterations (burn_in = 5 before it), so that its draws are kept"""
    burn, W, L, step0, seed = 5, 40, 3, 0.05, 4711
    m = _model(41, case["z_dims"], case["p"], case["binary"])
    n, q = case["n"], sum(case["z_dims"])
    x, y, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in _data(n, case["p"], 42, case["binary"]))
    x, y = x.reshape(-1), y.reshape(-1)
    eng = _engine(m)
    f = dict(device="cuda", dtype=torch.float32)
    state, grad, logp, step = torch.empty(n, q, **f), torch.empty(n, q, **f), torch.empty(n, **f), torch.full((n,), step0, **f)
    draws = torch.empty(W, n, q, **f)
    scale = torch.from_numpy(np.random.RandomState(43).uniform(0.5, 2.0, (n, q)).astype(np.float32)).cuda()
    scale0 = scale.clone()
    ref, s1, s2 = (torch.full((n, q), 7.0, **f) for _ in range(3))          # garbage: the W = 0 update resets it
    try:
        eng.set_hmc_mass(scale)
        eng.hmc_run(x, y, v, state, logp, grad, step, 0, burn, burn, L, seed, init=True)
        before = state.clone()
        eng.hmc_mass_update(0, state, scale, ref, s1, s2)
        assert torch.equal(ref, before) and torch.equal(scale, scale0) and not bool(s1.any()) and not bool(s2.any())
        eng.set_hmc_mass(scale, ref, s1, s2, accumulate=True)
        eng.hmc_run(x, y, v, state, logp, grad, step, burn, 17, burn, L, seed, draws=draws, n_keep=W)      # (cut inside the window)
        eng.hmc_run(x, y, v, state, logp, grad, step, burn + 17, W - 17, burn, L, seed, draws=draws, n_keep=W)
        assert torch.equal(ref, before) and torch.equal(state, draws[-1])
        d = draws.cpu().numpy().astype(np.float64) - before.cpu().numpy().astype(np.float64)[None]
        m1, m2 = s1.cpu().numpy(), s2.cpu().numpy()
        e1, e2 = np.abs(m1 - d.sum(axis=0)), np.abs(m2 - (d * d).sum(axis=0))
        b1, b2 = 1e-5 * np.abs(d).sum(axis=0), 1e-5 * (d * d).sum(axis=0)
        moved = np.abs(d).sum(axis=0) > 0
        print("moments: worst |S1 - float64| / bar %.3f, |S2 - float64| / bar %.3f; chains that moved %.3f"
              % ((e1[moved] / b1[moved]).max(), (e2[moved] / b2[moved]).max(), moved.all(axis=1).mean()))
        assert np.all(e1 <= b1) and np.all(e2 <= b2) and moved.all(axis=1).mean() > 0.9
        eng.hmc_mass_update(W, state, scale, ref, s1, s2)
    finally:
        eng.set_hmc_mass(None)
    s = scale.cpu().numpy()
    live = moved.all(axis=1)
    own, fresh = _rule64(W, m1[live], m2[live]), _rule64(W, d.sum(axis=0)[live], (d * d).sum(axis=0)[live])
    print("update: worst relative difference to the rule from the device's moments %.3g, from the draws %.3g; s min / median / max "
          "%.3f / %.3f / %.3f" % (np.abs(s[live] / own - 1).max(), np.abs(s[live] / fresh - 1).max(), s.min(), np.median(s), s.max()))
    assert s.dtype == np.float32 and np.abs(s[live] / own - 1).max() <= 1e-6 and np.abs(s[live] / fresh - 1).max() <= 1e-3
    assert np.array_equal(s[~live], scale0.cpu().numpy()[~live])            # a chain that never moved keeps its scales
    assert np.abs(np.exp(np.log(s[live].astype(np.float64)).mean(axis=1)) - 1).max() <= 1e-5
    assert torch.equal(ref, state) and not bool(s1.any()) and not bool(s2.any())
    host = HM.mass_update(W, state.cpu().numpy(), scale0.cpu().numpy(), None, m1, m2)[0]      # the package's own statement of the rule
    assert np.abs(s / host - 1).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 4. segments and row subsets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[6]])
def test_windows_are_launch_boundaries_and_rows_are_independent(torch, case):
    burn, keep, L, step0, seed = 36, 8, 2, 0.1, 99
    m = _model(31, case["z_dims"], case["p"], case["binary"])
    n = case["n"]
    x, y, v = _data(n, case["p"], 32, case["binary"])
    eng = _engine(m)
    kw = dict(want_draws=True, adapt=TARGET, mass="diag", mass_windows=WINDOWS)
    full = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, **kw)
    for chunk in (5, 1):
        cut = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, chunk=chunk, **kw)
        for k in KEYS + ("mass_scale",):
            assert torch.equal(full[k], cut[k]), (k, chunk)
    s = full["mass_scale"].cpu().numpy()
    assert s.shape == (n, sum(case["z_dims"])) and np.all(np.isfinite(s)) and (np.ptp(s, axis=1) > 0).mean() > 0.5
    assert bool(torch.isfinite(full["draws"]).all()) and int(full["acc_count"].sum()) > 0
    plain = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt=TARGET)
    assert not torch.equal(plain["draws"], full["draws"])
    # rows [s, e) alone, starting inside a tile, with row_base = s
    a, e = (5, n) if n < 64 else (23, 71)
    part = eng.hmc_sample(x[a:e], y[a:e], v[a:e], burn, keep, step0, L, seed, row_base=a, **kw)
    assert torch.equal(full["draws"][:, a:e], part["draws"]) and torch.equal(full["row_step"][a:e], part["row_step"])
    assert torch.equal(full["logp"][a:e], part["logp"]) and torch.equal(full["grad"][a:e], part["grad"])
    assert torch.equal(full["mass_scale"][a:e], part["mass_scale"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the whole adaptive run against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES[:3])
def test_adaptive_run_matches_restatement(torch, case):
    burn, keep, L, step0, seed = 36, 8, 2, 0.1, 1234567890123
    m = _model(21, case["z_dims"], case["p"], case["binary"])
    n = case["n"]
    x, y, v = _data(n, case["p"], 22, case["binary"])
    out = _engine(m).hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt=TARGET, mass="diag", mass_windows=WINDOWS)
    (start, ends), (up, dn) = HM.mass_schedule(burn, TARGET, WINDOWS)
    ref = hmc_mass_sampler(m, (x, y, v), burn, keep, step0, L, seed, up, dn, windows=(start, ends))
    draws, s = out["draws"].cpu().numpy(), out["mass_scale"].cpu().numpy()
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    rel = np.abs(s[row_ok] / ref["scale"][row_ok] - 1)
    print("rows equal to the restatement: %.4f; worst relative difference of their scales %.3g; s q05 / median / q95 %.3f / %.3f / %.3f"
          % (row_ok.mean(), rel.max(), *np.quantile(s, [0.05, 0.5, 0.95])))
    assert row_ok.mean() >= 0.97, row_ok.mean()
    assert rel.max() <= 1e-3
    assert np.array_equal(out["row_step"].cpu().numpy()[row_ok], ref["step"][row_ok])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the metric leaves the posterior alone
# ---------------------------------------------------------------------------------------------------------------------
def test_same_posterior_as_identity_mass(torch):
    """The concentrated panel, 500 + 1500 transitions, L = 5.  Identity HMC against identity HMC under two seeds is printed first: the
    bar must be comfortable for that pair before it can say anything about the metric."""
    from bayesgm_amd.diagnostics import chain_diagnostics
    z_dims, p, n, burn, keep, L = [3, 3, 3, 1], 50, 64, 500, 1500, 5
    m = concentrated_model(0, z_dims, p)
    x, y, v = concentrated_panel(m, n, 1)
    eng = _engine(m)

    def share(da, db, what):
        live = (da.sd > 0) & (db.sd > 0) & np.isfinite(da.mcse) & np.isfinite(db.mcse)
        assert live.mean() > 0.9
        zs = np.abs(da.mean - db.mean)[live] / np.sqrt(da.mcse[live] ** 2 + db.mcse[live] ** 2)
        print("%s: |difference of posterior means| / combined MCSE median %.2f, max %.2f, within 5: %.4f" % (what, np.median(zs), zs.max(), (zs <= 5).mean()))
        return (zs <= 5.0).mean()

    def report(out, d, what):
        print("%s: ESS median %.1f, 1 %% quantile %.1f; acceptance %.3f; step median %.4f"
              % (what, np.median(d.ess), np.quantile(d.ess, 0.01), float(out["acc_count"][burn:].sum()) / (keep * n), float(out["row_step"].median())))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ident = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, 11, want_draws=True, adapt=TARGET)
        other = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, 12, want_draws=True, adapt=TARGET)
        diag = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, 11, want_draws=True, adapt=TARGET, mass="diag")
        di, do, dd = (chain_diagnostics(o["draws"]) for o in (ident, other, diag))
    report(ident, di, "identity mass")
    report(diag, dd, "mass='diag'  ")
    s = diag["mass_scale"].cpu().numpy()
    print("per-coordinate median of s: " + " ".join("%.3f" % t for t in np.median(s, axis=0)))
    base = share(di, do, "identity against identity, two seeds")
    got = share(dd, di, "mass='diag' against identity")
    assert base >= 0.95                                      # (else the chains are too short for the bar: lengthen them)
    assert got >= 0.95
    assert (np.ptp(s, axis=1) > 0).mean() > 0.9 and np.abs(np.log(s.astype(np.float64)).mean(axis=1)).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 7. the class surface
# ---------------------------------------------------------------------------------------------------------------------
Z_DIMS, P = [3, 3, 3, 1], 50


def _causal(tmp_path, m, binary=False, seed=3, **kw):
    from bayesgm_amd.models import CausalBGM
    params = dict(dataset="t", output_dir=str(tmp_path), save_res=False, save_model=False, binary_treatment=binary, use_bnn=False,
                  z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
                  e_units=[64] * 5, dz_units=[64, 32, 8], kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, mixing_check=False, **kw)
    model = CausalBGM(params, random_seed=seed)
    model.set_weights(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
    return model


def _seed_of(model):
    return (model._base_seed * 1000003 + model._seed_counter) & 0x7FFFFFFFFFFFFFFF


def test_class_surface(torch, tmp_path):
    m = OC.init_model(0, Z_DIMS, P)
    n, burn, keep, q = 200, 30, 20, sum(Z_DIMS)
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    xs = np.linspace(0.0, 3.0, 5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = _causal(tmp_path, m)
        draws = a.hmc_sampler(data, n_keep=keep, burn_in=burn, step_size=0.1, n_leapfrog=3, mass="diag")
        assert draws.shape == (keep, n, q) and a.hmc_row_mass_.shape == (n, q) and a.hmc_row_mass_.dtype == np.float32
        ref = a.engine.hmc_sample(x, y, v, burn, keep, 0.1, 3, _seed_of(a), want_draws=True, adapt=TARGET, mass="diag")
        assert np.array_equal(ref["draws"].cpu().numpy(), draws) and np.array_equal(ref["mass_scale"].cpu().numpy(), a.hmc_row_mass_)
        assert np.array_equal(ref["row_step"].cpu().numpy(), a.hmc_row_step_) and (np.ptp(a.hmc_row_mass_, axis=1) > 0).mean() > 0.5
        a.hmc_sampler(data, n_keep=keep, burn_in=burn, step_size=0.1, n_leapfrog=3)
        assert a.hmc_row_mass_ is None
        # predict: the same under two draw budgets, and with and without diagnose_rows
        kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, x_values=xs, verbose=0, sampler="hmc", step_size=0.1, n_leapfrog=3)
        b, c, d = _causal(tmp_path, m), _causal(tmp_path, m), _causal(tmp_path, m)
        eff_b, int_b = b.predict(data, mass="diag", diagnose_rows=32, **kw)
        eff_d, int_d = d.predict(data, mass="diag", **kw)
        assert np.array_equal(eff_b, eff_d) and np.array_equal(int_b, int_d) and np.array_equal(b.hmc_row_mass_, d.hmc_row_mass_)
        assert b.mcmc_diagnostics_.rows.shape == (32,) and d.mcmc_diagnostics_ is None and b._seed_counter == d._seed_counter
        eff_c, int_c = c.predict(data, mass="diag", draw_budget_bytes=4 * keep * q * 48, **kw)      # 48-row blocks
        assert np.array_equal(b.hmc_row_mass_, c.hmc_row_mass_) and np.array_equal(b.hmc_row_step_, c.hmc_row_step_)
        assert b.hmc_row_mass_.shape == (n, q) and (np.ptp(b.hmc_row_mass_, axis=1) > 0).mean() > 0.5
        out = b.engine.hmc_sample(x, y, v, burn, keep, 0.1, 3, _seed_of(b), want_draws=True, adapt=TARGET, mass="diag")
        assert np.array_equal(b.hmc_row_mass_, out["mass_scale"].cpu().numpy())
        # (the ADRF sums of several blocks are reassociated: the bound of tests/test_gpu_causal_hmc.py)
        bound = n * 2.0 ** -24 * float(out["draws"].abs().max())
        assert np.abs(eff_c - eff_b).max() <= bound and np.abs(int_c - int_b).max() <= bound, (np.abs(eff_c - eff_b).max(), bound)
        # the diagnosed chains are predict's chains
        rows = b.mcmc_diagnostics_.rows
        from bayesgm_amd.diagnostics import chain_diagnostics
        assert np.array_equal(b.mcmc_diagnostics_.mean, chain_diagnostics(out["draws"][:, torch.from_numpy(rows).cuda()]).mean)
        # without mass: the identity-mass call
        e, f = _causal(tmp_path, m), _causal(tmp_path, m)
        eff_e, int_e = e.predict(data, **kw)
        eff_f, int_f = f.predict(data, mass="identity", **kw)
    assert np.array_equal(eff_e, eff_f) and np.array_equal(int_e, int_f) and e.hmc_row_mass_ is None and f.hmc_row_mass_ is None
    assert np.array_equal(e.hmc_row_step_, f.hmc_row_step_) and not np.array_equal(eff_e, eff_b)


def test_binary_predict_with_a_metric_does_not_depend_on_the_draw_budget(torch, tmp_path):
    m = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    n, burn, keep = 150, 30, 20
    data = _data(n, P, 8, True)
    kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, verbose=0, sampler="hmc", step_size=0.1, n_leapfrog=3, mass="diag")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c = _causal(tmp_path, m, True), _causal(tmp_path, m, True), _causal(tmp_path, m, True)
        ite_a, int_a = a.predict(data, **kw)
        ite_b, int_b = b.predict(data, draw_budget_bytes=4 * keep * sum(Z_DIMS) * 32, **kw)      # 32-row blocks
        ite_c, int_c = c.predict(data, diagnose_rows=16, **kw)
    assert ite_a.shape == (n,) and int_a.shape == (n, 2) and np.all(np.isfinite(ite_a))
    assert np.array_equal(ite_a, ite_b) and np.array_equal(int_a, int_b) and np.array_equal(a.hmc_row_mass_, b.hmc_row_mass_)
    assert np.array_equal(ite_a, ite_c) and np.array_equal(int_a, int_c) and np.array_equal(a.hmc_row_mass_, c.hmc_row_mass_)


def test_metric_refusals(torch):
    """the entry points refuse what bgm_causal_logpost_grad refuses, and the argument checks of hmc_sample"""
    x, y, v = _data(40, 20, 52)
    m = _model(51, [1, 1, 1, 7], 20)
    eng = _engine(m)
    ones = torch.ones(40, 10, device="cuda")
    eng.set_precision("f16x3")
    with pytest.raises(RuntimeError, match=r"\(-4\).*split-precision"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, mass_scale=ones)
    with pytest.raises(RuntimeError, match=r"\(-4\).*split-precision"):
        eng.hmc_mass_update(0, ones, ones.clone(), ones.clone(), ones.clone(), ones.clone())
    eng.set_precision("fp32")
    mw = _model(53, [1, 1, 1, 7], 20, g_units=(32, 32), f_units=(32, 8), h_units=(32, 8))
    with pytest.raises(RuntimeError, match=r"\(-4\).*general-width engine"):
        _engine(mw, g_units=[32, 32], f_units=[32, 8], h_units=[32, 8]).hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, mass_scale=ones)
    with pytest.raises(RuntimeError, match="accumulate needs"):
        eng.set_hmc_mass(ones, None, None, None, accumulate=True)
    eng.set_hmc_mass(None)
    for bad, word in ((dict(mass="dense"), "mass must be"), (dict(mass="diag", adapt=None), "adapt"), (dict(mass="diag"), "burn_in"),
                      (dict(mass="diag", mass_scale=ones), "mass_scale"), (dict(mass_scale=ones[:, :9]), "mass_scale"),
                      (dict(mass="diag", mass_windows=(0, [3])), "mass_windows")):
        with pytest.raises(ValueError, match=word):
            eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, **bad)
    out = eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7)              # the refusals left the handle usable, on identity mass
    assert out["row_step"].shape == (40,) and "mass_scale" not in out


# ---------------------------------------------------------------------------------------------------------------------
# 8. the second trip of the tile loop
# ---------------------------------------------------------------------------------------------------------------------
def test_metric_beyond_one_trip_of_the_tile_loop(torch):
    """The smallest model with more 16-row tiles than wave slots, a ragged last tile, burn-in 20 (the least mass='diag' accepts): the
    full run against three runs over a partition of the rows, each within one trip and with its own row_base, bit for bit."""
    burn, keep, L, step0, seed = 20, 2, 2, 0.1, 4242
    m = _model(65, [1, 1, 1, 7], 20)
    eng = _engine(m)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus + 17
    slots = eng.mh_slots(n)
    assert waves == 8 and slots == waves * n_cus and (n + 15) // 16 > slots
    x, y, v = _data(n, 20, 66)
    kw = dict(want_draws=True, adapt=TARGET, mass="diag", mass_windows=(6, [12, 18]))
    full = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, **kw)
    cuts = [0, n // 3 // 16 * 16 + 7, 2 * n // 3 // 16 * 16, n]
    assert cuts[1] % 16 != 0 and all((e - s + 15) // 16 <= slots for s, e in zip(cuts[:-1], cuts[1:]))
    parts = [eng.hmc_sample(x[s:e], y[s:e], v[s:e], burn, keep, step0, L, seed, row_base=s, **kw) for s, e in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(full["draws"], torch.cat([p["draws"] for p in parts], dim=1))
    for k in ("state", "logp", "grad", "row_step", "mass_scale"):
        assert torch.equal(full[k], torch.cat([p[k] for p in parts], dim=0)), k
    assert torch.equal(full["acc_count"], sum(p["acc_count"] for p in parts))
    assert bool(torch.isfinite(full["draws"]).all()) and 0 < int(full["acc_count"].sum()) < (burn + keep) * n
    s = full["mass_scale"]
    assert bool(torch.isfinite(s).all()) and float((s.max(dim=1).values > s.min(dim=1).values).float().mean()) > 0.9
