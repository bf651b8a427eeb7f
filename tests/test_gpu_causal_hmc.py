"""The HMC latent sampler of CausalBGM on the GPU (csrc/causal_hmc_kernels.h, bgm_causal_logpost_grad / bgm_causal_hmc_run) against the
NumPy restatement (tests/_causal_hmc_ref.py), and the properties that make it usable.

Bars (all taken from tests that check the same quantity elsewhere in the project):
  log posterior         |hip - float64| <= 2e-6 |ref| + 2e-4          the Gram-form bar of tests/test_gpu_mh_gram_likelihood.py
  gradient              |hip - float64| <= 5e-5 max|grad of the row|   the bar of the BGM HMC gradient, tests/test_gpu_bgm.py
  chains                last draw within 1e-4 of the float32 restatement on >= 97 % of the rows (the BGM HMC bar); on those rows the
                        step equals the restatement's bit for bit; acc_count[it] differs by at most the number of other rows.
                        The float32 restatement against the float64 one on the same five cases (CPU, 15 + 15 transitions, L = 3,
                        adaptation on): 100 % of the rows equal on every case, so the 98.5 % the cap rests on holds.
  same target as MH     posterior means within 5 combined MCSE on >= 95 % of the non-constant series
everything else is bit-identity."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _causal_hmc_ref import hmc_sampler, log_posterior_and_grad  # noqa: E402
from _row_adapt_ref import concentrated_model, concentrated_panel  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
CASES = [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=200),
         dict(z_dims=[3, 3, 6, 6], p=100, binary=True, n=150),
         dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=40),
         dict(z_dims=[1, 1, 1, 7], p=50, binary=False, n=60),
         dict(z_dims=[2, 2, 2, 6], p=150, binary=True, n=50),
         dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=1),           # a single row
         dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=17)]          # a partial second tile


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _table(burn, target=TARGET):
    from bayesgm_amd.row_adapt import row_adapt_factors
    return row_adapt_factors(burn, target)


def _ref64(m, x, y, v, z):
    return log_posterior_and_grad(OC.cast_model(m, np.float64), *(a.astype(np.float64) for a in (x, y, v, z)))


def _check_logp_grad(lp, gr, ref_lp, ref_gr, what):
    err = np.abs(lp - ref_lp)
    gmax = np.abs(ref_gr).max(axis=1)
    gerr = np.abs(gr - ref_gr).max(axis=1)
    print("%s: worst |logp - float64| / bar %.3f, worst |grad - float64| / (5e-5 max|grad|) %.3f"
          % (what, (err / (2e-6 * np.abs(ref_lp) + 2e-4)).max(), (gerr / (5e-5 * gmax)).max()))
    assert np.all(err <= 2e-6 * np.abs(ref_lp) + 2e-4), (err.max(), np.abs(ref_lp).max())
    assert np.all(gerr <= 5e-5 * gmax), (gerr / gmax).max()


# ---------------------------------------------------------------------------------------------------------------------
# 1. log posterior and gradient against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("fixed", [False, True])
def test_logpost_grad_matches_float64(torch, case, fixed):
    kw = dict(sigma_v=0.8, sigma_x=1.3, sigma_y=0.5) if fixed else {}
    m = _model(1, case["z_dims"], case["p"], case["binary"], **kw)
    x, y, v = _data(case["n"], case["p"], 2, case["binary"])
    z = np.random.RandomState(3).randn(case["n"], sum(case["z_dims"])).astype(np.float32)
    eng = _engine(m)
    lp, gr = eng.logpost_grad(x.ravel(), y.ravel(), v, z)
    assert lp.shape == (case["n"],) and gr.shape == z.shape
    _check_logp_grad(lp.cpu().numpy(), gr.cpu().numpy(), *_ref64(m, x, y, v, z), "p = %d, n = %d" % (case["p"], case["n"]))
    # the value is the one bgm_causal_logpost computes (Gram or direct form), within twice the bar both meet
    lp0 = eng.logpost(x.ravel(), y.ravel(), v, z)
    assert bool(torch.all((lp - lp0).abs() <= 2 * (2e-6 * lp0.abs() + 2e-4)))


def test_logpost_grad_on_the_gram_stress_model(torch):
    """|v| >> |residual| (tests/test_gpu_mh_gram_likelihood.py: output bias offset by 5, v = g(z*) + N(0, 0.05^2), sigma_v = 0.05),
    evaluated near z*.  The log posterior keeps the Gram-form bar.  The gradient is checked against 5e-5 max|grad| and, where that does
    not hold, against 4 x the difference between the float32 and the float64 restatement on the same inputs; both ratios are printed."""
    from oracle.nets import mlp_forward
    z_dims, p, n = [1, 1, 1, 7], 200, 256
    m = _model(41, z_dims, p, False, sigma_v=0.05)
    W, b = m["g"][-1]
    m["g"][-1] = (W, (b + 5.0).astype(np.float32))
    rs = np.random.RandomState(42)
    zs = rs.randn(n, sum(z_dims))
    v = (mlp_forward(OC.cast_model(m, np.float64)["g"], zs)[:, :p] + 0.05 * rs.randn(n, p)).astype(np.float32)
    x, y, _ = _data(n, p, 43)
    z = (zs + 0.02 * rs.randn(*zs.shape)).astype(np.float32)
    lp, gr = _engine(m).logpost_grad(x.ravel(), y.ravel(), v, z)
    lp, gr = lp.cpu().numpy(), gr.cpu().numpy()
    ref_lp, ref_gr = _ref64(m, x, y, v, z)
    _, gr32 = log_posterior_and_grad(m, x, y, v, z)
    err = np.abs(lp - ref_lp)
    assert np.all(err <= 2e-6 * np.abs(ref_lp) + 2e-4), (err.max(), np.abs(ref_lp).max())
    gmax = np.abs(ref_gr).max(axis=1)
    gerr = np.abs(gr - ref_gr).max(axis=1)
    r32 = np.abs(gr32.astype(np.float64) - ref_gr).max(axis=1)
    print("stress model: worst |grad - float64| / (5e-5 max|grad|) %.3f; float32 restatement / same %.3f; worst |grad - float64| / "
          "|restatement32 - float64| %.3f; median max|grad| %.3g"
          % ((gerr / (5e-5 * gmax)).max(), (r32 / (5e-5 * gmax)).max(), (gerr / np.maximum(r32, 1e-30)).max(), np.median(gmax)))
    assert np.all(gerr <= np.maximum(5e-5 * gmax, 4.0 * r32)), (gerr / gmax).max()


# ---------------------------------------------------------------------------------------------------------------------
# 2. chains against the float32 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES[:5])
def test_chain_and_step_match_restatement(torch, case):
    burn, keep, L, step0, seed = 15, 15, 3, 0.1, 1234567890123
    m = _model(21, case["z_dims"], case["p"], case["binary"])
    x, y, v = _data(case["n"], case["p"], 22, case["binary"])
    eng = _engine(m)
    out = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, chunk=7, adapt=TARGET)      # odd chunking on purpose
    draws, acc, step = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy().astype(np.int64), out["row_step"].cpu().numpy()
    up, dn = _table(burn)
    ref = hmc_sampler(m, (x, y, v), burn, keep, step0, L, seed, up, dn)
    assert draws.shape == ref["draws"].shape == (keep, case["n"], sum(case["z_dims"]))
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    print("rows equal to the restatement: %.4f; acceptance %.3f; step q05 / median / q95 %.4f / %.4f / %.4f"
          % (row_ok.mean(), acc.sum() / float(acc.size * case["n"]), *np.quantile(step, [0.05, 0.5, 0.95])))
    assert row_ok.mean() >= 0.97, row_ok.mean()
    assert step.dtype == np.float32 and np.array_equal(step[row_ok], ref["step"][row_ok])
    assert np.ptp(step) > 0
    assert np.abs(acc - ref["acc"].sum(axis=1)).max() <= int((~row_ok).sum())
    assert np.array_equal(out["state"].cpu().numpy(), draws[-1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. bit identities, 4. cached values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[6]])
def test_bit_identities_and_cached_values(torch, case):
    burn, keep, L, step0, seed = 12, 10, 3, 0.1, 99
    m = _model(31, case["z_dims"], case["p"], case["binary"])
    n = case["n"]
    x, y, v = _data(n, case["p"], 32, case["binary"])
    eng = _engine(m)
    keys = ("draws", "state", "logp", "grad", "acc_count", "row_step")
    full = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt=TARGET)
    again = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt=TARGET)
    cut = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt=TARGET, chunk=5)
    one = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt=TARGET, chunk=1)
    for k in keys:
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(full[k], cut[k]), k
        assert torch.equal(full[k], one[k]), k
    assert bool(torch.isfinite(full["draws"]).all()) and int(full["acc_count"].sum()) > 0
    # rows [s, e) alone, starting inside a tile, with row_base = s
    s, e = (5, n) if n < 64 else (23, 71)
    part = eng.hmc_sample(x[s:e], y[s:e], v[s:e], burn, keep, step0, L, seed, want_draws=True, adapt=TARGET, row_base=s)
    assert torch.equal(full["draws"][:, s:e], part["draws"]) and torch.equal(full["row_step"][s:e], part["row_step"])
    assert torch.equal(full["logp"][s:e], part["logp"]) and torch.equal(full["grad"][s:e], part["grad"])
    # a neutral table is the fixed-step run
    ones = np.ones(burn, np.float32)
    fixed = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt=None)
    neutral = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, want_draws=True, adapt_table=(ones, ones))
    for k in keys:
        assert torch.equal(fixed[k], neutral[k]), k
    assert bool(torch.all(fixed["row_step"] == float(np.float32(step0)))) and not torch.equal(fixed["draws"], full["draws"])
    # the cached log posterior and gradient are those of the final state
    lp, gr = eng.logpost_grad(x.ravel(), y.ravel(), v, full["state"])
    _check_logp_grad(full["logp"].cpu().numpy(), full["grad"].cpu().numpy(), lp.cpu().numpy().astype(np.float64), gr.cpu().numpy().astype(np.float64), "cached / fresh")
    _check_logp_grad(full["logp"].cpu().numpy(), full["grad"].cpu().numpy(), *_ref64(m, x, y, v, full["state"].cpu().numpy()), "cached")


# ---------------------------------------------------------------------------------------------------------------------
# 5. HMC and row-adaptive MH sample the same posterior
# ---------------------------------------------------------------------------------------------------------------------
def test_same_target_as_row_adaptive_mh(torch):
    from bayesgm_amd.diagnostics import chain_diagnostics
    z_dims, p, n = [3, 3, 3, 1], 50, 64
    m = concentrated_model(0, z_dims, p)
    x, y, v = concentrated_panel(m, n, 1)
    eng = _engine(m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hmc = eng.hmc_sample(x, y, v, 500, 1500, 0.1, 5, 11, want_draws=True, adapt=TARGET)
        mh = eng.mh_sample(x, y, v, 2000, 6000, 1.0, 11, want_draws=True, row_adapt=0.25)
        dh, dm = chain_diagnostics(hmc["draws"]), chain_diagnostics(mh["draws"])
    print("ESS median: HMC (1500 draws, L = 5) %.1f, row-adaptive MH (6000 draws) %.1f; HMC acceptance %.3f, step median %.4f"
          % (np.median(dh.ess), np.median(dm.ess), float(hmc["acc_count"][500:].sum()) / (1500 * n), float(hmc["row_step"].median())))
    live = (dh.sd > 0) & (dm.sd > 0) & np.isfinite(dh.mcse) & np.isfinite(dm.mcse)
    assert live.mean() > 0.9
    zscore = np.abs(dh.mean - dm.mean)[live] / np.sqrt(dh.mcse[live] ** 2 + dm.mcse[live] ** 2)
    print("posterior means: |difference| / combined MCSE median %.2f, max %.2f, within 5: %.4f" % (np.median(zscore), zscore.max(), (zscore <= 5).mean()))
    assert (zscore <= 5.0).mean() >= 0.95


# ---------------------------------------------------------------------------------------------------------------------
# 6. the class surface
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


def test_class_sampler_and_continuous_predict(torch, tmp_path):
    m = OC.init_model(0, Z_DIMS, P)
    n, burn, keep = 200, 30, 20
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    xs = np.linspace(0.0, 3.0, 5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = _causal(tmp_path, m)
        draws = a.hmc_sampler(data, n_keep=keep, burn_in=burn, step_size=0.1, n_leapfrog=3, diagnostics=True)
        assert draws.shape == (keep, n, sum(Z_DIMS)) and a.hmc_row_step_.shape == (n,) and a.hmc_row_step_.dtype == np.float32
        assert a.mcmc_diagnostics_ is not None and a.mcmc_diagnostics_.ess.shape == (n, sum(Z_DIMS))
        ref = a.engine.hmc_sample(x, y, v, burn, keep, 0.1, 3, _seed_of(a), want_draws=True, adapt=TARGET)
        assert np.array_equal(ref["draws"].cpu().numpy(), draws) and np.array_equal(ref["row_step"].cpu().numpy(), a.hmc_row_step_)
        # predict: one block = engine.effects on hmc_sample's draws, bit for bit; several blocks within the reassociation bound
        kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, x_values=xs, verbose=0, sampler="hmc", step_size=0.1, n_leapfrog=3)
        b, c, d = _causal(tmp_path, m), _causal(tmp_path, m), _causal(tmp_path, m)
        eff_b, int_b = b.predict(data, **kw)
        eff_c, int_c = c.predict(data, draw_budget_bytes=4 * keep * sum(Z_DIMS) * 48, diagnose_rows=32, **kw)      # 48-row blocks
        out = b.engine.hmc_sample(x, y, v, burn, keep, 0.1, 3, _seed_of(b), want_draws=True, adapt=TARGET)
        adrf = b.engine.effects(x, out["draws"], burn, _seed_of(b), x_values=xs, sample_y=True)
        sums = (adrf.double() * float(n) / float(n)).float().contiguous()
        want, lo, hi = b.engine.row_mean_quantiles(sums, 0.025, 0.975)
        assert np.array_equal(eff_b, want.cpu().numpy()) and np.array_equal(int_b, torch.stack([lo, hi], dim=1).cpu().numpy())
        assert np.array_equal(b.hmc_row_step_, out["row_step"].cpu().numpy()) and np.array_equal(c.hmc_row_step_, b.hmc_row_step_)
        bound = n * 2.0 ** -24 * float(out["draws"].abs().max())
        assert np.abs(eff_c - eff_b).max() <= bound and np.abs(int_c - int_b).max() <= bound, (np.abs(eff_c - eff_b).max(), bound)
        assert b.mh_row_scale_ is None and b.mcmc_diagnostics_ is None
        assert c.mcmc_diagnostics_.rows.shape == (32,) and b._seed_counter == c._seed_counter
        # 'mh' is the call without the argument
        eff_d, int_d = d.predict(data, alpha=0.05, n_mcmc=keep, burn_in=burn, x_values=xs, verbose=0, sampler="mh")
        eff_e, int_e = _causal(tmp_path, m).predict(data, alpha=0.05, n_mcmc=keep, burn_in=burn, x_values=xs, verbose=0)
    assert np.array_equal(eff_d, eff_e) and np.array_equal(int_d, int_e) and d.hmc_row_step_ is None
    assert not np.array_equal(eff_d, eff_b)


def test_binary_predict_does_not_depend_on_the_draw_budget(torch, tmp_path):
    m = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    n, burn, keep = 150, 30, 20
    data = _data(n, P, 8, True)
    kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, verbose=0, sampler="hmc", step_size=0.1, n_leapfrog=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = _causal(tmp_path, m, True), _causal(tmp_path, m, True)
        ite_a, int_a = a.predict(data, **kw)
        ite_b, int_b = b.predict(data, draw_budget_bytes=4 * keep * sum(Z_DIMS) * 32, **kw)      # 32-row blocks
    assert ite_a.shape == (n,) and int_a.shape == (n, 2) and np.all(np.isfinite(ite_a))
    assert np.array_equal(ite_a, ite_b) and np.array_equal(int_a, int_b) and np.array_equal(a.hmc_row_step_, b.hmc_row_step_)


def test_unsupported_paths_refuse(torch):
    from oracle import identifiable as OI
    x, y, v = _data(40, 20, 52)
    m = _model(51, [1, 1, 1, 7], 20)
    z = np.zeros((40, 10), np.float32)
    calls = (lambda eng, *d: eng.hmc_sample(*(d or (x, y, v)), 5, 5, 0.1, 2, 7), lambda eng, *d: eng.logpost_grad(*(d or (x, y, v)), z))
    eng = _engine(m)
    for run in calls:
        for mode in ("bf16x3", "f16x3"):
            eng.set_precision(mode)
            with pytest.raises(RuntimeError, match=r"\(-4\).*split-precision"):
                run(eng)
        eng.set_precision("fp32")
        rs = np.random.RandomState(33)
        pn = OI.init_prior_net(rs, 5, 10)
        eng.set_prior(torch.from_numpy(rs.randint(0, 5, 40).astype(np.int32)).cuda(), torch.from_numpy(OI.prior_table(pn, 10)).cuda())
        with pytest.raises(RuntimeError, match=r"\(-4\).*conditional latent prior"):
            run(eng)
        eng.set_prior(None, None)
        mw = _model(53, [1, 1, 1, 7], 20, g_units=(32, 32), f_units=(32, 8), h_units=(32, 8))
        with pytest.raises(RuntimeError, match=r"\(-4\).*general-width engine"):
            run(_engine(mw, g_units=[32, 32], f_units=[32, 8], h_units=[32, 8]))
        mp = _model(54, [1, 1, 1, 7], 300)
        with pytest.raises(RuntimeError, match=r"\(-4\).*streamed-fragment"):
            run(_engine(mp), *_data(40, 300, 55))
    assert eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7)["row_step"].shape == (40,)          # the refusals left the handle usable
    for bad in (dict(step_size=0.0), dict(n_leapfrog=0), dict(adapt=1.0)):
        with pytest.raises(ValueError):
            eng.hmc_sample(x, y, v, 5, 5, **dict(dict(step_size=0.1, n_leapfrog=2, seed=7), **bad))


# ---------------------------------------------------------------------------------------------------------------------
# 7. the second trip of the tile loop: more 16-row tiles than wave slots (the grid is capped at one workgroup per CU)
# ---------------------------------------------------------------------------------------------------------------------
def _two_trip_panel(torch, seed):
    """the smallest model and n = 16 * waves * n_cus + 17 rows: every wave slot takes one tile, the first of them a second one, the last
    tile is ragged.  Returns (engine, model, x, y, v, n, wave slots)."""
    m = _model(seed, [1, 1, 1, 7], 20)
    eng = _engine(m)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus + 17
    slots = eng.mh_slots(n)                                   # grid * waves of bgm_causal_grid: the grid of the HMC kernels too
    assert waves == 8 and slots == waves * n_cus
    assert (n + 15) // 16 > slots                             # more tiles than wave slots: the loop takes a second trip
    x, y, v = _data(n, 20, seed + 1)
    return eng, m, x, y, v, n, slots


def test_logpost_grad_beyond_one_trip_of_the_tile_loop(torch):
    eng, m, x, y, v, n, slots = _two_trip_panel(torch, 61)
    z = np.random.RandomState(63).randn(n, 10).astype(np.float32)
    lp, gr = eng.logpost_grad(x.ravel(), y.ravel(), v, z)
    assert lp.shape == (n,) and gr.shape == (n, 10)
    _check_logp_grad(lp.cpu().numpy(), gr.cpu().numpy(), *_ref64(m, x, y, v, z), "p = 20, n = %d (%d tiles, %d wave slots)" % (n, (n + 15) // 16, slots))
    for s, e in ((0, 64), (n - 64, n)):                       # first-trip rows and second-trip rows (ragged tile included) alone
        assert (e - s + 15) // 16 <= slots
        lp1, gr1 = eng.logpost_grad(x[s:e].ravel(), y[s:e].ravel(), v[s:e], z[s:e])
        assert torch.equal(lp[s:e], lp1) and torch.equal(gr[s:e], gr1), (s, e)


def test_hmc_beyond_one_trip_of_the_tile_loop(torch):
    """The full run against three runs over a partition of the rows, each within one trip, each with its own row_base, the first
    boundary inside a tile: bit for bit (test_bit_identities_and_cached_values establishes the piecewise identity at small n)."""
    burn, keep, L, step0, seed = 3, 2, 2, 0.1, 4242
    eng, m, x, y, v, n, slots = _two_trip_panel(torch, 65)
    kw = dict(want_draws=True, adapt=TARGET)
    full = eng.hmc_sample(x, y, v, burn, keep, step0, L, seed, **kw)
    cuts = [0, n // 3 // 16 * 16 + 7, 2 * n // 3 // 16 * 16, n]
    assert cuts[1] % 16 != 0 and all((e - s + 15) // 16 <= slots for s, e in zip(cuts[:-1], cuts[1:]))
    parts = [eng.hmc_sample(x[s:e], y[s:e], v[s:e], burn, keep, step0, L, seed, row_base=s, **kw) for s, e in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(full["draws"], torch.cat([p["draws"] for p in parts], dim=1))
    for k in ("state", "logp", "grad", "row_step"):
        assert torch.equal(full[k], torch.cat([p[k] for p in parts], dim=0)), k
    assert torch.equal(full["acc_count"], sum(p["acc_count"] for p in parts))
    assert bool(torch.isfinite(full["draws"]).all()) and 0 < int(full["acc_count"].sum()) < (burn + keep) * n
    assert float(full["row_step"].min()) < float(full["row_step"].max())
