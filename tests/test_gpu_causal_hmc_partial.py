"""Partially observed rows on the GPU (csrc/causal_hmc_obs_kernels.h, bgm_causal_hmc_set_partial; engine partial=True,
CausalBGM.predict_new): NaN in y, or in x and y, marks what a row does not observe, and the row's chain samples p(z | x, v) or
p(z | v) -- the log posterior with the outcome term of f, and the treatment term of h, left out.

Bars (those of the tests that check the same quantity without the option, tests/test_gpu_causal_hmc.py):
  log posterior   |hip - float64| <= 2e-6 |ref| + 2e-4;   gradient  |hip - float64| <= 5e-5 max|grad of the row|
  chains          last draw within 1e-4 of the float32 restatement (tests/_causal_partial_ref.py) on >= 97 % of the rows, the steps
                  of those rows bit for bit; tests/test_causal_hmc_partial_host.py keeps the restatement within 98.5 % of its float64
                  twin on the same inputs
  moments         row_mean / row_sd against float64 on the run's own float32 row_draws: the float32 accumulation of KEEP terms,
                  with D = max |y - ref| of the (row, dose):  |mean| <= 2 KEEP D 2^-24,  |var| <= 6 KEEP^2 / (KEEP - 1) D^2 2^-24
                  (s1 and s2 are sums of KEEP terms bounded by D and D^2 whose partial sums are bounded by KEEP times that; doubled
                  for the rounding of y - ref itself)
  class, blocks   32-row blocks against one block: bit-identical bounds for interval='quantile'; mean and sd within n 2^-24 Y, the
                  reassociation bound of predict_individual's test (every (row, dose) has one owner lane, so they are in fact equal)
everything else is bit-identity."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_partial_ref as PR  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_causal_hmc_partial_host import (CHAIN_BURN, CHAIN_BURN_MASS, CHAIN_CASES, CHAIN_KEEP, CHAIN_L, CHAIN_SEED, CHAIN_STEP0,  # noqa: E402
                                                chain_inputs, chain_runs)
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402

from bayesgm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
BURN, KEEP, LEAP, STEP0 = 10, 10, 3, 0.1
BURN_MASS = 20                                       # the shortest burn-in with an estimation window of the metric
KT = {1: [1, 1, 1, 7], 2: [3, 3, 6, 6]}              # both first-layer tilings; with KT1 = 2 the treatment rides in the second tile
CASES = [dict(kt1=1, binary=False), dict(kt1=2, binary=True), dict(kt1=2, binary=False), dict(kt1=1, binary=True)]
P = 20
KEYS = ("draws", "state", "logp", "grad", "row_step", "acc_count")
XS = np.linspace(0.0, 3.0, 5)
NAN = float("nan")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _id(case):
    return "kt%d-%s" % (case["kt1"], "binary" if case["binary"] else "continuous")


def _setup(case, n, seed, mixed=True):
    m = _model(seed, KT[case["kt1"]], P, case["binary"])
    x, y, v = _data(n, P, seed + 1, case["binary"])
    if mixed:
        x, y = PR.mixed_panel(x, y, seed + 2)
    return m, _engine(m), x, y, v


def _sample(eng, x, y, v, seed, burn=BURN, **kw):
    return eng.hmc_sample(x, y, v, burn, KEEP, STEP0, LEAP, seed, adapt=TARGET, **kw)


def _effect_kw(case):
    return dict(effect=_lib.EFFECT_ITE) if case["binary"] else dict(row_effects=True, row_draws=True, x_values=XS)


def _effect_keys(case):
    return ("ite",) if case["binary"] else ("row_mean", "row_sd", "row_draws")


def _check_grad(gr, ref_gr, what):
    gmax = np.abs(ref_gr).max(axis=1)
    gerr = np.abs(gr - ref_gr).max(axis=1)
    print("%s: worst |grad - float64| / (5e-5 max|grad|) %.3f" % (what, (gerr / (5e-5 * gmax)).max()))
    assert np.all(gerr <= 5e-5 * gmax), (gerr / gmax).max()


def _check_logp_grad(lp, gr, ref_lp, ref_gr, what):
    err = np.abs(lp - ref_lp)
    print("%s: worst |logp - float64| / bar %.3f" % (what, (err / (2e-6 * np.abs(ref_lp) + 2e-4)).max()))
    assert np.all(err <= 2e-6 * np.abs(ref_lp) + 2e-4), (err.max(), np.abs(ref_lp).max())
    _check_grad(gr, ref_gr, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. on a fully observed panel the option changes nothing, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_observed_panel_is_the_run_without_the_option(torch, case):
    n, seed = 33, 99
    m, eng, x, y, v = _setup(case, n, 31, mixed=False)
    z = np.random.RandomState(3).randn(n, sum(KT[case["kt1"]])).astype(np.float32)
    lp0, gr0 = eng.logpost_grad(x.ravel(), y.ravel(), v, z)
    lp1, gr1 = eng.logpost_grad(x.ravel(), y.ravel(), v, z, partial=True)
    assert torch.equal(lp0, lp1) and torch.equal(gr0, gr1)
    for kw, keys, burn in ((dict(want_draws=True), (), BURN), (dict(want_draws=True, mass="diag"), ("mass_scale",), BURN_MASS),
                           (dict(want_draws=True, **_effect_kw(case)), _effect_keys(case), BURN),
                           (dict(mass="diag", **_effect_kw(case)), ("mass_scale",) + _effect_keys(case), BURN_MASS)):
        a = _sample(eng, x, y, v, seed, burn, **kw)
        b = _sample(eng, x, y, v, seed, burn, partial=True, **kw)
        for k in KEYS + keys:
            if a[k] is not None:
                assert torch.equal(a[k], b[k]), (k, sorted(kw))
        assert 0 < int(a["acc_count"].sum()) < (burn + KEEP) * n
    # the flag is cleared on the way out: a NaN without the option is today's NaN
    ynan = y.copy()
    ynan[5] = NAN
    lp2, _ = eng.logpost_grad(x.ravel(), ynan.ravel(), v, z)
    assert bool(torch.isnan(lp2[5])) and torch.equal(lp2[:5], lp0[:5]) and torch.equal(lp2[6:], lp0[6:])


# ---------------------------------------------------------------------------------------------------------------------
# 2. log posterior and gradient against float64, the three patterns mixed within a tile and across tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True], ids=["learned", "fixed"])
@pytest.mark.parametrize("n", [1, 16, 17, 33])
@pytest.mark.parametrize("case", CASES[:2], ids=_id)
def test_logpost_grad_matches_float64(torch, case, n, fixed):
    kw = dict(sigma_v=0.8, sigma_x=1.3, sigma_y=0.5) if fixed else {}
    m = _model(1, KT[case["kt1"]], P, case["binary"], **kw)
    x, y, v = _data(n, P, 2, case["binary"])
    x, y = PR.mixed_panel(x, y, 4 + n)
    has_x, has_y = PR.patterns(x, y)
    assert n < 3 or (has_y.any() and (has_x & ~has_y).any() and (~has_x).any())
    z = np.random.RandomState(3).randn(n, sum(KT[case["kt1"]])).astype(np.float32)
    eng = _engine(m)
    lp, gr = eng.logpost_grad(x.ravel(), y.ravel(), v, z, partial=True)
    assert lp.shape == (n,) and gr.shape == z.shape and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(gr).all())
    ref = PR.log_posterior_and_grad(OC.cast_model(m, np.float64), *(a.astype(np.float64) for a in (x, y, v, z)))
    _check_logp_grad(lp.cpu().numpy(), gr.cpu().numpy(), *ref, "%s n = %d" % (_id(case), n))


@pytest.mark.parametrize("case", CASES[:2], ids=_id)
def test_missing_terms_are_those_of_a_model_without_them(torch, case):
    """Nothing known but v: the gradient of partial=True (x = y = NaN) is the float64 gradient without the f and h terms, and so is
    the gradient of the run WITHOUT the option on a model whose f / h output layers are zero (their terms are constant in z), at
    finite stand-in values: what stands in for a missing entry does not enter."""
    n = 33
    m = _model(1, KT[case["kt1"]], P, case["binary"])
    _, _, v = _data(n, P, 2, case["binary"])
    nan = np.full((n, 1), NAN, np.float32)
    z = np.random.RandomState(3).randn(n, sum(KT[case["kt1"]])).astype(np.float32)
    ref = PR.log_posterior_and_grad(OC.cast_model(m, np.float64), *(a.astype(np.float64) for a in (nan, nan, v, z)))
    lp, gr = _engine(m).logpost_grad(nan.ravel(), nan.ravel(), v, z, partial=True)
    _check_logp_grad(lp.cpu().numpy(), gr.cpu().numpy(), *ref, "x, y missing")
    m0 = dict(m)
    for k in ("f", "h"):
        W, b = m[k][-1]
        m0[k] = list(m[k][:-1]) + [(np.zeros_like(W), np.zeros_like(b))]
    for xs, ys in ((0.0, 0.0), (1.0, -2.5)):
        _, gr0 = _engine(m0).logpost_grad(np.full(n, xs, np.float32), np.full(n, ys, np.float32), v, z)
        _check_grad(gr0.cpu().numpy(), ref[1], "f, h zeroed, stand-in (%g, %g)" % (xs, ys))


# ---------------------------------------------------------------------------------------------------------------------
# 3. a row's value does not depend on the patterns of the other rows of its tile: beside observed rows (its missing term is masked
#    while the tile's other rows use theirs) or in a tile where no row has the target (the case a tile-skipping branch would take:
#    the kernels have none, DESIGN.md section 4x, and this is the test such a branch has to pass)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, "diag"], ids=["identity", "diag"])
@pytest.mark.parametrize("case", CASES[:2], ids=_id)
def test_a_row_does_not_depend_on_the_patterns_of_its_tile(torch, case, mass):
    n, seed = 33, 4711
    burn = BURN_MASS if mass else BURN
    m, eng, x, y, v = _setup(case, n, 41)
    y[32] = NAN                                              # the one row of the ragged tile: without its outcome
    has_x, has_y = PR.patterns(x, y)
    for t0 in (0, 16):                    # the full tiles of the mixed panel hold rows with and without either target
        assert has_y[t0:t0 + 16].any() and has_x[t0:t0 + 16].any() and not has_y[t0:t0 + 16].all() and not has_x[t0:t0 + 16].all()
    z = np.random.RandomState(5).randn(n, sum(KT[case["kt1"]])).astype(np.float32)
    lp, gr = eng.logpost_grad(x.ravel(), y.ravel(), v, z, partial=True)
    full = _sample(eng, x, y, v, seed, burn, want_draws=True, partial=True, mass=mass)
    y_rows = np.flatnonzero((has_x & ~has_y)[:32])[[0, 5, -1]]      # alone: a tile without an outcome
    xy_rows = np.flatnonzero((~has_x)[:32])[[0, 5, -1]]            # alone: a tile without outcome and treatment
    for r in list(y_rows) + list(xy_rows) + [32]:
        lp1, gr1 = eng.logpost_grad(x[r:r + 1].ravel(), y[r:r + 1].ravel(), v[r:r + 1], z[r:r + 1], partial=True)
        assert torch.equal(lp1, lp[r:r + 1]) and torch.equal(gr1, gr[r:r + 1]), r
        one = _sample(eng, x[r:r + 1], y[r:r + 1], v[r:r + 1], seed, burn, want_draws=True, partial=True, mass=mass, row_base=int(r))
        assert torch.equal(one["draws"], full["draws"][:, r:r + 1]), r
        for k in ("state", "logp", "grad", "row_step") + (("mass_scale",) if mass else ()):
            assert torch.equal(one[k], full[k][r:r + 1]), (k, r)
    # a whole tile without outcomes beside the mixed ones: rows 16..31 lose y (x kept where it was), the other rows do not notice
    y2 = y.copy()
    y2[16:32] = NAN
    lp2, gr2 = eng.logpost_grad(x.ravel(), y2.ravel(), v, z, partial=True)
    same = ~has_y
    same[:16] = True
    same[32:] = True
    idx = torch.from_numpy(np.flatnonzero(same)).to(lp.device)
    assert torch.equal(lp2[idx], lp[idx]) and torch.equal(gr2[idx], gr[idx])
    assert not torch.equal(lp2[16:32], lp[16:32])


# ---------------------------------------------------------------------------------------------------------------------
# 4. chains against the float32 restatement, adaptation on, with and without the estimated metric
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [False, True], ids=["identity", "diag"])
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: "q%d" % sum(c["z_dims"]))
def test_chains_match_the_float32_restatement(torch, case, mass):
    m, (x, y, v) = chain_inputs(case)
    n, burn = len(x), CHAIN_BURN_MASS if mass else CHAIN_BURN
    out = _engine(m).hmc_sample(x, y, v, burn, CHAIN_KEEP, CHAIN_STEP0, CHAIN_L, CHAIN_SEED, want_draws=True, chunk=7, adapt=TARGET,
                                mass="diag" if mass else None, partial=True)
    ref = chain_runs(case, mass)
    draws, acc, step = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy().astype(np.int64), out["row_step"].cpu().numpy()
    assert draws.shape == ref["draws"].shape and np.all(np.isfinite(draws))
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    print("rows equal to the restatement: %.4f; acceptance %.3f; step q05 / median / q95 %.4f / %.4f / %.4f"
          % (row_ok.mean(), acc.sum() / float(acc.size * n), *np.quantile(step, [0.05, 0.5, 0.95])))
    assert row_ok.mean() >= 0.97, row_ok.mean()
    assert np.array_equal(step[row_ok], ref["step"][row_ok]) and np.ptp(step) > 0
    assert np.abs(acc - ref["acc"].sum(axis=1)).max() <= int((~row_ok).sum())
    if mass:
        rel = np.abs(out["mass_scale"].cpu().numpy()[row_ok] / ref["scale"][row_ok] - 1)
        assert rel.max() <= 1e-3, rel.max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the effects of a partial run are engine.effects on its stored draws; cuts and row windows change nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_effects_are_those_of_the_stored_draws(torch, case):
    n, seed = 33, 5
    m, eng, x, y, v = _setup(case, n, 51)
    kw = dict(want_draws=True, partial=True, **_effect_kw(case))
    one = _sample(eng, x, y, v, seed, **kw)
    x0 = np.nan_to_num(x)                       # (the effect pass puts the dose into the treatment slot; a row's own x is never read)
    assert bool(torch.isfinite(one["draws"]).all())
    if case["binary"]:
        ite = eng.effects(x0, one["draws"], BURN, seed, sample_y=True)              # [keep, n]
        assert torch.equal(one["ite"], ite.t().contiguous()) and bool(torch.isfinite(ite).all())
    else:
        for r in (0, 1, 2, 15, 16, 32):
            ref = eng.effects(x0[r:r + 1], one["draws"][:, r:r + 1].contiguous(), BURN, seed, x_values=XS, sample_y=True, row_base=r)
            assert torch.equal(one["row_draws"][r], ref), r
        yd = one["row_draws"].cpu().numpy().astype(np.float64)
        D = np.abs(yd - yd[..., :1]).max(axis=-1)
        e_mean = np.abs(one["row_mean"].cpu().numpy() - yd.mean(axis=-1))
        e_var = np.abs(one["row_sd"].cpu().numpy() ** 2 - yd.var(axis=-1, ddof=1))
        print("moments against float64 on the run's own draws: mean / bound %.3f, var / bound %.3f"
              % ((e_mean / (2 * KEEP * D * 2.0 ** -24)).max(), (e_var / (6 * KEEP ** 2 / (KEEP - 1.0) * D ** 2 * 2.0 ** -24)).max()))
        assert np.all(D > 0) and np.all(e_mean <= 2 * KEEP * D * 2.0 ** -24) and np.all(e_var <= 6 * KEEP ** 2 / (KEEP - 1.0) * D ** 2 * 2.0 ** -24)
    cut = _sample(eng, x, y, v, seed, chunk=7, **kw)      # cuts inside burn-in, across burn_in = 10 (7 | 14) and after it
    a, e = 7, 29                                          # rows [a, e) alone with their global row index, both edges inside a tile
    part = _sample(eng, x[a:e], y[a:e], v[a:e], seed, row_base=a, **kw)
    for k in KEYS + _effect_keys(case):
        assert torch.equal(one[k], cut[k]), k
        if k != "acc_count":
            rows = (slice(None), slice(a, e)) if k == "draws" else slice(a, e)
            assert torch.equal(one[k][rows], part[k]), k


def test_effect_kernels_without_a_partial_twin_refuse(torch):
    n = 16
    m, eng, x, y, v = _setup(CASES[0], n, 61)
    with pytest.raises(RuntimeError, match=r"\(-4\).*bgm_causal_hmc_set_partial"):
        _sample(eng, x, y, v, 3, effect=_lib.EFFECT_ADRF, x_values=XS, partial=True)
    mb, engb, xb, yb, vb = _setup(CASES[1], n, 62)
    with pytest.raises(RuntimeError, match=r"\(-4\).*bgm_causal_hmc_set_partial"):
        _sample(engb, xb, yb, vb, 3, effect=_lib.EFFECT_GROUP_ITE, labels=np.zeros(n, np.int32), n_labels=1, partial=True)
    xo, yo, _ = _data(n, P, 62)
    bad_x = xo.copy()
    bad_x[3] = NAN
    with pytest.raises(ValueError, match="row 3 has its outcome y observed"):
        eng.logpost_grad(bad_x.ravel(), yo.ravel(), v, np.zeros((n, 10), np.float32), partial=True)
    # the refusals left the handles usable and the option off
    adrf = _sample(eng, xo, yo, v, 3, effect=_lib.EFFECT_ADRF, x_values=XS)["adrf"]
    assert adrf.shape == (len(XS), KEEP) and bool(torch.isfinite(adrf).all())
    assert _sample(engb, xb, yb, vb, 3, partial=True)["row_step"].shape == (n,)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the second trip of the tile loop, every outcome missing
# ---------------------------------------------------------------------------------------------------------------------
def test_second_trip_of_the_tile_loop(torch):
    burn, keep, L, seed = 3, 2, 2, 4242
    m = _model(65, KT[1], P)
    eng = _engine(m)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus + 17
    slots = eng.mh_slots(n)
    assert (n + 15) // 16 > slots
    x, _, v = _data(n, P, 66)
    y = np.full((n, 1), NAN, np.float32)
    x[1::3] = NAN                                      # and a third of the rows without their treatment
    kw = dict(want_draws=True, adapt=TARGET, partial=True)
    full = eng.hmc_sample(x, y, v, burn, keep, STEP0, L, seed, **kw)
    cuts = [0, n // 3 // 16 * 16 + 7, 2 * n // 3 // 16 * 16, n]
    assert cuts[1] % 16 != 0 and all((e - s + 15) // 16 <= slots for s, e in zip(cuts[:-1], cuts[1:]))
    parts = [eng.hmc_sample(x[s:e], y[s:e], v[s:e], burn, keep, STEP0, L, seed, row_base=s, **kw) for s, e in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(full["draws"], torch.cat([p["draws"] for p in parts], dim=1))
    for k in ("state", "logp", "grad", "row_step"):
        assert torch.equal(full[k], torch.cat([p[k] for p in parts], dim=0)), k
    assert torch.equal(full["acc_count"], sum(p["acc_count"] for p in parts))
    assert bool(torch.isfinite(full["draws"]).all()) and 0 < int(full["acc_count"].sum()) < (burn + keep) * n
    z = full["state"].cpu().numpy()
    lp, gr = eng.logpost_grad(x.ravel(), y.ravel(), v, z, partial=True)
    ref = PR.log_posterior_and_grad(OC.cast_model(m, np.float64), *(a.astype(np.float64) for a in (x, y, v, z)))
    _check_logp_grad(lp.cpu().numpy(), gr.cpu().numpy(), *ref, "n = %d (%d tiles, %d wave slots)" % (n, (n + 15) // 16, slots))


# ---------------------------------------------------------------------------------------------------------------------
# 7. the class surface
# ---------------------------------------------------------------------------------------------------------------------
def _causal(tmp_path, m, binary, seed=3):
    from bayesgm_amd.models import CausalBGM
    params = dict(dataset="t", output_dir=str(tmp_path), save_res=False, save_model=False, binary_treatment=binary, use_bnn=False,
                  z_dims=KT[1], v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
                  e_units=[64] * 5, dz_units=[64, 32, 8], kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, mixing_check=False)
    model = CausalBGM(params, random_seed=seed)
    model.set_weights(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
    return model


def _seed_of(model):
    return (model._base_seed * 1000003 + model._seed_counter) & 0x7FFFFFFFFFFFFFFF


@pytest.mark.parametrize("mass", ["identity", "diag"])
@pytest.mark.parametrize("binary", [False, True], ids=["continuous", "binary"])
def test_predict_new(torch, tmp_path, binary, mass):
    n, burn, keep = 70, 30, 20
    m = OC.init_model(0, KT[1], P, binary_treatment=binary)
    x, _, v = _data(n, P, 8, binary)
    x_some = x.ravel().copy()
    x_some[::4] = NAN
    kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=3, mass=mass)
    if not binary:
        kw["x_values"] = XS
    shape = (n,) if binary else (n, len(XS))
    n_doses = 1 if binary else len(XS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = {}
        for name, data_x in (("none", None), ("some", x_some)):
            for interval in ("normal", "quantile"):
                a = _causal(tmp_path, m, binary)
                mean, bounds = a.predict_new(v, data_x, interval=interval, **kw)
                assert mean.shape == shape and bounds.shape == shape + (2,) and a.individual_sd_.shape == shape
                assert np.all(np.isfinite(mean)) and np.all(np.isfinite(bounds)) and np.all(a.individual_sd_ > 0)
                assert np.all(bounds[..., 0] <= mean) and np.all(mean <= bounds[..., 1])
                assert a.hmc_row_step_.shape == (n,) and np.ptp(a.hmc_row_step_) > 0
                assert (a.hmc_row_mass_ is None) == (mass == "identity")
                res[name, interval] = (mean, bounds, a.individual_sd_, a.hmc_row_step_)
            assert np.array_equal(res[name, "normal"][0], res[name, "quantile"][0])            # one chain, one mean
            assert not np.array_equal(res[name, "normal"][1], res[name, "quantile"][1])
        assert not np.array_equal(res["none", "normal"][0], res["some", "normal"][0])          # a known treatment informs z
        # 32-row blocks against one block
        b = _causal(tmp_path, m, binary)
        mean_b, bounds_b = b.predict_new(v, x_some, interval="quantile", draw_budget_bytes=4 * keep * n_doses * 32, **kw)
        mean_a, bounds_a, sd_a, step_a = res["some", "quantile"]
        assert np.array_equal(bounds_b, bounds_a) and np.array_equal(b.hmc_row_step_, step_a)
        big = float(np.abs(bounds_a).max())
        bound = n * 2.0 ** -24 * big
        assert np.abs(mean_b - mean_a).max() <= bound and np.abs(b.individual_sd_ - sd_a).max() <= bound
        # the engine call behind it: the rows' chains are those of hmc_sample(partial=True) with the class's seed
        c = _causal(tmp_path, m, binary)
        mean_c, _ = c.predict_new(v, x_some, interval="normal", **kw)
        assert np.array_equal(mean_c, res["some", "normal"][0])
    y = np.full(n, NAN, np.float32)
    out = c.engine.hmc_sample(x_some, y, v, burn, keep, 0.1, 3, _seed_of(c), adapt=TARGET, mass=None if mass == "identity" else "diag",
                              partial=True, **(dict(effect=_lib.EFFECT_ITE) if binary else dict(row_effects=True, x_values=XS)))
    assert np.array_equal(out["row_step"].cpu().numpy(), c.hmc_row_step_)
    if binary:
        assert np.allclose(out["ite"].double().mean(dim=1).cpu().numpy(), mean_c, rtol=1e-5, atol=1e-6)
    else:
        assert np.array_equal(out["row_mean"].cpu().numpy(), mean_c)


def test_hmc_sampler_with_partial_rows(torch, tmp_path):
    n, burn, keep = 33, 10, 10
    m = OC.init_model(0, KT[1], P)
    x, y, v = _data(n, P, 8)
    x, y = PR.mixed_panel(x, y, 9)
    a = _causal(tmp_path, m, False)
    draws = a.hmc_sampler((x, y, v), n_keep=keep, burn_in=burn, step_size=0.1, n_leapfrog=3, partial=True)
    ref = a.engine.hmc_sample(x, y, v, burn, keep, 0.1, 3, _seed_of(a), want_draws=True, adapt=TARGET, partial=True)
    assert draws.shape == (keep, n, 10) and np.all(np.isfinite(draws)) and np.array_equal(ref["draws"].cpu().numpy(), draws)
    assert a.hmc_row_step_.shape == (n,) and np.ptp(a.hmc_row_step_) > 0
