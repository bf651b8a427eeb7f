"""The CausalBGM HMC sampler with the dose-response of every row kept inside the kernel (csrc/causal_hmc_rowfx_kernels.h,
bgm_causal_hmc_run_row_effects; hmc_sample(row_effects=True), CausalBGM.predict_individual).

Bars:
  chain, cuts, row windows, blocks   bit-identity (torch.equal / np.array_equal)
  one-row anchor                     row_draws[r] equals, bit for bit, the fused ADRF of the one-row panel (x[r:r+1], row_base=r): the
                                     routine of the parent commit (the sum over a tile with one valid row adds zeros to y)
  oracle                             row_draws and row_mean against float64 oracle.causal on the returned latent draws: 2e-4 absolute,
                                     the bar tests/test_gpu_causal.py applies to engine.effects.  row_sd: the sd of a series is
                                     1-Lipschitz in the largest per-draw error up to sqrt(m / (m - 1)), so 2e-4 sqrt(m / (m - 1)) plus
                                     the float32 accumulation error of the m shifted terms, ACC[m]
  ACC[m]                             row_mean / row_sd against float64 mean / sd of the run's own float32 row_draws.  Measured on
                                     an MI355X over the cases of this file (printed by the tests) and
                                     entered with a margin of 4x over the largest value seen, which covers other seeds
  class level                        mean over rows of predict_individual's mean against predict(fused_effects=True)'s ADRF:
                                     n * 2**-24 * Y, the reassociation bound of tests/test_gpu_causal_hmc_fused.py"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import causal as OC  # noqa: E402
from oracle import rng as R  # noqa: E402
from oracle.nets import mlp_forward  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402
from tests.test_gpu_causal_hmc_fused import P, Z_DIMS, _causal, _largest_outcome_draw, _seed_of  # noqa: E402

from bayesgm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
BURN, KEEP, LEAP, STEP0 = 30, 20, 3, 0.1
SHAPES = [dict(z_dims=[1, 1, 1, 7], p=20), dict(z_dims=[3, 3, 6, 6], p=20)]      # both first-layer tilings (KT1 = 1, 2)
KEYS = ("draws", "state", "logp", "grad", "row_step", "acc_count")
N = 200                                                                             # 13 tiles, the last one of 8 rows
ANCHOR_ROWS = (0, 15, 16, 192, 199)                                                 # tile edges and the ragged tile
ACC = {20: 4 * 1.80e-6, 400: 4 * 8.46e-6}     # see the module docstring: 4 x the largest |moments - float64 of the own draws| measured


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _id(case):
    return "q%d" % sum(case["z_dims"])


def _plain(eng, x, y, v, burn, keep, leap, seed, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, want_draws=True, adapt=TARGET, **kw)


def _rows(eng, x, y, v, burn, keep, leap, seed, xs, sample_y=True, want_draws=True, row_draws=True, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, want_draws=want_draws, adapt=TARGET, row_effects=True, row_draws=row_draws,
                          x_values=xs, sample_y=sample_y, **kw)


def _one_row_adrf(eng, x, y, v, r, burn, keep, leap, seed, xs, sample_y, **kw):
    """the ADRF of the one-row panel (row r alone, with its global index): [n_doses, keep], the routine of the fused-ADRF kernels"""
    return eng.hmc_sample(x[r:r + 1], y[r:r + 1], v[r:r + 1], burn, keep, STEP0, leap, seed, adapt=TARGET, row_base=r, effect=_lib.EFFECT_ADRF,
                          x_values=xs, sample_y=sample_y, **kw)["adrf"]


def _same_chain(torch, plain, other):
    for k in KEYS + (("mass_scale",) if "mass_scale" in plain else ()):
        assert torch.equal(plain[k], other[k]), k


def _same_rows(torch, a, b, rows=slice(None)):
    for k in ("row_mean", "row_sd", "row_draws"):
        assert torch.equal(a[k][rows], b[k]), k


def _shapes_ok(torch, out, n, n_doses, keep):
    assert out["row_mean"].shape == out["row_sd"].shape == (n, n_doses) and out["row_mean"].dtype == out["row_sd"].dtype == torch.float64
    assert out["row_draws"].shape == (n, n_doses, keep) and out["row_draws"].dtype == torch.float32
    assert bool(torch.isfinite(out["row_draws"]).all()) and bool(torch.isfinite(out["row_mean"]).all()) and bool((out["row_sd"] >= 0).all())


def _oracle_rows(m, draws, xs, sample_y, seed, burn, row0=0):
    """float64 y_i(x_k) of every row, dose and draw: the per-row body of oracle.causal.infer_from_latent_posterior before its
    .mean() -> [n, n_doses, keep]"""
    m64 = OC.cast_model(m, np.float64)
    draws = draws.astype(np.float64)
    keep, n, _ = draws.shape
    doses = np.asarray(xs, np.float32).astype(np.float64)
    out = np.empty((n, len(doses), keep))
    for d in range(keep):
        nz = R.normals_seq(np.arange(row0, row0 + n), burn + d, len(doses), R.TAG_YNOISE, seed).astype(np.float64)
        z0, z1, _ = OC.split_z(m64, draws[d])
        for k, xv in enumerate(doses):
            f = mlp_forward(m64["f"], np.concatenate([z0, z1, np.full((n, 1), xv)], axis=-1))
            s2 = OC._sig2(m64, "sigma_y", f[:, 1], np.float64)
            out[:, k, d] = f[:, 0] + np.sqrt(s2) * nz[:, k] if sample_y else f[:, 0]
    return out


def _own_moment_error(out):
    """|row_mean - mean|, |row_sd - sd| against float64 on the run's own float32 row_draws: the float32 accumulation alone"""
    y = out["row_draws"].cpu().numpy().astype(np.float64)
    return (float(np.abs(out["row_mean"].cpu().numpy() - y.mean(axis=-1)).max()),
            float(np.abs(out["row_sd"].cpu().numpy() - y.std(axis=-1, ddof=1)).max()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. + 2. the chain is unchanged; a row's draws are the ADRF of the one-row panel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_chain_unchanged_and_rows_are_one_row_panels(torch, case):
    seed = 99
    m = _model(31, case["z_dims"], case["p"])
    x, y, v = _data(N, case["p"], 32)
    eng = _engine(m)
    plain = _plain(eng, x, y, v, BURN, KEEP, LEAP, seed)
    assert "row_mean" not in plain and "row_draws" not in plain
    assert bool(torch.isfinite(plain["draws"]).all()) and 0 < int(plain["acc_count"].sum()) < (BURN + KEEP) * N
    for n_doses in (1, 5, 17, 20):      # 17, 20: lane groups with a Philox call of their own, and the shared remainder
        xs = np.linspace(0.0, 3.0, n_doses)
        for sample_y in (True, False):
            out = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y)
            _same_chain(torch, plain, out)
            _shapes_ok(torch, out, N, n_doses, KEEP)
            assert "adrf" not in out and "ite" not in out
            if n_doses >= 17:
                for r in ANCHOR_ROWS:
                    anchor = _one_row_adrf(eng, x, y, v, r, BURN, KEEP, LEAP, seed, xs, sample_y)
                    assert torch.equal(out["row_draws"][r], anchor), (r, n_doses, sample_y)
            if not sample_y:            # without noise the doses of a row differ through the net alone
                assert n_doses == 1 or not torch.equal(out["row_draws"][:, 0], out["row_draws"][:, -1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. + 4. the float64 oracle on the returned draws; the moments are those of the draws
# ---------------------------------------------------------------------------------------------------------------------
def _against_oracle(torch, case, sample_y, keep):
    seed = 5
    m = _model(51, case["z_dims"], case["p"])
    x, y, v = _data(N, case["p"], 52)
    xs = np.linspace(0.0, 3.0, 20)
    out = _rows(_engine(m), x, y, v, BURN, keep, LEAP, seed, xs, sample_y)
    _shapes_ok(torch, out, N, 20, keep)
    ref = _oracle_rows(m, out["draws"].cpu().numpy(), xs, sample_y, seed, BURN)
    got, mean, sd = (out[k].cpu().numpy() for k in ("row_draws", "row_mean", "row_sd"))
    e_draws = np.abs(got - ref).max()
    e_mean = np.abs(mean - ref.mean(axis=-1)).max()
    e_sd = np.abs(sd - ref.std(axis=-1, ddof=1)).max()
    a_mean, a_sd = _own_moment_error(out)
    bar_sd = 2e-4 * np.sqrt(keep / (keep - 1.0)) + ACC[keep]
    print("rows q%d sample_y=%d keep=%d against the float64 oracle: draws %.3g, mean %.3g (bar 2e-4), sd %.3g (bar %.6g); "
          "accumulation alone: mean %.3g, sd %.3g (ACC %.3g); largest |y| %.3f, largest sd %.3f"
          % (sum(case["z_dims"]), sample_y, keep, e_draws, e_mean, e_sd, bar_sd, a_mean, a_sd, ACC[keep], np.abs(ref).max(), sd.max()))
    assert e_draws <= 2e-4 and e_mean <= 2e-4 and e_sd <= bar_sd
    # 4. (never alone: the lines above tie the draws to the oracle)
    assert a_mean <= ACC[keep] and a_sd <= ACC[keep]


@pytest.mark.parametrize("sample_y", [True, False], ids=["noise", "mean"])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_rows_match_the_float64_oracle_and_the_moments_their_draws(torch, case, sample_y):
    _against_oracle(torch, case, sample_y, KEEP)


def test_rows_match_the_float64_oracle_over_400_draws(torch):
    """the one case where the float32 accumulation is more than a rounding or two"""
    _against_oracle(torch, SHAPES[0], True, 400)


# ---------------------------------------------------------------------------------------------------------------------
# 5. invariances
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_cuts_row_windows_and_missing_draws_change_nothing(torch, case):
    seed = 4711
    m = _model(41, case["z_dims"], case["p"])
    x, y, v = _data(N, case["p"], 42)
    eng = _engine(m)
    xs = np.linspace(0.0, 3.0, 17)
    one = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs)
    cut = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, chunk=7)      # cuts in burn-in, at 28 | 35 across burn_in = 30, and after it
    _same_chain(torch, one, cut)
    _same_rows(torch, one, cut)
    a, e = 23, 171                                                       # rows [a, e) alone with their global row index
    part = _rows(eng, x[a:e], y[a:e], v[a:e], BURN, KEEP, LEAP, seed, xs, row_base=a)
    _same_rows(torch, one, part, slice(a, e))
    assert torch.equal(part["draws"], one["draws"][:, a:e])
    nodraws = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, want_draws=False)
    assert nodraws["draws"] is None and torch.equal(nodraws["state"], one["state"])
    _same_rows(torch, one, nodraws)
    moments_only = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, want_draws=False, row_draws=False)
    assert "row_draws" not in moments_only
    assert torch.equal(moments_only["row_mean"], one["row_mean"]) and torch.equal(moments_only["row_sd"], one["row_sd"])


def test_rows_beyond_one_trip_of_the_tile_loop(torch):
    """16 x 8 x CUs x 2 + 37 rows: every wave slot walks two or three tiles, the last tile is ragged; a row's result is that of the
    one-row panel wherever the tile walk puts it"""
    burn, keep, leap, seed = 3, 2, 2, 4242
    m = _model(65, [1, 1, 1, 7], 20)
    eng = _engine(m)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus * 2 + 37
    assert waves == 8 and eng.mh_slots(n) == waves * n_cus and (n + 15) // 16 == 2 * waves * n_cus + 3
    x, y, v = _data(n, 20, 66)
    xs = np.linspace(0.0, 3.0, 5)
    plain = _plain(eng, x, y, v, burn, keep, leap, seed)
    out = _rows(eng, x, y, v, burn, keep, leap, seed, xs)
    _same_chain(torch, plain, out)
    _shapes_ok(torch, out, n, 5, keep)
    chunked = _rows(eng, x, y, v, burn, keep, leap, seed, xs, chunk=2)
    _same_rows(torch, out, chunked)
    for r in (0, 16 * waves * n_cus + 21, n - 1):      # the first row, a row of the second trip, the last row (ragged tile, third trip)
        anchor = _one_row_adrf(eng, x, y, v, r, burn, keep, leap, seed, xs, True)      # [n_doses, keep]
        assert torch.equal(out["row_draws"][r], anchor), r
        mean = anchor[:, 0].double() + (anchor[:, 1] - anchor[:, 0]).double() / 2      # ref + s1 / m with m = 2: s1 is one float32 difference
        assert torch.equal(out["row_mean"][r], mean), r


def test_row_draws_beyond_two_to_the_31_elements(torch):
    """[n, 20, keep] with n * 20 * keep > 2**31: the rows whose draws straddle that element index, and the last row, are still the
    one-row panels (a 32-bit index would wrap there and nowhere below)"""
    burn, leap, seed, n, n_doses = 2, 1, 77, 65573, 20
    keep = 2 ** 31 // (n * n_doses) + 2
    assert n * n_doses * keep > 2 ** 31 + n_doses * keep and n * n_doses * keep * 4 < 9 << 30
    m = _model(67, [1, 1, 1, 7], 20)
    eng = _engine(m)
    x, y, v = _data(n, 20, 68)
    xs = np.linspace(0.0, 3.0, n_doses)
    out = _rows(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False)
    assert out["row_draws"].shape == (n, n_doses, keep)
    edge = 2 ** 31 // (n_doses * keep)                                   # the row that holds element 2**31
    assert 0 < edge < n - 2
    for r in (edge - 1, edge, edge + 1, n - 1):
        anchor = _one_row_adrf(eng, x, y, v, r, burn, keep, leap, seed, xs, True)
        assert torch.equal(out["row_draws"][r], anchor), r
    del out


# ---------------------------------------------------------------------------------------------------------------------
# 6. with a metric
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_rows_with_a_metric(torch, case):
    seed, burn = 99, 40
    m = _model(31, case["z_dims"], case["p"])
    x, y, v = _data(N, case["p"], 32)
    eng = _engine(m)
    xs = np.linspace(0.0, 3.0, 17)
    identity = _plain(eng, x, y, v, burn, KEEP, LEAP, seed)
    # the metric every chain estimates for itself
    plain = _plain(eng, x, y, v, burn, KEEP, LEAP, seed, mass="diag")
    assert not torch.equal(plain["draws"], identity["draws"])
    out = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, mass="diag")
    _same_chain(torch, plain, out)
    cut = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, chunk=7, mass="diag")
    _same_chain(torch, plain, cut)
    _same_rows(torch, out, cut)
    for r in ANCHOR_ROWS:             # the metric does not enter the outcome net: engine.effects on the row's stored draws
        ref = eng.effects(x[r:r + 1], plain["draws"][:, r:r + 1].contiguous(), burn, seed, x_values=xs, sample_y=True, row_base=r)
        assert torch.equal(out["row_draws"][r], ref), r
    # that metric given frozen: another chain (the scale holds from the first iteration), the same identities
    scale = out["mass_scale"].clone()
    frozen_plain = _plain(eng, x, y, v, burn, KEEP, LEAP, seed, mass_scale=scale)
    assert not torch.equal(frozen_plain["draws"], plain["draws"])
    for sample_y in (True, False):
        frozen = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass_scale=scale)
        _same_chain(torch, frozen_plain, frozen)
        for r in ANCHOR_ROWS:
            anchor = _one_row_adrf(eng, x, y, v, r, burn, KEEP, LEAP, seed, xs, sample_y, mass_scale=scale[r:r + 1])
            assert torch.equal(frozen["row_draws"][r], anchor), (r, sample_y)
    again = _plain(eng, x, y, v, burn, KEEP, LEAP, seed)      # the metric was cleared
    _same_chain(torch, identity, again)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the class surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", ["identity", "diag"])
def test_predict_individual(torch, tmp_path, mass):
    m = OC.init_model(0, Z_DIMS, P)
    n, burn, keep, q = 96, 40, 20, sum(Z_DIMS)
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    xs = np.linspace(0.0, 3.0, 5)
    kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=3, mass=mass)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c, d = (_causal(tmp_path, m) for _ in range(4))
        mean_a, int_a = a.predict_individual(data, xs, interval="quantile", **kw)                                          # one block
        mean_b, int_b = b.predict_individual(data, xs, interval="quantile", draw_budget_bytes=4 * keep * len(xs) * 32, **kw)      # 32-row blocks
        assert mean_a.shape == (n, 5) and int_a.shape == (n, 5, 2) and a.individual_sd_.shape == (n, 5)
        assert np.array_equal(mean_a, mean_b) and np.array_equal(int_a, int_b) and np.array_equal(a.individual_sd_, b.individual_sd_)
        assert np.array_equal(a.hmc_row_step_, b.hmc_row_step_) and a._seed_counter == b._seed_counter
        seed = _seed_of(a)                                                         # the seed of the call just made
        mean_c, int_c = c.predict_individual(data, xs, groups=np.zeros(n, np.int64), **kw)                                 # interval='normal'
        assert np.array_equal(mean_c, mean_a) and np.array_equal(c.individual_sd_, a.individual_sd_) and a.group_dose_response_ is None
        z = 1.959963984540054                                                      # the 0.975 quantile of the standard normal
        assert np.allclose(int_c[..., 0], mean_c - z * c.individual_sd_, rtol=1e-12) and np.allclose(int_c[..., 1], mean_c + z * c.individual_sd_, rtol=1e-12)
        assert np.all(int_a[..., 0] <= mean_a) and np.all(mean_a <= int_a[..., 1]) and np.all(a.individual_sd_ > 0)
        if mass == "diag":
            assert c.hmc_row_mass_.shape == (n, q) and np.array_equal(c.hmc_row_mass_, a.hmc_row_mass_)
        else:
            assert c.hmc_row_mass_ is None
        adrf, _ = d.predict(data, x_values=xs, sampler="hmc", fused_effects=True, **kw)
        assert np.array_equal(d.hmc_row_step_, c.hmc_row_step_) and d._seed_counter == c._seed_counter
        out = d.engine.hmc_sample(x, y, v, burn, keep, 0.1, 3, seed, want_draws=True, adapt=TARGET, mass=None if mass == "identity" else mass)
        assert seed == _seed_of(d) and np.array_equal(out["row_step"].cpu().numpy(), d.hmc_row_step_)
        big = _largest_outcome_draw(m, out["draws"].cpu().numpy(), xs, seed, burn)
        bound = n * 2.0 ** -24 * big
        err = np.abs(mean_c.mean(axis=0) - adrf).max()
        print("mean over rows of predict_individual against the fused ADRF: %.3g; bound %.3g (Y = %.3f)" % (err, bound, big))
        assert err <= bound
        (label, (mean_g, sd_g)), = c.group_dose_response_.items()                  # one label: the panel's mean curve
        assert label == 0 and np.allclose(mean_g, mean_c.mean(axis=0), rtol=1e-14) and np.abs(mean_g - adrf).max() <= bound
        assert np.allclose(sd_g, np.sqrt((c.individual_sd_ ** 2).sum(axis=0)) / n, rtol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# 8. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks(torch):
    m = _model(51, [1, 1, 1, 7], 20)
    x, y, v = _data(40, 20, 52)
    eng = _engine(m)
    xs = np.linspace(0.0, 3.0, 5)
    with pytest.raises(ValueError, match="row_effects and effect"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, effect=_lib.EFFECT_ADRF, x_values=xs)
    with pytest.raises(ValueError, match="row_effects needs x_values"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True)
    with pytest.raises(ValueError, match="row_draws belongs to row_effects"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_draws=True)
    mb = _model(51, [1, 1, 1, 7], 20, True)
    xb, yb, vb = _data(40, 20, 52, True)
    engb = _engine(mb)
    with pytest.raises(ValueError, match="binary treatment"):
        engb.hmc_sample(xb, yb, vb, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs)
    f = dict(device="cuda", dtype=torch.float32)
    state, grad, logp, step = torch.empty(40, 10, **f), torch.empty(40, 10, **f), torch.empty(40, **f), torch.full((40,), 0.1, **f)
    xv, moments = torch.linspace(0, 3, 5, **f), torch.zeros(3, 5, 40, **f)
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (xb.reshape(-1), yb.reshape(-1), vb))
    with pytest.raises(RuntimeError, match=r"\(-1\).*BGM_EFFECT_ITE"):               # the C entry point on a binary handle
        engb.hmc_run_rows_effects(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, init=True, n_keep=5, x_values=xv, row_moments=moments)
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (x.reshape(-1), y.reshape(-1), v))
    with pytest.raises(RuntimeError, match=r"\(-1\).*row_moments"):
        eng.hmc_run_rows_effects(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, init=True, n_keep=5, x_values=xv)
    with pytest.raises(RuntimeError, match=r"\(-1\).*beyond burn_in \+ n_keep"):
        eng.hmc_run_rows_effects(xt, yt, vt, state, logp, grad, step, 0, 11, 5, 2, 7, init=True, n_keep=5, x_values=xv, row_moments=moments)
    assert not bool(moments.any())
    out = eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs)      # the handle stays usable; no draws of either kind by default
    assert out["draws"] is None and "row_draws" not in out and out["row_mean"].shape == (40, 5)


def test_a_generator_too_deep_for_the_row_kernels_is_refused(torch):
    """the LDS budget of the fused kernels, named in bytes (tests/test_gpu_causal_hmc_fused.py): seven layers of 64 at KT1 = 1"""
    m = _model(71, [1, 1, 1, 7], 20, g_units=(64,) * 7)
    x, y, v = _data(40, 20, 72)
    eng = _engine(m, g_units=[64] * 7)
    with pytest.raises(RuntimeError, match=r"\(-4\).*178320 B.*draws route"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=np.linspace(0.0, 3.0, 5))
