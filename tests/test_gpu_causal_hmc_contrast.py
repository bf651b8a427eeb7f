"""Per-row dose contrasts against a baseline dose, c_i(k) = y_i(x_k) - y_i(x_0), formed inside the CausalBGM HMC sampler
(csrc/causal_hmc_contrast_kernels.h, bgm_causal_hmc_run_row_contrasts; hmc_sample(row_effects=True, row_contrasts=True),
CausalBGM.predict_dose_effect).

Bars:
  chain, curve, cuts, windows, trips, tails, partial rows, class    bit-identity (torch.equal / np.array_equal)
  contrast draws                     bit for bit the float32 difference of the columns k and 0 of the row_draws of the row_effects
                                     run at the same seed, at every dose count where the pass structure of the kernel changes
  contrast moments                   against float64 mean / sd (ddof 1) of the run's own contrast_draws, inside the two derived
                                     bounds of tests/_causal_hmc_contrast_ref.py (the worst ratios are printed)
  float64 anchor                     contrast_draws against the difference of two float64 oracle values on the returned latent
                                     draws: 4e-4 absolute, twice the 2e-4 tests/test_gpu_causal_hmc_rowfx.py grants one value
The models are the small ones of tests/test_gpu_causal_hmc_tails.py, both first-layer tilings."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_contrast_ref as CR  # noqa: E402
import _causal_partial_ref as PR  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402
from tests.test_gpu_causal_hmc_fused import P, Z_DIMS, _causal  # noqa: E402
from tests.test_gpu_causal_hmc_rowfx import _oracle_rows  # noqa: E402
from tests.test_gpu_causal_hmc_tails import _tails_are_sorted_draws  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
BURN, KEEP, LEAP, STEP0 = 30, 20, 3, 0.1
SHAPES = [dict(z_dims=[1, 1, 1, 7], p=20), dict(z_dims=[3, 3, 6, 6], p=20)]      # both first-layer tilings (KT1 = 1, 2)
KEYS = ("draws", "state", "logp", "grad", "row_step", "acc_count")
N = 200                                                                             # 13 tiles, the last one of 8 rows
# 1: the baseline alone; 3: a ragged pass; 5: a second, shared pass that must still see pass 0's baseline; 16: four passes whose
# noise is the lane groups' own; 18: those and one shared pass; 33: a second block of own passes
DOSES = (1, 3, 5, 16, 18, 33)
M_K_ALPHA = [(1, 1, 0.5), (20, 1, None), (20, 3, 0.1), (20, 20, 0.5), (400, 17, 0.05)]      # alpha None: K = 1 is below what any bound reads
_ENGINES = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _id(case):
    return "q%d" % sum(case["z_dims"])


def _setup(case, seed=31):
    """(model, engine) of a shape, built once for the module"""
    key = (tuple(case["z_dims"]), case["p"], seed)
    if key not in _ENGINES:
        m = _model(seed, case["z_dims"], case["p"])
        _ENGINES[key] = (m, _engine(m))
    return _ENGINES[key]


def _doses(n_doses):
    return np.linspace(0.5, 3.0, n_doses)                                # the baseline is dose 0, here 0.5


def _rows(eng, x, y, v, burn, keep, leap, seed, xs, sample_y=True, want_draws=True, row_draws=True, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, want_draws=want_draws, adapt=TARGET, row_effects=True, row_draws=row_draws,
                          x_values=xs, sample_y=sample_y, **kw)


def _con(eng, *args, **kw):
    return _rows(eng, *args, row_contrasts=True, **kw)


def _difference(rows):
    """the float32 difference of every column of the row_effects run's draws to its column 0: [n, n_doses, m]"""
    y = rows["row_draws"]
    return y - y[:, :1]


def _same_contrasts(torch, a, b, rows=slice(None)):
    for k in ("row_mean", "row_sd", "contrast_mean", "contrast_sd", "contrast_draws"):
        assert torch.equal(a[k][rows], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 1. the chain and the curve are unchanged
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, "diag"], ids=["identity", "metric"])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_chain_and_curve_unchanged(torch, case, mass):
    seed, burn = 99, 40
    _, eng = _setup(case)
    x, y, v = _data(N, case["p"], 32)
    xs = _doses(18)
    for sample_y in (True, False):
        rows = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass)
        con = _con(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass)
        for k in KEYS + ("row_mean", "row_sd") + (("mass_scale",) if mass else ()):
            assert torch.equal(rows[k], con[k]), (k, sample_y)
        assert ("mass_scale" in con) == (mass is not None)
        assert "row_draws" not in con and "contrast_mean" not in rows and "contrast_draws" not in rows
        assert con["contrast_mean"].shape == con["contrast_sd"].shape == (N, 18) and con["contrast_mean"].dtype == torch.float64
        assert torch.equal(con["contrast_draws"], _difference(rows)), sample_y


# ---------------------------------------------------------------------------------------------------------------------
# 2. the contrast draws are the difference of the row_effects run's draws
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_doses", DOSES)
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_contrast_draws_equal_the_difference_of_the_row_draws(torch, case, n_doses):
    seed = 4711 + n_doses
    _, eng = _setup(case)
    x, y, v = _data(N, case["p"], 32)
    xs = _doses(n_doses)
    for sample_y in (True, False):
        rows = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, want_draws=False)
        con = _con(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, want_draws=False)
        got, want = con["contrast_draws"], _difference(rows)
        assert got.shape == (N, n_doses, KEEP) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        bad = (got != want).any(dim=-1).any(dim=0)                        # per dose
        assert not bool(bad.any()), (sample_y, "doses that differ: %r" % (bad.nonzero().reshape(-1).tolist(),))
        # the baseline against itself: exactly zero on every draw, in the draws and in every plane
        assert not bool(got[:, 0].any()) and not bool(con["contrast_mean"][:, 0].any()) and not bool(con["contrast_sd"][:, 0].any())
        if n_doses > 1:
            assert bool((got[:, 1:] != 0).any(dim=-1).all())
        assert torch.equal(con["row_mean"], rows["row_mean"]) and torch.equal(con["row_sd"], rows["row_sd"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the contrast moments are those of the contrast draws
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [20, 400])
def test_contrast_moments_are_inside_the_derived_bounds(torch, keep):
    worst = [0.0, 0.0]
    for case in SHAPES:
        _, eng = _setup(case, 51)
        x, y, v = _data(N, case["p"], 52)
        for sample_y in (True, False):
            out = _con(eng, x, y, v, BURN, keep, LEAP, 5, _doses(18 if keep == 20 else 5), sample_y, want_draws=False)
            c = out["contrast_draws"].cpu().numpy()
            r_mean, r_var, inside = CR.worst_ratios(out["contrast_mean"].cpu().numpy(), out["contrast_sd"].cpu().numpy(), c)
            print("contrast moments q%d sample_y=%d m=%d: worst |mean - ref| / bound %.3g, worst |var - ref| / bound %.3g; largest |c| %.3f, "
                  "largest sd %.3f" % (sum(case["z_dims"]), sample_y, keep, r_mean, r_var, np.abs(c).max(), float(out["contrast_sd"].max())))
            worst = [max(worst[0], r_mean), max(worst[1], r_var)]
            assert inside, (case, sample_y)
            if keep > 1:
                assert bool((out["contrast_sd"][:, 1:] > 0).any())
    print("m = %d: worst ratios over the cases: mean %.3g, variance %.3g" % (keep, worst[0], worst[1]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the float64 anchor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_y", [True, False], ids=["noise", "mean"])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_contrast_draws_match_the_float64_oracle(torch, case, sample_y):
    seed = 5
    m, eng = _setup(case, 51)
    x, y, v = _data(N, case["p"], 52)
    xs = _doses(18)
    out = _con(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y)
    ref = _oracle_rows(m, out["draws"].cpu().numpy(), xs, sample_y, seed, BURN)
    ref = ref - ref[:, :1]
    got = out["contrast_draws"].cpu().numpy()
    err = np.abs(got - ref).max(axis=(0, 2))
    print("contrasts q%d sample_y=%d against the float64 oracle: worst %.3g (bar 4e-4), largest |c| %.3f" %
          (sum(case["z_dims"]), sample_y, err.max(), np.abs(ref).max()))
    assert err.max() <= 4e-4 and err[0] == 0.0
    assert np.abs(out["contrast_mean"].cpu().numpy() - ref.mean(axis=-1)).max() <= 4e-4


# ---------------------------------------------------------------------------------------------------------------------
# 5. the tails are those of the contrast series
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_k_alpha", M_K_ALPHA, ids=lambda mk: "m%d-K%d" % mk[:2])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_tails_are_those_of_the_contrast_series(torch, case, m_k_alpha):
    keep, K, alpha = m_k_alpha
    burn, leap, seed, n, n_doses = 6, 2, 4711 + keep, 33, 18
    _, eng = _setup(case)
    x, y, v = _data(n, case["p"], 32 + n)
    xs = _doses(n_doses)
    ties = 0
    for sample_y in (True, False):                  # False: a rejected transition repeats the value exactly
        plain = _con(eng, x, y, v, burn, keep, leap, seed, xs, sample_y, want_draws=False)
        out = _con(eng, x, y, v, burn, keep, leap, seed, xs, sample_y, want_draws=False, row_tails=K)
        _same_contrasts(torch, plain, out)          # the tails change nothing else
        assert "tails" not in plain
        c = out["contrast_draws"]
        _tails_are_sorted_draws(torch, dict(tails=out["tails"], row_draws=c), K, (sample_y,))
        assert not bool(out["tails"][:, :, 0].any())                      # dose 0: every value ties at zero
        if not sample_y and keep > 1:
            ties += int((c[:, 1:, 1:] == c[:, 1:, :-1]).sum())
        if alpha is not None:
            assert HM.tail_size(alpha, keep) <= K
            q_lo, q_hi = alpha / 2, 1 - alpha / 2
            _, lo_d, hi_d = eng.row_mean_quantiles(c.reshape(n * n_doses, keep), q_lo, q_hi)
            lo_t, hi_t = eng.row_tail_quantiles(out["tails"], keep, q_lo, q_hi)
            assert torch.equal(lo_t.t().reshape(-1), lo_d) and torch.equal(hi_t.t().reshape(-1), hi_d), sample_y
        moments_only = _con(eng, x, y, v, burn, keep, leap, seed, xs, sample_y, want_draws=False, row_draws=False, row_tails=K)
        assert "contrast_draws" not in moments_only and torch.equal(moments_only["tails"], out["tails"])      # the draws are not needed
    assert keep == 1 or ties > 0                    # the runs without noise did hold repeated values


# ---------------------------------------------------------------------------------------------------------------------
# 6. launch cuts, row windows, trips of the tile loop, guard bands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_launch_cuts_and_row_windows_change_nothing(torch, case):
    seed, K = 4711, 9
    _, eng = _setup(case, 41)
    x, y, v = _data(N, case["p"], 42)
    xs = _doses(18)
    for sample_y in (True, False):
        one = _con(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, row_tails=K)
        for chunk in (4, 1):                        # 4: launches end at 28 | 32 across burn_in = 30; 1: one iteration a launch
            cut = _con(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, row_tails=K, chunk=chunk)
            for k in KEYS:
                assert torch.equal(one[k], cut[k]), (k, chunk)
            _same_contrasts(torch, one, cut)
            assert torch.equal(one["tails"], cut["tails"]), chunk         # slot for slot, not only as sets
    a, e = 23, 171                                                        # rows [a, e) alone with their global row index
    part = _con(eng, x[a:e], y[a:e], v[a:e], BURN, KEEP, LEAP, seed, xs, False, row_base=a, row_tails=K)
    _same_contrasts(torch, one, part, slice(a, e))
    assert torch.equal(part["tails"], one["tails"][..., a:e]) and torch.equal(part["draws"], one["draws"][:, a:e])


def test_rows_beyond_one_trip_of_the_tile_loop(torch):
    """16 x 8 x CUs x 2 + 37 rows: every wave slot walks two or three tiles, the last tile is ragged"""
    case = SHAPES[0]
    burn, keep, leap, seed, K = 3, 5, 2, 4242, 2
    _, eng = _setup(case, 65)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus * 2 + 37
    assert eng.mh_slots(n) == waves * n_cus and (n + 15) // 16 == 2 * waves * n_cus + 3
    x, y, v = _data(n, case["p"], 66)
    xs = _doses(5)
    rows = _rows(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False)
    out = _con(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False, row_tails=K)
    assert torch.equal(out["contrast_draws"], _difference(rows)) and torch.equal(out["row_mean"], rows["row_mean"])
    _tails_are_sorted_draws(torch, dict(tails=out["tails"], row_draws=out["contrast_draws"]), K, "three trips")
    chunked = _con(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False, row_tails=K, chunk=2)
    _same_contrasts(torch, out, chunked)
    assert torch.equal(out["tails"], chunked["tails"])
    for a, e in ((0, 16), (16 * waves * n_cus - 5, 16 * waves * n_cus + 21), (n - 40, n)):      # the first tile; across the first two trips; the ragged end
        part = _con(eng, x[a:e], y[a:e], v[a:e], burn, keep, leap, seed, xs, want_draws=False, row_base=a, row_tails=K)
        _same_contrasts(torch, out, part, slice(a, e))
        assert torch.equal(part["tails"], out["tails"][..., a:e]), (a, e)


@pytest.mark.parametrize("n_doses", [5, 18])
def test_nothing_is_written_outside_the_buffers(torch, n_doses):
    """A ragged panel (n = 17: fifteen padding lanes in the second tile) and a padded dose pass write nothing: every buffer of the
    call lies between two guard bands.  The launches of the burn-in write nothing at all, and a run cut at every iteration leaves
    every raw plane, draw and tail slot bit-identical to one launch."""
    case = SHAPES[0]
    _, eng = _setup(case)
    n, K, burn, keep, leap, guard, mark = 17, 3, 4, 6, 2, 4096, -12345.0
    x, y, v = (torch.from_numpy(a).cuda() for a in _data(n, case["p"], 32))
    x, y = x.reshape(-1), y.reshape(-1)
    f = dict(device="cuda", dtype=torch.float32)
    q = sum(case["z_dims"])
    xv = torch.from_numpy(_doses(n_doses).astype(np.float32)).cuda()
    shapes = dict(row_moments=(3, n_doses, n), row_cmoments=(3, n_doses, n), contrast_draws=(n, n_doses, keep), contrast_tails=(2, K, n_doses, n))

    def run(cuts):
        flats = {k: torch.full((2 * guard + int(np.prod(s)),), mark, **f) for k, s in shapes.items()}
        bufs = {k: flats[k][guard:-guard].view(*s) for k, s in shapes.items()}
        state, grad, logp, step = torch.empty(n, q, **f), torch.empty(n, q, **f), torch.empty(n, **f), torch.full((n,), 0.1, **f)
        kw = dict(n_keep=keep, x_values=xv, **bufs)
        eng.hmc_run_rows_contrasts(x, y, v, state, logp, grad, step, 0, burn, burn, leap, 7, init=True, **kw)
        torch.cuda.synchronize()
        assert all(bool((fl == mark).all()) for fl in flats.values())      # burn-in: nothing is sampled into any buffer
        for a, e in zip(cuts[:-1], cuts[1:]):
            eng.hmc_run_rows_contrasts(x, y, v, state, logp, grad, step, a, e - a, burn, leap, 7, **kw)
        torch.cuda.synchronize()
        for k, fl in flats.items():
            assert bool((fl[:guard] == mark).all()) and bool((fl[-guard:] == mark).all()), k
            assert bool((bufs[k] != mark).all()), k                         # and every element inside was written
        return bufs, state
    one, state_one = run([burn, burn + keep])
    each, state_each = run(list(range(burn, burn + keep + 1)))
    assert torch.equal(state_one, state_each)
    for k in shapes:
        assert torch.equal(one[k], each[k]), k
    assert not bool(one["row_cmoments"][:, 0].any()) and not bool(one["contrast_draws"][:, 0].any())
    _tails_are_sorted_draws(torch, dict(tails=one["contrast_tails"], row_draws=one["contrast_draws"]), K)
    # the same run through hmc_sample's own buffers, and the curve planes of the entry point without contrasts
    xs = xv.cpu().numpy()
    ref = eng.hmc_sample(x, y, v, burn, keep, 0.1, leap, 7, adapt=None, row_effects=True, row_draws=True, x_values=xs, row_tails=K, row_contrasts=True)
    assert torch.equal(ref["tails"], one["contrast_tails"]) and torch.equal(ref["contrast_draws"], one["contrast_draws"])
    mean, sd = HM.row_moments_finalize(*one["row_cmoments"], keep)
    assert torch.equal(ref["contrast_mean"], mean.t()) and torch.equal(ref["contrast_sd"], sd.t())
    state, grad, logp, step = torch.empty(n, q, **f), torch.empty(n, q, **f), torch.empty(n, **f), torch.full((n,), 0.1, **f)
    moments = torch.zeros(3, n_doses, n, **f)
    eng.hmc_run_rows_effects(x, y, v, state, logp, grad, step, 0, burn + keep, burn, leap, 7, init=True, n_keep=keep, x_values=xv, row_moments=moments)
    assert torch.equal(moments, one["row_moments"]) and torch.equal(state, state_one)


# ---------------------------------------------------------------------------------------------------------------------
# 7. partially observed rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, "diag"], ids=["identity", "metric"])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_partial_rows(torch, case, mass):
    seed, burn, K = 99, 40, 4
    _, eng = _setup(case)
    x0, y0, v = _data(N, case["p"], 32)
    x, y = PR.mixed_panel(x0, y0, 34)                                     # the three observation patterns inside every tile
    assert np.isnan(y).sum() > np.isnan(x).sum() > 0 and not np.isnan(y).all()
    xs = _doses(5)
    for sample_y in (True, False):
        rows = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass, partial=True)
        con = _con(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass, partial=True, row_tails=K)
        for k in KEYS + ("row_mean", "row_sd") + (("mass_scale",) if mass else ()):
            assert torch.equal(rows[k], con[k]), (k, sample_y)
        assert torch.equal(con["contrast_draws"], _difference(rows)), sample_y
        _tails_are_sorted_draws(torch, dict(tails=con["tails"], row_draws=con["contrast_draws"]), K, (mass, sample_y))
    # a fully observed panel under partial=True is the run of partial=False
    full = _con(eng, x0, y0, v, burn, KEEP, LEAP, seed, xs, False, mass=mass, row_tails=K)
    same = _con(eng, x0, y0, v, burn, KEEP, LEAP, seed, xs, False, mass=mass, row_tails=K, partial=True)
    for k in KEYS:
        assert torch.equal(full[k], same[k]), k
    _same_contrasts(torch, full, same)
    assert torch.equal(full["tails"], same["tails"]) and not torch.equal(full["state"], con["state"])      # the pattern did reach the kernel


# ---------------------------------------------------------------------------------------------------------------------
# 8. the class surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", ["identity", "diag"])
def test_predict_dose_effect(torch, tmp_path, mass):
    m = OC.init_model(0, Z_DIMS, P)
    n, burn, keep, alpha, base = 96, 40, 20, 0.2, 0.5
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    xs = np.linspace(1.0, 3.0, 5)
    K = HM.tail_size(alpha, keep)
    assert 1 < K < keep
    kw = dict(alpha=alpha, n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=3, mass=mass)
    groups = np.arange(n) % 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ind, a, b, c, d = (_causal(tmp_path, m) for _ in range(5))
        curve_mean, _ = ind.predict_individual(data, np.concatenate([[base], xs]), **kw)
        eff_q, int_q = a.predict_dose_effect(data, xs, base, interval="quantile", **kw)
        eff_t, int_t = b.predict_dose_effect(data, xs, base, interval="tails", groups=groups, **kw)                                  # one block
        eff_s, int_s = c.predict_dose_effect(data, xs, base, interval="tails", draw_budget_bytes=8 * K * (len(xs) + 1) * 32, **kw)   # 32-row blocks
        eff_n, int_n = d.predict_dose_effect(data, xs, base, groups=groups, **kw)                                                    # interval='normal'
    assert eff_q.shape == (n, 5) and int_q.shape == (n, 5, 2) and eff_q.dtype == int_q.dtype == np.float64
    for model in (a, b, c, d):          # the curve at [baseline] + x_values is predict_individual's, bit for bit
        assert np.array_equal(model.dose_effect_curve_[0], curve_mean) and np.array_equal(model.dose_effect_curve_[1], ind.individual_sd_)
        assert model.dose_effect_sd_.shape == (n, 5) and np.array_equal(model.dose_effect_sd_, d.dose_effect_sd_)
        assert np.array_equal(model.hmc_row_step_, ind.hmc_row_step_) and model._seed_counter == ind._seed_counter
        assert (model.hmc_row_mass_ is None) == (mass == "identity") and model.individual_sd_ is None
    assert np.array_equal(eff_q, eff_n) and np.array_equal(eff_t, eff_n) and np.array_equal(eff_s, eff_n)
    assert np.array_equal(int_t, int_q) and np.array_equal(int_s, int_q)                       # the bounds of 'quantile', bit for bit
    assert not np.array_equal(int_t, int_n) and np.all(int_q[..., 0] <= int_q[..., 1]) and np.all(d.dose_effect_sd_ > 0)
    z = 1.2815515655446004                                                                     # the 0.9 quantile of the standard normal
    assert np.allclose(int_n[..., 0], eff_n - z * d.dose_effect_sd_, rtol=1e-12) and np.allclose(int_n[..., 1], eff_n + z * d.dose_effect_sd_, rtol=1e-12)
    # the effect is the difference of the curve's means up to the float32 sums, and its sd is NOT what the marginal sds give
    assert np.abs(eff_n - (curve_mean[:, 1:] - curve_mean[:, :1])).max() <= 1e-4
    marginal = np.sqrt(ind.individual_sd_[:, 1:] ** 2 + ind.individual_sd_[:, :1] ** 2)
    assert not np.allclose(d.dose_effect_sd_, marginal, rtol=1e-3)
    want = HM.group_dose_response(eff_n, d.dose_effect_sd_, groups)
    assert sorted(b.group_dose_effect_) == [0, 1, 2] and a.group_dose_effect_ is None and c.group_dose_effect_ is None
    for g in (0, 1, 2):
        for model in (b, d):
            assert all(np.array_equal(p_, q_) for p_, q_ in zip(model.group_dose_effect_[g], want[g]))
    # new units: the outcome of no row observed, the treatment of three rows in four
    x_some, y_none = x.copy(), np.full_like(y, np.nan)
    x_some[::4] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        new, e = _causal(tmp_path, m), _causal(tmp_path, m)
        new_curve, _ = new.predict_new(v, x_some.ravel(), np.concatenate([[base], xs]), **kw)
        eff_p, int_p = e.predict_dose_effect((x_some, y_none, v), xs, base, interval="tails", partial=True, **kw)
    assert np.array_equal(e.dose_effect_curve_[0], new_curve) and not np.array_equal(eff_p, eff_n) and int_p.shape == (n, 5, 2)


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(torch, tmp_path):
    case = SHAPES[0]
    _, eng = _setup(case, 51)
    x, y, v = _data(40, 20, 52)
    xs = _doses(5)
    f = dict(device="cuda", dtype=torch.float32)
    state, grad, logp, step = torch.empty(40, 10, **f), torch.empty(40, 10, **f), torch.empty(40, **f), torch.full((40,), 0.1, **f)
    xv, moments, cmoments = torch.linspace(0, 3, 5, **f), torch.zeros(3, 5, 40, **f), torch.zeros(3, 5, 40, **f)
    tails = torch.zeros(2, 2, 5, 40, **f)
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (x.reshape(-1), y.reshape(-1), v))
    run = dict(init=True, n_keep=5, x_values=xv, row_moments=moments)
    call = (xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7)
    # a trajectory option set on the handle: BGM_E_UNSUPPORTED naming it, before anything else is looked at
    for setting, word in (((1.0, False, None), "max_trajectory"), ((None, True, None), "jitter"),
                          ((None, False, torch.zeros(40, device="cuda", dtype=torch.int32)), "n_steps_dev")):
        eng.set_hmc_trajectory(*setting)
        try:
            with pytest.raises(RuntimeError, match=r"bgm_causal_hmc_run_row_contrasts failed \(-4\).*dose-contrast kernels.*%s is set" % word):
                eng.hmc_run_rows_contrasts(*call, row_cmoments=cmoments, **run)
        finally:
            eng.set_hmc_trajectory(None)
    with pytest.raises(RuntimeError, match=r"\(-1\).*row_cmoments_dev required"):
        eng.hmc_run_rows_contrasts(*call, **run)
    with pytest.raises(RuntimeError, match=r"\(-1\).*row_moments"):
        eng.hmc_run_rows_contrasts(*call, init=True, n_keep=5, x_values=xv, row_cmoments=cmoments)
    with pytest.raises(RuntimeError, match=r"\(-1\).*k_tail must be in \[1, n_keep\] = \[1, 5\]; got 6"):
        eng.hmc_run_rows_contrasts(*call, row_cmoments=cmoments, contrast_tails=torch.zeros(2, 6, 5, 40, **f), **run)
    lib_args = eng._hmc_args(*call[:12], True, 0, None, None, 0.0, 1.0, None, None, 5)      # k_tail = 0 with a tails buffer: the C ABI itself
    rc = eng.lib.bgm_causal_hmc_run_row_contrasts(*lib_args, 1, xv.data_ptr(), 5, moments.data_ptr(), cmoments.data_ptr(), None,
                                                  tails.data_ptr(), 0, eng._stream())
    assert rc == -1
    with pytest.raises(RuntimeError, match=r"\(-1\).*beyond burn_in \+ n_keep"):
        eng.hmc_run_rows_contrasts(xt, yt, vt, state, logp, grad, step, 0, 11, 5, 2, 7, row_cmoments=cmoments, **run)
    with pytest.raises(ValueError, match=r"contrast_tails must be .*\[2, K, 5, 40\]"):
        eng.hmc_run_rows_contrasts(*call, row_cmoments=cmoments, contrast_tails=torch.zeros(2, 2, 5, 39, **f), **run)
    mb = _model(51, [1, 1, 1, 7], 20, True)
    xb, yb, vb = _data(40, 20, 52, True)
    engb = _engine(mb)
    xbt, ybt, vbt = (torch.from_numpy(a).cuda() for a in (xb.reshape(-1), yb.reshape(-1), vb))
    with pytest.raises(RuntimeError, match=r"\(-1\).*BGM_EFFECT_ITE"):      # the C entry point on a binary handle
        engb.hmc_run_rows_contrasts(xbt, ybt, vbt, state, logp, grad, step, 0, 10, 5, 2, 7, row_cmoments=cmoments, contrast_tails=tails, **run)
    assert not bool(moments.any()) and not bool(cmoments.any()) and not bool(tails.any())
    # the engine's own refusals
    with pytest.raises(ValueError, match="binary treatment"):
        engb.hmc_sample(xb, yb, vb, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_contrasts=True)
    with pytest.raises(ValueError, match="row_contrasts belongs to row_effects"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_contrasts=True)
    with pytest.raises(ValueError, match="not available with row_contrasts"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_contrasts=True, jitter=True)
    for bad in (0, 6, 2.5, True):
        with pytest.raises(ValueError, match=r"row_tails must be an integer K with 1 <= K <= n_keep = 5"):
            eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_contrasts=True, row_tails=bad)
    out = eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_contrasts=True, row_tails=5)      # the handle stays usable
    assert out["tails"].shape == (2, 5, 5, 40) and "contrast_draws" not in out and out["contrast_mean"].shape == (40, 5)
    # the LDS budget of the fused kernels, named in bytes: seven layers of 64 at KT1 = 1
    deep = _model(71, [1, 1, 1, 7], 20, g_units=(64,) * 7)
    with pytest.raises(RuntimeError, match=r"\(-4\).*178320 B.*draws route"):
        _engine(deep, g_units=[64] * 7).hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_contrasts=True)
    # the class: a binary treatment has the ITE
    mbin = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = _causal(tmp_path, mbin, binary=True)
        with pytest.raises(ValueError, match="predict's ITE"):
            model.predict_dose_effect(_data(8, P, 8, True), xs, 0.0, n_mcmc=5, burn_in=5, verbose=0)
