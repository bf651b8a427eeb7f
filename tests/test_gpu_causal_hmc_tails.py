"""interval='tails': the CausalBGM HMC sampler with the K smallest and the K largest values of every (row, dose) series kept inside the
kernel (csrc/causal_hmc_tails_kernels.h, bgm_causal_hmc_run_row_tails, bgm_row_tail_quantiles; hmc_sample(row_effects=True,
row_tails=K), CausalBGM.predict_individual / predict_new(interval='tails')).

Every bar is bit-identity (torch.equal / np.array_equal): the tails are a selection of the run's own draws and the bounds apply the
arithmetic of bgm_row_mean_quantiles to them, so nothing is rounded differently on the two routes.  Draws and tails always come from
ONE run (row_draws=True with row_tails=K).  The models are the small ones of tests/test_gpu_causal_hmc_rowfx.py, both first-layer
tilings."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_partial_ref as PR  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402
from tests.test_gpu_causal_hmc_fused import P, Z_DIMS, _causal  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
BURN, KEEP, LEAP, STEP0 = 30, 20, 3, 0.1
SHAPES = [dict(z_dims=[1, 1, 1, 7], p=20), dict(z_dims=[3, 3, 6, 6], p=20)]      # both first-layer tilings (KT1 = 1, 2)
KEYS = ("draws", "state", "logp", "grad", "row_step", "acc_count")
N = 200                                                                             # 13 tiles, the last one of 8 rows
M_K = [(1, 1), (6, 6), (7, 3), (40, 1), (40, 2), (400, 17)]                         # K = m: fill only; K = 1: a heap of its root alone
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


def _rows(eng, x, y, v, burn, keep, leap, seed, xs, sample_y=True, want_draws=True, row_draws=True, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, want_draws=want_draws, adapt=TARGET, row_effects=True, row_draws=row_draws,
                          x_values=xs, sample_y=sample_y, **kw)


def _same_run(torch, rows, tails):
    """check 1: chain, moments and draws of the tails run are those of the row_effects run"""
    for k in KEYS + ("row_mean", "row_sd", "row_draws") + (("mass_scale",) if "mass_scale" in rows else ()):
        assert torch.equal(rows[k], tails[k]), k
    assert "tails" not in rows


def _tails_are_sorted_draws(torch, out, K, what=""):
    """check 2: as multisets tail 0 is the K smallest and tail 1 the K largest of the series' draws, and slot 0 is the threshold"""
    tails, draws = out["tails"], out["row_draws"]                        # [2, K, n_doses, n], [n, n_doses, m]
    n, n_doses, m = draws.shape
    assert tails.shape == (2, K, n_doses, n) and tails.dtype == torch.float32 and bool(torch.isfinite(tails).all()), what
    srt = draws.sort(dim=-1).values.permute(2, 1, 0)                     # [m, n_doses, n]
    got = tails.sort(dim=1).values
    assert torch.equal(got[0], srt[:K]), what
    assert torch.equal(got[1], srt[m - K:]), what
    assert torch.equal(tails[0, 0], srt[K - 1]) and torch.equal(tails[1, 0], srt[m - K]), what


# ---------------------------------------------------------------------------------------------------------------------
# 1. the chain, the moments and the draws are unchanged
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, "diag"], ids=["identity", "metric"])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_chain_moments_and_draws_unchanged(torch, case, mass):
    seed, burn = 99, 40
    _, eng = _setup(case)
    x, y, v = _data(N, case["p"], 32)
    xs = np.linspace(0.0, 3.0, 17)
    for sample_y in (True, False):
        rows = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass)
        tails = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass, row_tails=5)
        _same_run(torch, rows, tails)
        assert ("mass_scale" in tails) == (mass is not None)
        _tails_are_sorted_draws(torch, tails, 5, (mass, sample_y))
    moments_only = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, False, want_draws=False, row_draws=False, mass=mass, row_tails=5)
    assert "row_draws" not in moments_only and torch.equal(moments_only["tails"], tails["tails"])      # the draws are not needed


# ---------------------------------------------------------------------------------------------------------------------
# 2. the tails are the sorted draws
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_k", M_K, ids=lambda mk: "m%d-K%d" % mk)
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_tails_equal_sorted_draws(torch, case, m_k):
    keep, K = m_k
    burn, leap, seed = 6, 2, 4711 + keep
    _, eng = _setup(case)
    ties = 0
    for n in (1, 16, 17, 33):                       # one row, one tile, a ragged second tile, a ragged third one
        x, y, v = _data(n, case["p"], 32 + n)
        for n_doses in (1, 5, 17, 20):              # 17, 20: lane groups with a Philox call of their own, and the shared remainder
            if keep == 400 and (n, n_doses) not in ((1, 20), (16, 17), (17, 5), (33, 20), (33, 1)):
                continue                            # (the long run at one pairing of every n and every dose count)
            xs = np.linspace(0.0, 3.0, n_doses)
            for sample_y in (True, False):          # False: a rejected transition repeats the value exactly
                out = _rows(eng, x, y, v, burn, keep, leap, seed, xs, sample_y, want_draws=False, row_tails=K)
                _tails_are_sorted_draws(torch, out, K, (n, n_doses, sample_y))
                if not sample_y and keep > 1:
                    ties += int((out["row_draws"][..., 1:] == out["row_draws"][..., :-1]).sum())
    assert keep == 1 or ties > 0                    # the runs without noise did hold repeated values


# ---------------------------------------------------------------------------------------------------------------------
# 3. launch cuts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_launch_cuts_leave_the_raw_buffers_unchanged(torch, case):
    """chunk = 7 with burn_in = 30: launches end at 28, 35 (draw 5: inside the fill phase of K = 9), 42 (draw 12: after it), 49"""
    seed, K = 4711, 9
    _, eng = _setup(case, 41)
    x, y, v = _data(N, case["p"], 42)
    xs = np.linspace(0.0, 3.0, 17)
    for sample_y in (True, False):
        one = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, row_tails=K)
        cut = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, row_tails=K, chunk=7)
        _same_run(torch, {k: v_ for k, v_ in one.items() if k != "tails"}, cut)
        assert torch.equal(one["tails"], cut["tails"])                    # slot for slot, not only as sets
        _tails_are_sorted_draws(torch, cut, K, sample_y)
    each = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, False, row_tails=K, chunk=1)
    assert torch.equal(one["tails"], each["tails"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. row windows and a second trip of the tile loop
# ---------------------------------------------------------------------------------------------------------------------
def test_row_windows_and_a_second_trip(torch):
    case = SHAPES[0]
    seed, K = 4711, 4
    _, eng = _setup(case, 41)
    x, y, v = _data(N, case["p"], 42)
    xs = np.linspace(0.0, 3.0, 5)
    one = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, row_tails=K)
    a, e = 23, 171                                                        # rows [a, e) alone with their global row index
    part = _rows(eng, x[a:e], y[a:e], v[a:e], BURN, KEEP, LEAP, seed, xs, row_base=a, row_tails=K)
    assert torch.equal(part["tails"].sort(dim=1).values, one["tails"][..., a:e].sort(dim=1).values)
    assert torch.equal(part["tails"], one["tails"][..., a:e])            # a series' buffer depends on its draw sequence alone
    # 16 x waves x CUs + 17 rows: every wave slot walks one tile and the first two a second one, the last of them ragged
    burn, keep, leap, K = 3, 5, 2, 2
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus + 17
    assert eng.mh_slots(n) == waves * n_cus and (n + 15) // 16 == waves * n_cus + 2
    x, y, v = _data(n, case["p"], 66)
    out = _rows(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False, row_tails=K)
    _tails_are_sorted_draws(torch, out, K, "two trips")
    for a, e in ((0, 16), (16 * waves * n_cus - 5, n)):                   # the first tile; the end of the first trip with the second
        part = _rows(eng, x[a:e], y[a:e], v[a:e], burn, keep, leap, seed, xs, want_draws=False, row_base=a, row_tails=K)
        assert torch.equal(part["tails"].sort(dim=1).values, out["tails"][..., a:e].sort(dim=1).values), (a, e)


# ---------------------------------------------------------------------------------------------------------------------
# 5. guard bands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_doses", [5, 17])
def test_nothing_is_written_outside_the_buffer(torch, n_doses):
    """A ragged panel (n = 17: fifteen padding lanes in the second tile) and a padded dose pass write nothing: a padding lane's store
    would land in the columns of the next dose or slot, or behind the buffer.  The buffer lies between two guard bands, and the
    launches of the burn-in write nothing at all: no row is sampled into it before iteration burn_in."""
    case = SHAPES[0]
    _, eng = _setup(case)
    n, K, burn, keep, leap, guard, mark = 17, 3, 4, 6, 2, 4096, -12345.0
    x, y, v = (torch.from_numpy(a).cuda() for a in _data(n, case["p"], 32))
    x, y = x.reshape(-1), y.reshape(-1)
    f = dict(device="cuda", dtype=torch.float32)
    q = sum(case["z_dims"])
    state, grad, logp, step = torch.empty(n, q, **f), torch.empty(n, q, **f), torch.empty(n, **f), torch.full((n,), 0.1, **f)
    xv = torch.linspace(0, 3, n_doses, **f)
    size = 2 * K * n_doses * n
    flat = torch.full((guard + size + guard,), mark, **f)
    tails = flat[guard:guard + size].view(2, K, n_doses, n)
    moments, draws = torch.zeros(3, n_doses, n, **f), torch.empty(n, n_doses, keep, **f)
    kw = dict(n_keep=keep, x_values=xv, row_moments=moments, row_draws=draws, row_tails=tails)
    eng.hmc_run_rows_tails(x, y, v, state, logp, grad, step, 0, burn, burn, leap, 7, init=True, **kw)
    torch.cuda.synchronize()
    assert bool((flat == mark).all())                                     # burn-in: nothing is sampled into the buffer
    eng.hmc_run_rows_tails(x, y, v, state, logp, grad, step, burn, keep, burn, leap, 7, **kw)
    torch.cuda.synchronize()
    assert bool((flat[:guard] == mark).all()) and bool((flat[guard + size:] == mark).all())
    assert bool((tails != mark).all())                                    # every slot of every series was filled (K <= keep)
    _tails_are_sorted_draws(torch, dict(tails=tails, row_draws=draws), K)
    # the same run through hmc_sample's own buffer
    ref = eng.hmc_sample(x, y, v, burn, keep, 0.1, leap, 7, adapt=None, row_effects=True, row_draws=True, x_values=xv.cpu().numpy(), row_tails=K)
    assert torch.equal(ref["tails"], tails) and torch.equal(ref["row_draws"], draws)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the bounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,keep", [(0.01, 40), (0.05, 40), (0.5, 40), (0.9, 101), (0.1, 21), (0.05, 400), (0.9, 7), (0.01, 1)])
def test_bounds_equal_the_quantiles_of_the_draws(torch, alpha, keep):
    """(0.9, 101): 0.55 * 100 is integral in exact arithmetic and 55.00000000000001 in double (tests/test_causal_hmc_tails_host.py);
    (0.1, 21): both products are integral and exact"""
    case = SHAPES[1]
    _, eng = _setup(case)
    burn, leap, seed, n = 6, 2, 17, 33
    K = HM.tail_size(alpha, keep)
    assert {(0.1, 21): 3, (0.9, 101): 47}.get((alpha, keep), K) == K
    x, y, v = _data(n, case["p"], 32)
    xs = np.linspace(0.0, 3.0, 5)
    q_lo, q_hi = alpha / 2, 1 - alpha / 2
    for sample_y in (True, False):
        out = _rows(eng, x, y, v, burn, keep, leap, seed, xs, sample_y, want_draws=False, row_tails=K)
        _, lo_d, hi_d = eng.row_mean_quantiles(out["row_draws"].reshape(n * 5, keep), q_lo, q_hi)
        lo_t, hi_t = eng.row_tail_quantiles(out["tails"], keep, q_lo, q_hi)
        assert lo_t.shape == hi_t.shape == (5, n) and lo_t.dtype == torch.float32
        assert torch.equal(lo_t.t().reshape(-1), lo_d) and torch.equal(hi_t.t().reshape(-1), hi_d), sample_y
        if K < keep:                                # a larger buffer holds the same order statistics
            more = _rows(eng, x, y, v, burn, keep, leap, seed, xs, sample_y, want_draws=False, row_draws=False, row_tails=K + 1)
            lo_m, hi_m = eng.row_tail_quantiles(more["tails"], keep, q_lo, q_hi)
            assert torch.equal(lo_m, lo_t) and torch.equal(hi_m, hi_t)
        if K > 1:                                   # and one slot less is refused, naming what the bounds read
            with pytest.raises(RuntimeError, match=r"\(-1\).*k_tail must be in \[%d, m = %d\]" % (K, keep)):
                eng.row_tail_quantiles(out["tails"][:, :K - 1].contiguous(), keep, q_lo, q_hi)


# ---------------------------------------------------------------------------------------------------------------------
# 7. partially observed rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, "diag"], ids=["identity", "metric"])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_partial_rows(torch, case, mass):
    seed, burn, K = 99, 40, 4
    _, eng = _setup(case)
    x, y, v = _data(N, case["p"], 32)
    x, y = PR.mixed_panel(x, y, 34)                                       # the three observation patterns inside every tile
    assert np.isnan(y).sum() > np.isnan(x).sum() > 0 and not np.isnan(y).all()
    xs = np.linspace(0.0, 3.0, 5)
    full = _rows(eng, np.nan_to_num(x), np.nan_to_num(y), v, burn, KEEP, LEAP, seed, xs, mass=mass, row_tails=K)
    for sample_y in (True, False):
        rows = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass, partial=True)
        tails = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass, partial=True, row_tails=K)
        _same_run(torch, rows, tails)
        _tails_are_sorted_draws(torch, tails, K, (mass, sample_y))
    assert not torch.equal(tails["state"], full["state"])                 # the pattern did reach the kernel
    cut = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, False, mass=mass, partial=True, row_tails=K, chunk=7)
    assert torch.equal(cut["tails"], tails["tails"])


# ---------------------------------------------------------------------------------------------------------------------
# 8. the class surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", ["identity", "diag"])
def test_predict_individual_and_predict_new(torch, tmp_path, mass):
    m = OC.init_model(0, Z_DIMS, P)
    n, burn, keep, alpha = 96, 40, 20, 0.2
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    xs = np.linspace(0.0, 3.0, 5)
    K = HM.tail_size(alpha, keep)
    assert 1 < K < keep
    kw = dict(alpha=alpha, n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=3, mass=mass)
    groups = np.arange(n) % 3
    x_some = x.ravel().copy()
    x_some[::4] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c, d = (_causal(tmp_path, m) for _ in range(4))
        mean_q, int_q = a.predict_individual(data, xs, interval="quantile", **kw)
        mean_t, int_t = b.predict_individual(data, xs, interval="tails", groups=groups, **kw)                                  # one block
        mean_s, int_s = c.predict_individual(data, xs, interval="tails", draw_budget_bytes=8 * K * len(xs) * 32, **kw)        # 32-row blocks
        mean_n, int_n = d.predict_individual(data, xs, groups=groups, **kw)                                                   # interval='normal'
        assert int_t.shape == (n, 5, 2) and int_t.dtype == np.float64
        assert np.array_equal(int_t, int_q) and np.array_equal(int_s, int_q)                   # the bounds of 'quantile', bit for bit
        assert not np.array_equal(int_t, int_n)
        for model, mean in ((b, mean_t), (c, mean_s)):                                         # mean and sd of 'normal', bit for bit
            assert np.array_equal(mean, mean_n) and np.array_equal(model.individual_sd_, d.individual_sd_)
            assert np.array_equal(model.hmc_row_step_, d.hmc_row_step_) and model._seed_counter == d._seed_counter
            assert (model.hmc_row_mass_ is None) == (mass == "identity")
        assert sorted(b.group_dose_response_) == [0, 1, 2] and c.group_dose_response_ is None
        for g in (0, 1, 2):
            assert all(np.array_equal(p_, q_) for p_, q_ in zip(b.group_dose_response_[g], d.group_dose_response_[g]))
        # new units: the treatment known for three rows in four, the outcome for none
        new = {}
        for name, extra in (("quantile", {}), ("tails", {}), ("blocks", dict(draw_budget_bytes=8 * K * len(xs) * 32)), ("normal", {})):
            model = _causal(tmp_path, m)
            new[name] = model.predict_new(v, x_some, xs, interval="tails" if name == "blocks" else name, **extra, **kw) + (model.individual_sd_,)
        assert np.array_equal(new["tails"][1], new["quantile"][1]) and np.array_equal(new["blocks"][1], new["quantile"][1])
        for name in ("tails", "blocks"):
            assert np.array_equal(new[name][0], new["normal"][0]) and np.array_equal(new[name][2], new["normal"][2])
        assert not np.array_equal(new["tails"][1], int_t)


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(torch, tmp_path):
    case = SHAPES[0]
    m, eng = _setup(case, 51)
    x, y, v = _data(40, 20, 52)
    xs = np.linspace(0.0, 3.0, 5)
    with pytest.raises(ValueError, match="row_tails belongs to row_effects"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_tails=2)
    for bad in (0, 6, 2.5, True):
        with pytest.raises(ValueError, match=r"row_tails must be an integer K with 1 <= K <= n_keep = 5"):
            eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_tails=bad)
    mb = _model(51, [1, 1, 1, 7], 20, True)
    xb, yb, vb = _data(40, 20, 52, True)
    engb = _engine(mb)
    with pytest.raises(ValueError, match="binary treatment"):
        engb.hmc_sample(xb, yb, vb, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_tails=2)
    f = dict(device="cuda", dtype=torch.float32)
    state, grad, logp, step = torch.empty(40, 10, **f), torch.empty(40, 10, **f), torch.empty(40, **f), torch.full((40,), 0.1, **f)
    xv, moments = torch.linspace(0, 3, 5, **f), torch.zeros(3, 5, 40, **f)
    tails = torch.zeros(2, 2, 5, 40, **f)
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (xb.reshape(-1), yb.reshape(-1), vb))
    run = dict(init=True, n_keep=5, x_values=xv, row_moments=moments)
    with pytest.raises(RuntimeError, match=r"\(-1\).*BGM_EFFECT_ITE"):      # the C entry point on a binary handle
        engb.hmc_run_rows_tails(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, row_tails=tails, **run)
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (x.reshape(-1), y.reshape(-1), v))
    with pytest.raises(RuntimeError, match=r"\(-1\).*row_tails_dev"):
        eng.hmc_run_rows_tails(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, **run)
    with pytest.raises(RuntimeError, match=r"\(-1\).*k_tail must be in \[1, n_keep\] = \[1, 5\]; got 6"):
        eng.hmc_run_rows_tails(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, row_tails=torch.zeros(2, 6, 5, 40, **f), **run)
    with pytest.raises(RuntimeError, match=r"\(-1\).*row_moments"):
        eng.hmc_run_rows_tails(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, init=True, n_keep=5, x_values=xv, row_tails=tails)
    with pytest.raises(RuntimeError, match=r"\(-1\).*beyond burn_in \+ n_keep"):
        eng.hmc_run_rows_tails(xt, yt, vt, state, logp, grad, step, 0, 11, 5, 2, 7, row_tails=tails, **run)
    with pytest.raises(ValueError, match=r"row_tails must be \[2, K, n_doses, n\] = \[2, K, 5, 40\]"):
        eng.hmc_run_rows_tails(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, row_tails=torch.zeros(2, 2, 5, 39, **f), **run)
    assert not bool(moments.any()) and not bool(tails.any())
    with pytest.raises(RuntimeError, match=r"\(-1\).*k_tail must be in \[3, m = 21\].*the 3 smallest and the 2 largest"):
        eng.row_tail_quantiles(torch.zeros(2, 2, 5, 40, **f), 21, 0.05, 0.95)
    with pytest.raises(RuntimeError, match=r"\(-1\).*k_tail must be in \[2, m = 5\]"):
        eng.row_tail_quantiles(torch.zeros(2, 6, 5, 40, **f), 5, 0.05, 0.95)                   # more slots than values
    out = eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_tails=5)   # the handle stays usable
    assert out["tails"].shape == (2, 5, 5, 40) and "row_draws" not in out
    # the LDS budget of the fused kernels, named in bytes: seven layers of 64 at KT1 = 1
    deep = _model(71, [1, 1, 1, 7], 20, g_units=(64,) * 7)
    with pytest.raises(RuntimeError, match=r"\(-4\).*178320 B.*draws route"):
        _engine(deep, g_units=[64] * 7).hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_tails=2)
    # the class: a binary treatment has no tails route
    mbin = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = _causal(tmp_path, mbin, binary=True)
        with pytest.raises(ValueError, match="interval='tails'.*ITE route"):
            model.predict_new(_data(8, P, 8, True)[2], interval="tails", n_mcmc=5, burn_in=5, verbose=0)
        with pytest.raises(ValueError, match="predict's ITE"):
            model.predict_individual(_data(8, P, 8, True), xs, interval="tails", n_mcmc=5, burn_in=5, verbose=0)
