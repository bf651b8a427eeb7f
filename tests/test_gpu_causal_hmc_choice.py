"""The choice among the doses, compared per retained draw inside the CausalBGM HMC sampler (csrc/causal_hmc_choice_kernels.h,
bgm_causal_hmc_run_row_choice; hmc_sample(row_effects=True, row_choice=True), CausalBGM.predict_best_dose).

Bars:
  chain, curve, draws, cuts, windows, trips, partial rows, class     bit-identity (torch.equal / np.array_equal)
  best_count, above_count            exactly the counts of tests/_causal_hmc_choice_ref.py on the run's own row_draws, at every dose
                                     count where the pass structure of the kernel changes, maximising and minimising
  best_ref, best_s1                  bit for bit the float32 sequential sums of the per-draw best of the run's own row_draws
  best_mean                          beyond the largest row_mean by no more than the two float32 summation bounds (the mean of a
                                     maximum is at least the maximum of the means on the same values)
  float64 anchor                     the best dose of every (row, draw) against the argmax of the float64 oracle on the returned latent
                                     draws; pairs whose float64 top-two gap is below 4e-4 -- twice the 2e-4
                                     tests/test_gpu_causal_hmc_rowfx.py grants one value -- are left out, at most 10 % of them
The models are the small ones of tests/test_gpu_causal_hmc_contrast.py, both first-layer tilings."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_choice_ref as CH  # noqa: E402
import _causal_partial_ref as PR  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402
from tests.test_gpu_causal_hmc_fused import P, Z_DIMS, _causal  # noqa: E402
from tests.test_gpu_causal_hmc_rowfx import _oracle_rows  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
BURN, KEEP, LEAP, STEP0 = 30, 20, 3, 0.1
SHAPES = [dict(z_dims=[1, 1, 1, 7], p=20), dict(z_dims=[3, 3, 6, 6], p=20)]      # both first-layer tilings (KT1 = 1, 2)
KEYS = ("draws", "state", "logp", "grad", "row_step", "acc_count")
CHOICE = ("row_mean", "row_sd", "row_draws", "best_count", "best_ref", "best_s1", "best_mean")
N = 200                                                                             # 13 tiles, the last one of 8 rows
# 1: one dose, three lane groups hold padding only; 3: a ragged shared pass; 5: two shared passes; 16: four passes of the lane
# groups' own doses, k = 4 g + p; 18: those and one shared pass; 33: a second block of own passes and a shared pass of one dose
DOSES = (1, 3, 5, 16, 18, 33)
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
    return np.linspace(0.5, 3.0, n_doses)


def _rows(eng, x, y, v, burn, keep, leap, seed, xs, sample_y=True, want_draws=True, row_draws=True, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, want_draws=want_draws, adapt=TARGET, row_effects=True, row_draws=row_draws,
                          x_values=xs, sample_y=sample_y, **kw)


def _cho(eng, *args, **kw):
    return _rows(eng, *args, row_choice=True, **kw)


def _same_choice(torch, a, b, rows=slice(None), keys=CHOICE):
    for k in keys + (("above_count",) if "above_count" in a else ()):
        assert torch.equal(a[k][rows], b[k]), k


def _counts_are_those_of_the_draws(torch, out, maximize, threshold=None, what=None):
    """best_count / best_ref / best_s1 / above_count of a run against the restatement on the run's own row_draws"""
    y = out["row_draws"].cpu().numpy()
    n, n_doses, keep = y.shape
    got = out["best_count"].cpu().numpy()
    assert got.shape == (n, n_doses) and got.dtype == np.int64
    want = CH.best_count(y, maximize)
    bad = (got != want).any(axis=0)
    assert not bad.any(), (what, "doses whose counts differ: %r" % (np.flatnonzero(bad).tolist(),))
    assert (got.sum(axis=1) == keep).all(), what
    ref, s1 = CH.best_moments(y, maximize)
    assert np.array_equal(out["best_ref"].cpu().numpy(), ref) and np.array_equal(out["best_s1"].cpu().numpy(), s1), what
    if threshold is not None:
        assert np.array_equal(out["above_count"].cpu().numpy(), CH.above_count(y, threshold)), what
    else:
        assert "above_count" not in out
    return y, got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the chain, the curve and the draws are unchanged
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
        cho = _cho(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass)
        for k in KEYS + ("row_mean", "row_sd", "row_draws") + (("mass_scale",) if mass else ()):
            assert torch.equal(rows[k], cho[k]), (k, sample_y)
        assert ("mass_scale" in cho) == (mass is not None)
        assert "best_count" not in rows and "best_mean" not in rows and "above_count" not in cho
        assert cho["best_count"].shape == (N, 18) and cho["best_count"].dtype == torch.int64
        assert cho["best_mean"].shape == (N,) and cho["best_mean"].dtype == torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# 2. the counts are those of the run's own draws
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_doses", DOSES)
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_counts_are_those_of_the_runs_own_draws(torch, case, n_doses):
    seed = 4711 + n_doses
    _, eng = _setup(case)
    x, y, v = _data(N, case["p"], 32)
    xs = _doses(n_doses)
    for sample_y in (True, False):
        rows = _rows(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, want_draws=False)
        thr = float(np.median(rows["row_draws"].cpu().numpy()))
        winners = set()
        for maximize in (True, False):
            out = _cho(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, want_draws=False, maximize=maximize, threshold=thr)
            assert torch.equal(out["row_draws"], rows["row_draws"]) and torch.equal(out["row_mean"], rows["row_mean"])
            draws, got = _counts_are_those_of_the_draws(torch, out, maximize, thr, (sample_y, maximize))
            assert np.isfinite(draws).all()
            winners |= set(np.flatnonzero(got.sum(axis=0)).tolist())
            above = out["above_count"].cpu().numpy()
            assert 0 < above.sum() < above.size * KEEP                     # the median: both sides of the threshold occur
            if n_doses == 1:
                assert (got == KEEP).all()
        if n_doses > 1:                                                      # the largest and the smallest are not the same dose
            assert len(winners) > 1, sorted(winners)
    for bad in (float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="threshold must be None or a finite scalar"):
            _cho(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, threshold=bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. ties: the lowest dose index wins, whichever lane group and pass holds it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_ties_go_to_the_lowest_dose_index(torch, case):
    """18 doses: own passes 0 .. 3 hold dose k in lane group (k >> 2) & 3 at pass k & 3, the shared pass 4 holds dose 16 + g in lane
    group g.  The largest dose stands at 5 (group 1, pass 1), 10 (group 2, pass 2), 13 (group 3, pass 1) and 16 (group 0, shared):
    the lane group that writes the counts holds the HIGHEST copy itself and must give way to group 1's.  The smallest stands at 9
    (group 2, pass 1), 14 (group 3, pass 2) and 17 (group 1, shared): lane group 0 holds no copy, meets 17 in the first exchange
    step and must give it up for 9 in the second.  A rule that keeps what it saw first gets both wrong.  Without noise equal doses
    run the same instructions on the same operands: bit-equal values, so every draw an extreme dose wins is a tie."""
    hi, lo = (5, 10, 13, 16), (9, 14, 17)
    xs = np.linspace(0.7, 2.8, 18)
    xs[list(hi)], xs[list(lo)] = 3.0, 0.5
    _, eng = _setup(case)
    x, y, v = _data(N, case["p"], 32)
    tied, won = 0, np.zeros(2, np.int64)
    for maximize in (True, False):
        out = _cho(eng, x, y, v, BURN, KEEP, LEAP, 4729, xs, False, want_draws=False, maximize=maximize)
        draws, got = _counts_are_those_of_the_draws(torch, out, maximize, None, maximize)
        for same in (hi, lo):
            assert all(np.array_equal(draws[:, same[0]], draws[:, k]) for k in same[1:])      # bit-equal values
            assert not got[:, list(same[1:])].any()                        # a later copy never wins
        best = draws.max(axis=1) if maximize else draws.min(axis=1)
        ties = ((draws == best[:, None]).sum(axis=1) > 1)                  # [n, keep]: the best value stands at more than one index
        tied += int(ties.sum())
        won += (got[:, hi[0]].sum(), got[:, lo[0]].sum())                  # every draw an extreme dose won is such a tie
        assert int(ties.sum()) >= int(got[:, hi[0]].sum() + got[:, lo[0]].sum())
    print("ties at the best value q%d: %d of %d (row, draw) pairs; won by the largest dose %d, by the smallest %d" %
          (sum(case["z_dims"]), tied, 2 * N * KEEP, won[0], won[1]))
    assert tied > 0 and (won > 0).all()                                    # both arrangements were put to the test


# ---------------------------------------------------------------------------------------------------------------------
# 4. the best value
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [20, 400])
def test_best_moments_are_the_float32_sequential_sums(torch, keep):
    for case in SHAPES:
        _, eng = _setup(case, 51)
        x, y, v = _data(N, case["p"], 52)
        for sample_y in (True, False):
            for maximize in (True, False):
                out = _cho(eng, x, y, v, BURN, keep, LEAP, 5, _doses(18 if keep == 20 else 5), sample_y, want_draws=False, maximize=maximize)
                draws, _ = _counts_are_those_of_the_draws(torch, out, maximize, None, (case, sample_y, maximize))      # ref, s1: bit for bit
                ref, s1 = out["best_ref"].double(), out["best_s1"].double()
                assert torch.equal(out["best_mean"], ref + s1 / keep)
                best_mean, row_mean = out["best_mean"].cpu().numpy(), out["row_mean"].cpu().numpy()
                bound = CH.best_mean_bound(draws, maximize) + CH.shifted_mean_bound(draws).max(axis=1)
                slack = (best_mean - row_mean.max(axis=1)) if maximize else (row_mean.min(axis=1) - best_mean)      # the least regret
                print("best value q%d sample_y=%d maximize=%d m=%d: least regret %.3g, its bound -%.3g, largest regret %.3g" %
                      (sum(case["z_dims"]), sample_y, maximize, keep, slack.min(), bound.max(), slack.max()))
                assert (slack >= -bound).all()
                exact = CH.best_value(draws, maximize).astype(np.float64).mean(axis=1)
                assert (np.abs(best_mean - exact) <= CH.best_mean_bound(draws, maximize)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the float64 anchor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_best_dose_matches_the_float64_oracle(torch, case):
    seed, gap = 5, 4e-4
    m, eng = _setup(case, 51)
    x, y, v = _data(N, case["p"], 52)
    xs = np.linspace(0.5, 3.0, 5)
    out = _cho(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, False)
    ref = _oracle_rows(m, out["draws"].cpu().numpy(), xs, False, seed, BURN)       # [n, 5, keep] float64
    got = CH.best_index(out["row_draws"].cpu().numpy(), True)                     # [n, keep]
    top = np.sort(ref, axis=1)
    close = (top[:, -1] - top[:, -2]) < gap
    share = close.mean()
    interior = np.isin(np.argmax(ref, axis=1), (1, 2, 3)).mean()
    print("best dose q%d against the float64 oracle: %.2f %% of the (row, draw) pairs left out (top-two gap below %.0e; cap 10 %%), an "
          "interior dose wins %.1f %% of the pairs" % (sum(case["z_dims"]), 100 * share, gap, 100 * interior))
    assert share <= 0.10
    assert np.array_equal(got[~close], np.argmax(ref, axis=1)[~close])
    # and the counts are those of that index
    count = out["best_count"].cpu().numpy()
    assert all(np.array_equal(count[:, k], (got == k).sum(axis=1)) for k in range(5))


# ---------------------------------------------------------------------------------------------------------------------
# 6. launch cuts, row windows, trips of the tile loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_launch_cuts_and_row_windows_change_nothing(torch, case):
    seed = 4711
    _, eng = _setup(case, 41)
    x, y, v = _data(N, case["p"], 42)
    xs = _doses(18)
    for sample_y in (True, False):
        thr = 0.25
        one = _cho(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, threshold=thr, maximize=sample_y)
        _counts_are_those_of_the_draws(torch, one, sample_y, thr, sample_y)
        for chunk in (4, 1):                        # 4: launches end at 28 | 32 across burn_in = 30; 1: one iteration a launch
            cut = _cho(eng, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y, threshold=thr, maximize=sample_y, chunk=chunk)
            for k in KEYS:
                assert torch.equal(one[k], cut[k]), (k, chunk)
            _same_choice(torch, one, cut)
    a, e = 23, 171                                                        # rows [a, e) alone with their global row index
    part = _cho(eng, x[a:e], y[a:e], v[a:e], BURN, KEEP, LEAP, seed, xs, False, row_base=a, threshold=thr, maximize=False)
    _same_choice(torch, one, part, slice(a, e))
    assert torch.equal(part["draws"], one["draws"][:, a:e])


def test_rows_beyond_one_trip_of_the_tile_loop(torch):
    """16 x 8 x CUs x 2 + 37 rows: every wave slot walks two or three tiles, the last tile is ragged"""
    case = SHAPES[0]
    burn, keep, leap, seed, thr = 3, 5, 2, 4242, 0.25
    _, eng = _setup(case, 65)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus * 2 + 37
    assert eng.mh_slots(n) == waves * n_cus and (n + 15) // 16 == 2 * waves * n_cus + 3
    x, y, v = _data(n, case["p"], 66)
    xs = _doses(5)
    rows = _rows(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False)
    out = _cho(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False, threshold=thr)
    assert torch.equal(out["row_draws"], rows["row_draws"]) and torch.equal(out["row_mean"], rows["row_mean"])
    _counts_are_those_of_the_draws(torch, out, True, thr, "three trips")
    chunked = _cho(eng, x, y, v, burn, keep, leap, seed, xs, want_draws=False, threshold=thr, chunk=2)
    _same_choice(torch, out, chunked)
    for a, e in ((0, 16), (16 * waves * n_cus - 5, 16 * waves * n_cus + 21), (n - 40, n)):      # the first tile; across the first two trips; the ragged end
        part = _cho(eng, x[a:e], y[a:e], v[a:e], burn, keep, leap, seed, xs, want_draws=False, row_base=a, threshold=thr)
        _same_choice(torch, out, part, slice(a, e))


# ---------------------------------------------------------------------------------------------------------------------
# 7. guard bands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_doses", [5, 18])
def test_nothing_is_written_outside_the_buffers(torch, n_doses):
    """A ragged panel (n = 17: fifteen padding lanes in the second tile) and a padded dose pass write nothing: every buffer of the
    call lies between two guard bands.  The launches of the burn-in write nothing at all, the first retained iteration writes
    every element (zeros included), and a run cut at every iteration leaves every plane bit-identical to one launch."""
    case = SHAPES[0]
    _, eng = _setup(case)
    n, burn, keep, leap, guard, mark, thr = 17, 4, 6, 2, 4096, -12345, 0.25
    x, y, v = (torch.from_numpy(a).cuda() for a in _data(n, case["p"], 32))
    x, y = x.reshape(-1), y.reshape(-1)
    f = dict(device="cuda", dtype=torch.float32)
    q = sum(case["z_dims"])
    xv = torch.from_numpy(_doses(n_doses).astype(np.float32)).cuda()
    shapes = dict(row_moments=((3, n_doses, n), torch.float32), row_draws=((n, n_doses, keep), torch.float32),
                  best_count=((n_doses, n), torch.int32), best_moments=((2, n), torch.float32), above_count=((n_doses, n), torch.int32))

    def run(cuts):
        flats = {k: torch.full((2 * guard + int(np.prod(s)),), mark, device="cuda", dtype=dt) for k, (s, dt) in shapes.items()}
        bufs = {k: flats[k][guard:-guard].view(*s) for k, (s, _) in shapes.items()}
        state, grad, logp, step = torch.empty(n, q, **f), torch.empty(n, q, **f), torch.empty(n, **f), torch.full((n,), 0.1, **f)
        kw = dict(n_keep=keep, x_values=xv, threshold=thr, maximize=True, **bufs)
        eng.hmc_run_rows_choice(x, y, v, state, logp, grad, step, 0, burn, burn, leap, 7, init=True, **kw)
        torch.cuda.synchronize()
        assert all(bool((fl == mark).all()) for fl in flats.values())      # burn-in: nothing is sampled into any buffer
        eng.hmc_run_rows_choice(x, y, v, state, logp, grad, step, burn, 1, burn, leap, 7, **kw)      # the first retained iteration
        torch.cuda.synchronize()
        for k in ("row_moments", "best_count", "best_moments", "above_count"):
            assert bool((bufs[k] != mark).all()), k                         # every element inside is written by it, zeros included
        assert bool((bufs["best_count"].sum(dim=0) == 1).all()) and not bool(bufs["best_moments"][1].any())
        for a, e in zip(cuts[:-1], cuts[1:]):
            eng.hmc_run_rows_choice(x, y, v, state, logp, grad, step, a, e - a, burn, leap, 7, **kw)
        torch.cuda.synchronize()
        for k, fl in flats.items():
            assert bool((fl[:guard] == mark).all()) and bool((fl[-guard:] == mark).all()), k
            assert bool((bufs[k] != mark).all()), k
        return bufs, state
    one, state_one = run([burn + 1, burn + keep])
    each, state_each = run(list(range(burn + 1, burn + keep + 1)))
    assert torch.equal(state_one, state_each)
    for k in shapes:
        assert torch.equal(one[k], each[k]), k
    # the same run through hmc_sample's own buffers, and the curve planes of the entry point without the choice
    xs = xv.cpu().numpy()
    ref = eng.hmc_sample(x, y, v, burn, keep, 0.1, leap, 7, adapt=None, row_effects=True, row_draws=True, x_values=xs, row_choice=True, threshold=thr)
    assert torch.equal(ref["row_draws"], one["row_draws"]) and torch.equal(ref["best_count"], one["best_count"].t().long())
    assert torch.equal(ref["above_count"], one["above_count"].t().long())
    assert torch.equal(ref["best_ref"], one["best_moments"][0]) and torch.equal(ref["best_s1"], one["best_moments"][1])
    _counts_are_those_of_the_draws(torch, ref, True, thr)
    state, grad, logp, step = torch.empty(n, q, **f), torch.empty(n, q, **f), torch.empty(n, **f), torch.full((n,), 0.1, **f)
    moments = torch.zeros(3, n_doses, n, **f)
    eng.hmc_run_rows_effects(x, y, v, state, logp, grad, step, 0, burn + keep, burn, leap, 7, init=True, n_keep=keep, x_values=xv, row_moments=moments)
    assert torch.equal(moments, one["row_moments"]) and torch.equal(state, state_one)


# ---------------------------------------------------------------------------------------------------------------------
# 8. partially observed rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, "diag"], ids=["identity", "metric"])
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_partial_rows(torch, case, mass):
    seed, burn, thr = 99, 40, 0.25
    _, eng = _setup(case)
    x0, y0, v = _data(N, case["p"], 32)
    x, y = PR.mixed_panel(x0, y0, 34)                                     # the three observation patterns inside every tile
    assert np.isnan(y).sum() > np.isnan(x).sum() > 0 and not np.isnan(y).all()
    xs = _doses(5)
    if mass and sum(case["z_dims"]) + 1 > 12:
        # The one instantiation that is not shipped: the metric with the observation pattern at KT1 = 2 needs
        # scratch memory.  hmc_sample refuses the combination before a device is touched, the library naming itself before anything
        # is launched; the handle stays usable, and the fully observed kernel with the metric exists.
        with pytest.raises(ValueError, match=r"more than 11 latent features \(here 18\).*not built"):
            _cho(eng, x, y, v, burn, KEEP, LEAP, seed, xs, True, mass=mass, partial=True)
        q = sum(case["z_dims"])
        f, i32 = dict(device="cuda", dtype=torch.float32), dict(device="cuda", dtype=torch.int32)
        xt, yt, vt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x.reshape(-1), y.reshape(-1), v))
        state, grad, logp, step = torch.empty(N, q, **f), torch.empty(N, q, **f), torch.empty(N, **f), torch.full((N,), 0.1, **f)
        bufs = dict(row_moments=torch.zeros(3, 5, N, **f), best_count=torch.zeros(5, N, **i32), best_moments=torch.zeros(2, N, **f))
        eng.set_hmc_mass(torch.ones(N, q, **f))
        try:
            with pytest.raises(RuntimeError, match=r"bgm_causal_hmc_run_row_choice failed \(-4\).*partially observed rows, with a diagonal "
                                                   r"metric, at more than 11 latent features \(KT1 = 2\).*without the metric"):
                eng.hmc_run_rows_choice(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, init=True, n_keep=5,
                                        x_values=torch.from_numpy(xs.astype(np.float32)).cuda(), partial=True, **bufs)
        finally:
            eng.set_hmc_mass(None)
        assert not any(bool(b.any()) for b in bufs.values())              # nothing was launched
        full = _cho(eng, x0, y0, v, burn, KEEP, LEAP, seed, xs, False, mass=mass, threshold=thr)
        _counts_are_those_of_the_draws(torch, full, True, thr, "metric, fully observed")
        return
    for sample_y in (True, False):
        rows = _rows(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass, partial=True)
        cho = _cho(eng, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, mass=mass, partial=True, threshold=thr, maximize=not sample_y)
        for k in KEYS + ("row_mean", "row_sd", "row_draws") + (("mass_scale",) if mass else ()):
            assert torch.equal(rows[k], cho[k]), (k, sample_y)
        _counts_are_those_of_the_draws(torch, cho, not sample_y, thr, (mass, sample_y))
    # a fully observed panel under partial=True is the run of partial=False
    full = _cho(eng, x0, y0, v, burn, KEEP, LEAP, seed, xs, False, mass=mass, threshold=thr)
    same = _cho(eng, x0, y0, v, burn, KEEP, LEAP, seed, xs, False, mass=mass, threshold=thr, partial=True)
    for k in KEYS:
        assert torch.equal(full[k], same[k]), k
    _same_choice(torch, full, same)
    assert not torch.equal(full["state"], cho["state"])                   # the pattern did reach the kernel


# ---------------------------------------------------------------------------------------------------------------------
# 9. the class surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", ["identity", "diag"])
def test_predict_best_dose(torch, tmp_path, mass):
    m = OC.init_model(0, Z_DIMS, P)
    n, burn, keep, thr = 96, 40, 20, 0.1
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    xs = np.linspace(0.5, 3.0, 5)
    kw = dict(n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=3, mass=mass)
    groups = np.arange(n) % 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ind, a, b, c = (_causal(tmp_path, m) for _ in range(4))
        curve_mean, _ = ind.predict_individual(data, xs, sample_y=False, **kw)
        choice, prob = a.predict_best_dose(data, xs, threshold=thr, groups=groups, **kw)
        choice_min, prob_min = b.predict_best_dose(data, xs, maximize=False, **kw)
        _, prob_noise = c.predict_best_dose(data, xs, sample_y=True, **kw)
    assert choice.shape == (n,) and prob.shape == (n, 5) and prob.dtype == np.float64 and np.issubdtype(choice.dtype, np.integer)
    for model in (a, b):                # the curve is predict_individual's, bit for bit
        assert np.array_equal(model.dose_choice_curve_[0], curve_mean) and np.array_equal(model.dose_choice_curve_[1], ind.individual_sd_)
        assert np.array_equal(model.hmc_row_step_, ind.hmc_row_step_) and model._seed_counter == ind._seed_counter
        assert (model.hmc_row_mass_ is None) == (mass == "identity") and model.individual_sd_ is None
    for p_ in (prob, prob_min, prob_noise):
        assert np.array_equal(np.rint(p_ * keep), p_ * keep) and (np.rint(p_ * keep).sum(axis=1) == keep).all()      # whole counts: rows sum to 1
        assert np.abs(p_.sum(axis=1) - 1.0).max() <= 1e-15
    assert np.array_equal(choice, np.argmax(curve_mean, axis=1)) and np.array_equal(choice_min, np.argmin(curve_mean, axis=1))
    assert not np.array_equal(prob, prob_min) and not np.array_equal(prob, prob_noise)
    # the regret: choice_finalize on the counts, not below minus the float32 rounding, smallest at the choice
    for model, p_, mx in ((a, prob, True), (b, prob_min, False)):
        reg = model.dose_regret_
        expected = reg[:, 0] + curve_mean[:, 0] if mx else curve_mean[:, 0] - reg[:, 0]
        want = HM.choice_finalize(p_ * keep, expected, np.zeros(n), curve_mean, keep, mx)
        assert reg.shape == (n, 5) and np.allclose(reg, want[2], rtol=0, atol=1e-12) and np.array_equal(want[0], p_)
        # no value of a series lies further from its mean than sqrt(m - 1) sd, so R <= 2 sqrt(m - 1) sd in the summation bound of
        # tests/_causal_hmc_choice_ref.py (shifted_mean_bound), once for E[best] and once for the mean
        bound = 2 * ((keep - 1) + (keep - 1) ** 2) / keep * 2.0 ** -24 * 2 * np.sqrt(keep - 1) * ind.individual_sd_.max()
        assert reg.min() >= -bound and reg.max() > 0
        ch = choice if mx else choice_min
        assert (reg[np.arange(n), ch] <= reg.min(axis=1) + 1e-12).all()
    exceed = a.dose_exceed_prob_
    assert exceed.shape == (n, 5) and exceed.min() >= 0 and exceed.max() <= 1 and 0 < exceed.mean() < 1
    assert np.array_equal(np.rint(exceed * keep), exceed * keep) and b.dose_exceed_prob_ is None
    want = HM.group_dose_choice(choice, prob, groups)
    assert sorted(a.group_dose_choice_) == [0, 1, 2] and b.group_dose_choice_ is None
    for g in (0, 1, 2):
        assert all(np.array_equal(p_, q_) for p_, q_ in zip(a.group_dose_choice_[g], want[g]))
        assert abs(a.group_dose_choice_[g][0].sum() - 1.0) <= 1e-15
    # new units: the outcome of no row observed, the treatment of three rows in four
    x_some, y_none = x.copy(), np.full_like(y, np.nan)
    x_some[::4] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        new, e = _causal(tmp_path, m), _causal(tmp_path, m)
        new_curve, _ = new.predict_new(v, x_some.ravel(), xs, sample_y=False, **kw)
        choice_p, prob_p = e.predict_best_dose((x_some, y_none, v), xs, partial=True, **kw)
    assert np.array_equal(e.dose_choice_curve_[0], new_curve) and not np.array_equal(prob_p, prob) and prob_p.shape == (n, 5)
    assert np.array_equal(choice_p, np.argmax(new_curve, axis=1))


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(torch, tmp_path):
    case = SHAPES[0]
    _, eng = _setup(case, 51)
    x, y, v = _data(40, 20, 52)
    xs = _doses(5)
    f = dict(device="cuda", dtype=torch.float32)
    i32 = dict(device="cuda", dtype=torch.int32)
    state, grad, logp, step = torch.empty(40, 10, **f), torch.empty(40, 10, **f), torch.empty(40, **f), torch.full((40,), 0.1, **f)
    xv, moments = torch.linspace(0, 3, 5, **f), torch.zeros(3, 5, 40, **f)
    best, bmom, above = torch.zeros(5, 40, **i32), torch.zeros(2, 40, **f), torch.zeros(5, 40, **i32)
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (x.reshape(-1), y.reshape(-1), v))
    run = dict(init=True, n_keep=5, x_values=xv, row_moments=moments)
    call = (xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7)
    # a trajectory option set on the handle: BGM_E_UNSUPPORTED naming it, before anything else is looked at
    for setting, word in (((1.0, False, None), "max_trajectory"), ((None, True, None), "jitter"),
                          ((None, False, torch.zeros(40, **i32)), "n_steps_dev")):
        eng.set_hmc_trajectory(*setting)
        try:
            with pytest.raises(RuntimeError, match=r"bgm_causal_hmc_run_row_choice failed \(-4\).*dose-choice kernels.*%s is set" % word):
                eng.hmc_run_rows_choice(*call, **run)
        finally:
            eng.set_hmc_trajectory(None)
    with pytest.raises(RuntimeError, match=r"\(-1\).*best_count_dev required"):
        eng.hmc_run_rows_choice(*call, best_moments=bmom, **run)
    with pytest.raises(RuntimeError, match=r"\(-1\).*best_moments_dev required"):
        eng.hmc_run_rows_choice(*call, best_count=best, **run)
    with pytest.raises(RuntimeError, match=r"\(-1\).*row_moments"):
        eng.hmc_run_rows_choice(*call, init=True, n_keep=5, x_values=xv, best_count=best, best_moments=bmom)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match=r"\(-1\).*threshold must be finite"):
            eng.hmc_run_rows_choice(*call, best_count=best, best_moments=bmom, above_count=above, threshold=bad, **run)
    with pytest.raises(RuntimeError, match=r"\(-1\).*beyond burn_in \+ n_keep"):
        eng.hmc_run_rows_choice(xt, yt, vt, state, logp, grad, step, 0, 11, 5, 2, 7, best_count=best, best_moments=bmom, **run)
    with pytest.raises(ValueError, match=r"best_count must be a contiguous int32 tensor \(5, 40\)"):
        eng.hmc_run_rows_choice(*call, best_count=torch.zeros(5, 39, **i32), best_moments=bmom, **run)
    with pytest.raises(ValueError, match=r"above_count must be a contiguous int32 tensor \(5, 40\)"):
        eng.hmc_run_rows_choice(*call, best_count=best, best_moments=bmom, above_count=torch.zeros(5, 40, **f), **run)
    mb = _model(51, [1, 1, 1, 7], 20, True)
    xb, yb, vb = _data(40, 20, 52, True)
    engb = _engine(mb)
    xbt, ybt, vbt = (torch.from_numpy(a).cuda() for a in (xb.reshape(-1), yb.reshape(-1), vb))
    with pytest.raises(RuntimeError, match=r"\(-1\).*BGM_EFFECT_ITE"):      # the C entry point on a binary handle
        engb.hmc_run_rows_choice(xbt, ybt, vbt, state, logp, grad, step, 0, 10, 5, 2, 7, best_count=best, best_moments=bmom, **run)
    assert not bool(moments.any()) and not bool(best.any()) and not bool(bmom.any()) and not bool(above.any())
    # the engine's own refusals
    with pytest.raises(ValueError, match="binary treatment"):
        engb.hmc_sample(xb, yb, vb, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_choice=True)
    with pytest.raises(ValueError, match="row_choice belongs to row_effects"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_choice=True)
    for kw in (dict(jitter=True), dict(max_trajectory=0.5)):
        with pytest.raises(ValueError, match="not available with row_choice"):
            eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_choice=True, **kw)
    for kw in (dict(row_contrasts=True), dict(row_tails=2)):
        with pytest.raises(ValueError, match="row_choice is not available with row_contrasts or row_tails"):
            eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_choice=True, **kw)
    out = eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_choice=True)      # the handle stays usable
    assert out["best_count"].shape == (40, 5) and "row_draws" not in out and bool((out["best_count"].sum(dim=1) == 5).all())
    # the LDS budget of the fused kernels, named in bytes: seven layers of 64 at KT1 = 1
    deep = _model(71, [1, 1, 1, 7], 20, g_units=(64,) * 7)
    with pytest.raises(RuntimeError, match=r"\(-4\).*178320 B.*draws route"):
        _engine(deep, g_units=[64] * 7).hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, row_effects=True, x_values=xs, row_choice=True)
    # the class: a binary treatment has the ITE
    mbin = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = _causal(tmp_path, mbin, binary=True)
        with pytest.raises(ValueError, match="predict's ITE"):
            model.predict_best_dose(_data(8, P, 8, True), xs, n_mcmc=5, burn_in=5, verbose=0)
