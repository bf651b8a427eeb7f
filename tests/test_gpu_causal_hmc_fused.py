"""The CausalBGM HMC sampler with the effect pass inside the kernel (csrc/causal_hmc_fx_kernels.h, bgm_causal_hmc_run_effects;
hmc_sample(effect=...), predict(sampler='hmc', fused_effects=True)) against the two-pass route it replaces: hmc_sample with its draws
kept, then engine.effects on them.

Bars: everything is bit-identity -- the chain of a fused run is the chain of the run without effects, and its ADRF / ITE are
engine.effects on that chain's draws (same routine, same LDS bytes, same additions in the same order) -- except
  several blocks   predict cut into 48-row blocks against the fused single block: n * 2**-24 * Y with Y the largest |outcome draw| of
                   the float64 oracle's outcome net on the draws: the float32 sums over rows are reassociated, nothing else differs
  oracle           fused ADRF / ITE with sample_y=False against oracle.causal.infer_from_latent_posterior (float64) on the returned
                   draws: 2e-4 absolute, the bar tests/test_gpu_causal.py applies to engine.effects."""
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

from bayesgm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
BURN, KEEP, LEAP, STEP0 = 30, 20, 3, 0.1
SHAPES = [dict(z_dims=[1, 1, 1, 7], p=20), dict(z_dims=[3, 3, 6, 6], p=20)]      # both first-layer tilings (KT1 = 1, 2)
CASES = [dict(s, binary=b) for s in SHAPES for b in (False, True)]
KEYS = ("draws", "state", "logp", "grad", "row_step", "acc_count")
N = 200                                                                             # 13 tiles, the last one of 8 rows


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _id(case):
    return "q%d-%s" % (sum(case["z_dims"]), "binary" if case["binary"] else "continuous")


def _fused(eng, binary, x, y, v, burn, keep, leap, seed, xs=None, sample_y=True, want_draws=True, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, want_draws=want_draws, adapt=TARGET,
                          effect=_lib.EFFECT_ITE if binary else _lib.EFFECT_ADRF, x_values=None if binary else xs, sample_y=sample_y, **kw)


def _same_chain(torch, plain, fused):
    for k in KEYS + (("mass_scale",) if "mass_scale" in plain else ()):
        assert torch.equal(plain[k], fused[k]), k


def _same_effects(torch, eng, binary, x, plain, fused, burn, seed, xs, sample_y, row_base=0):
    """the fused run's effects are engine.effects on the draws of the run without effects"""
    ref = eng.effects(x, plain["draws"], burn, seed, x_values=None if binary else xs, sample_y=sample_y, row_base=row_base)
    keep, n = plain["draws"].shape[:2]
    if binary:
        assert fused["ite"].shape == (n, keep) and torch.equal(fused["ite"], ref.t()), "ite"
    else:
        assert fused["adrf"].shape == (len(xs), keep) and torch.equal(fused["adrf"], ref), ("adrf", len(xs), sample_y)
    assert bool(torch.isfinite(ref).all())


# ---------------------------------------------------------------------------------------------------------------------
# 1. + 2. the chain is unchanged and the effects are those of the draws
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_chain_unchanged_and_effects_exact(torch, case):
    seed, binary = 99, case["binary"]
    m = _model(31, case["z_dims"], case["p"], binary)
    x, y, v = _data(N, case["p"], 32, binary)
    eng = _engine(m)
    plain = eng.hmc_sample(x, y, v, BURN, KEEP, STEP0, LEAP, seed, want_draws=True, adapt=TARGET)
    assert "adrf" not in plain and "ite" not in plain
    assert bool(torch.isfinite(plain["draws"]).all()) and 0 < int(plain["acc_count"].sum()) < (BURN + KEEP) * N
    for n_doses in ((2,) if binary else (1, 5, 17, 20)):      # 17, 20: lane groups with a Philox call of their own, and the shared remainder
        xs = np.linspace(0.0, 3.0, n_doses)
        for sample_y in (True, False):
            fused = _fused(eng, binary, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y)
            _same_chain(torch, plain, fused)
            _same_effects(torch, eng, binary, x, plain, fused, BURN, seed, xs, sample_y)
    # rows [a, e) alone with their global row index: the RNG streams of the chain and of the outcome noise follow row_base
    a, e = 23, 171
    xs = np.linspace(0.0, 3.0, 5)
    part_plain = eng.hmc_sample(x[a:e], y[a:e], v[a:e], BURN, KEEP, STEP0, LEAP, seed, want_draws=True, adapt=TARGET, row_base=a)
    part = _fused(eng, binary, x[a:e], y[a:e], v[a:e], BURN, KEEP, LEAP, seed, xs, True, row_base=a)
    _same_chain(torch, part_plain, part)
    _same_effects(torch, eng, binary, x[a:e], part_plain, part, BURN, seed, xs, True, row_base=a)
    assert torch.equal(part["draws"], plain["draws"][:, a:e])
    if binary:
        assert torch.equal(part["ite"], _fused(eng, binary, x, y, v, BURN, KEEP, LEAP, seed, xs, True)["ite"][a:e])
    # without the draws: the same effects
    nodraws = _fused(eng, binary, x, y, v, BURN, KEEP, LEAP, seed, xs, True, want_draws=False)
    full = _fused(eng, binary, x, y, v, BURN, KEEP, LEAP, seed, xs, True)
    key = "ite" if binary else "adrf"
    assert nodraws["draws"] is None and torch.equal(nodraws[key], full[key]) and torch.equal(nodraws["state"], plain["state"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. launch cuts and more than one trip of the tile loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_launch_cuts_change_nothing(torch, case):
    seed, binary = 4711, case["binary"]
    m = _model(41, case["z_dims"], case["p"], binary)
    x, y, v = _data(N, case["p"], 42, binary)
    eng = _engine(m)
    xs = np.linspace(0.0, 3.0, 17)
    one = _fused(eng, binary, x, y, v, BURN, KEEP, LEAP, seed, xs)
    cut = _fused(eng, binary, x, y, v, BURN, KEEP, LEAP, seed, xs, chunk=7)      # cuts in burn-in, at 28 | 35 across burn_in = 30, and after it
    _same_chain(torch, one, cut)
    key = "ite" if binary else "adrf"
    assert torch.equal(one[key], cut[key])


@pytest.mark.parametrize("binary", [False, True], ids=["continuous", "binary"])
def test_fused_beyond_one_trip_of_the_tile_loop(torch, binary):
    """16 x 8 x CUs x 2 + 37 rows: every wave slot adds two or three tiles into its partial sums, the last tile is ragged"""
    burn, keep, leap, seed = 3, 2, 2, 4242
    m = _model(65, [1, 1, 1, 7], 20, binary)
    eng = _engine(m)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = int(eng.mh_info(16).waves_per_block)
    n = 16 * waves * n_cus * 2 + 37
    assert waves == 8 and eng.mh_slots(n) == waves * n_cus and (n + 15) // 16 == 2 * waves * n_cus + 3
    x, y, v = _data(n, 20, 66, binary)
    xs = np.linspace(0.0, 3.0, 5)
    plain = eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, want_draws=True, adapt=TARGET)
    fused = _fused(eng, binary, x, y, v, burn, keep, leap, seed, xs)
    _same_chain(torch, plain, fused)
    _same_effects(torch, eng, binary, x, plain, fused, burn, seed, xs, True)


# ---------------------------------------------------------------------------------------------------------------------
# 4. with a metric
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_with_a_metric(torch, case):
    seed, binary, burn = 99, case["binary"], 40
    m = _model(31, case["z_dims"], case["p"], binary)
    q = sum(case["z_dims"])
    x, y, v = _data(N, case["p"], 32, binary)
    eng = _engine(m)
    xs = np.linspace(0.0, 3.0, 17)
    scale = np.random.RandomState(23).uniform(0.3, 3.0, (N, q)).astype(np.float32)
    identity = eng.hmc_sample(x, y, v, burn, KEEP, STEP0, LEAP, seed, want_draws=True, adapt=TARGET)
    for kw in (dict(mass="diag"), dict(mass_scale=scale)):
        plain = eng.hmc_sample(x, y, v, burn, KEEP, STEP0, LEAP, seed, want_draws=True, adapt=TARGET, **kw)
        assert not torch.equal(plain["draws"], identity["draws"])
        for sample_y in (True, False):
            fused = _fused(eng, binary, x, y, v, burn, KEEP, LEAP, seed, xs, sample_y, **kw)
            _same_chain(torch, plain, fused)
            _same_effects(torch, eng, binary, x, plain, fused, burn, seed, xs, sample_y)
        cut = _fused(eng, binary, x, y, v, burn, KEEP, LEAP, seed, xs, False, chunk=7, **kw)
        _same_chain(torch, plain, cut)
        key = "ite" if binary else "adrf"
        assert torch.equal(cut[key], fused[key])
    again = eng.hmc_sample(x, y, v, burn, KEEP, STEP0, LEAP, seed, want_draws=True, adapt=TARGET)      # the metric was cleared
    _same_chain(torch, identity, again)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the class surface
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


def _largest_outcome_draw(m, draws, xs, seed, burn):
    """max |mu + sd * noise| of the float64 oracle's outcome net over every draw, row and dose (binary: the two arms)"""
    m64 = OC.cast_model(m, np.float64)
    draws = draws.astype(np.float64)
    keep, n, _ = draws.shape
    doses = [1.0, 0.0] if m["binary_treatment"] else list(np.asarray(xs, np.float32).astype(np.float64))
    big = 0.0
    for d in range(keep):
        nz = R.normals_seq(np.arange(n), burn + d, len(doses), R.TAG_YNOISE, seed).astype(np.float64)
        z0, z1, _ = OC.split_z(m64, draws[d])
        for k, xv in enumerate(doses):
            out = mlp_forward(m64["f"], np.concatenate([z0, z1, np.full((n, 1), xv)], axis=-1))
            s2 = OC._sig2(m64, "sigma_y", out[:, 1], np.float64)
            big = max(big, float(np.abs(out[:, 0] + np.sqrt(s2) * nz[:, k]).max()))
    return big


@pytest.mark.parametrize("mass", ["identity", "diag"])
def test_predict_fused_is_the_draws_route(torch, tmp_path, mass):
    m = OC.init_model(0, Z_DIMS, P)
    n, burn, keep, q = 200, 40, 20, sum(Z_DIMS)
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    xs = np.linspace(0.0, 3.0, 5)
    kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, x_values=xs, verbose=0, sampler="hmc", step_size=0.1, n_leapfrog=3, mass=mass)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c, d = (_causal(tmp_path, m) for _ in range(4))
        eff_a, int_a = a.predict(data, **kw)                                      # the draws route, one block
        eff_b, int_b = b.predict(data, fused_effects=True, **kw)
        assert np.array_equal(eff_a, eff_b) and np.array_equal(int_a, int_b)
        assert np.array_equal(a.hmc_row_step_, b.hmc_row_step_) and a._seed_counter == b._seed_counter
        if mass == "diag":
            assert np.array_equal(a.hmc_row_mass_, b.hmc_row_mass_) and b.hmc_row_mass_.shape == (n, q)
        else:
            assert b.hmc_row_mass_ is None
        eff_c, int_c = c.predict(data, draw_budget_bytes=4 * keep * q * 48, **kw)      # the draws route in 48-row blocks
        out = b.engine.hmc_sample(x, y, v, burn, keep, 0.1, 3, _seed_of(b), want_draws=True, adapt=TARGET, mass=None if mass == "identity" else mass)
        big = _largest_outcome_draw(m, out["draws"].cpu().numpy(), xs, _seed_of(b), burn)
        bound = n * 2.0 ** -24 * big
        print("fused against 48-row blocks: effect %.3g, interval %.3g; bound %.3g (Y = %.3f)"
              % (np.abs(eff_c - eff_b).max(), np.abs(int_c - int_b).max(), bound, big))
        assert np.abs(eff_c - eff_b).max() <= bound and np.abs(int_c - int_b).max() <= bound
        assert np.array_equal(c.hmc_row_step_, b.hmc_row_step_) and c._seed_counter == b._seed_counter
        eff_d, int_d = d.predict(data, fused_effects=True, diagnose_rows=32, **kw)
        assert np.array_equal(eff_d, eff_b) and np.array_equal(int_d, int_b) and d._seed_counter == b._seed_counter
        assert d.mcmc_diagnostics_.rows.shape == (32,) and b.mcmc_diagnostics_ is None
        assert np.all(np.isfinite(eff_b)) and np.all(int_b[:, 0] <= eff_b) and np.all(eff_b <= int_b[:, 1])


def test_binary_predict_fused_is_the_draws_route(torch, tmp_path):
    m = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    n, burn, keep = 150, 30, 20
    data = _data(n, P, 8, True)
    kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, verbose=0, sampler="hmc", step_size=0.1, n_leapfrog=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c = (_causal(tmp_path, m, True) for _ in range(3))
        ite_a, int_a = a.predict(data, **kw)
        ite_b, int_b = b.predict(data, fused_effects=True, **kw)
        ite_c, int_c = c.predict(data, draw_budget_bytes=4 * keep * sum(Z_DIMS) * 48, **kw)      # rows do not interact: equal, not within a bound
    assert ite_b.shape == (n,) and int_b.shape == (n, 2) and np.all(np.isfinite(ite_b))
    assert np.array_equal(ite_a, ite_b) and np.array_equal(int_a, int_b)
    assert np.array_equal(ite_c, ite_b) and np.array_equal(int_c, int_b)
    assert np.array_equal(a.hmc_row_step_, b.hmc_row_step_) and a._seed_counter == b._seed_counter == c._seed_counter


# ---------------------------------------------------------------------------------------------------------------------
# 6. the LDS budget
# ---------------------------------------------------------------------------------------------------------------------
def test_a_generator_too_deep_for_the_fused_kernels_is_refused(torch):
    """seven layers of 64 at KT1 = 1: the HMC blob alone (162 192 B) fits the 160 KiB, with f's part of the sampling blob
    (16 128 B) it does not"""
    m = _model(71, [1, 1, 1, 7], 20, g_units=(64,) * 7)
    x, y, v = _data(40, 20, 72)
    eng = _engine(m, g_units=[64] * 7)
    xs = np.linspace(0.0, 3.0, 5)
    plain = eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, want_draws=True)
    with pytest.raises(RuntimeError, match=r"\(-4\).*178320 B.*draws route"):
        _fused(eng, False, x, y, v, 5, 5, 2, 7, xs)
    again = eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, want_draws=True)          # the handle stays usable
    _same_chain(torch, plain, again)
    # six layers fit (160 656 B): the deepest generator of this family the fused kernels hold
    m6 = _model(73, [1, 1, 1, 7], 20, g_units=(64,) * 6)
    eng6 = _engine(m6, g_units=[64] * 6)
    plain6 = eng6.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, want_draws=True, adapt=TARGET)
    fused6 = _fused(eng6, False, x, y, v, 5, 5, 2, 7, xs)
    _same_chain(torch, plain6, fused6)
    _same_effects(torch, eng6, False, x, plain6, fused6, 5, 7, xs, True)


def test_argument_checks(torch):
    m = _model(51, [1, 1, 1, 7], 20)
    x, y, v = _data(40, 20, 52)
    eng = _engine(m)
    with pytest.raises(ValueError, match="x_values"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, effect=_lib.EFFECT_ADRF)
    with pytest.raises(ValueError, match="effect"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, effect=_lib.EFFECT_ITE)          # a continuous treatment has no ITE
    with pytest.raises(ValueError, match="effect"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, effect=7)
    f = dict(device="cuda", dtype=torch.float32)
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (x.reshape(-1), y.reshape(-1), v))
    state, grad, logp, step = torch.empty(40, 10, **f), torch.empty(40, 10, **f), torch.empty(40, **f), torch.full((40,), 0.1, **f)
    xv = torch.linspace(0, 3, 5, **f)
    with pytest.raises(RuntimeError, match=r"\(-1\).*adrf_partial"):
        eng.hmc_run(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, init=True, n_keep=5, effect=_lib.EFFECT_ADRF, x_values=xv)
    partial = torch.zeros(eng.mh_slots(40), 5, 5, **f)
    with pytest.raises(RuntimeError, match=r"\(-1\).*beyond burn_in \+ n_keep"):
        eng.hmc_run(xt, yt, vt, state, logp, grad, step, 0, 11, 5, 2, 7, init=True, n_keep=5, effect=_lib.EFFECT_ADRF, x_values=xv,
                    adrf_partial=partial)
    assert not bool(partial.any())
    assert eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7)["row_step"].shape == (40,)


# ---------------------------------------------------------------------------------------------------------------------
# 7. one anchor outside the project's own kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=_id)
def test_fused_effects_match_the_float64_oracle_on_the_returned_draws(torch, case):
    seed, binary = 5, case["binary"]
    m = _model(51, case["z_dims"], case["p"], binary)
    x, y, v = _data(N, case["p"], 52, binary)
    xs = np.linspace(0.0, 3.0, 20)
    out = _fused(_engine(m), binary, x, y, v, BURN, KEEP, LEAP, seed, xs, sample_y=False)
    ref = OC.infer_from_latent_posterior(OC.cast_model(m, np.float64), out["draws"].cpu().numpy().astype(np.float64), None if binary else xs,
                                         False, seed, burn_in=BURN)
    got = out["ite"].cpu().numpy().T if binary else out["adrf"].cpu().numpy()
    print("fused %s against the float64 oracle: %.3g" % ("ITE" if binary else "ADRF", np.abs(got - ref).max()))
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 2e-4
