"""The trajectory options of the CausalBGM HMC sampler on the GPU (csrc/causal_hmc_traj_kernels.h, bgm_causal_hmc_set_trajectory):
max_trajectory caps the leapfrog steps of a chain by its own step, jitter draws their number per chain and iteration, and a wave's
loop ends at the largest count of its 16 rows.

Everything is bit-identity except
  chains against the restatement   the bars of tests/test_gpu_causal_hmc.py::test_chain_and_step_match_restatement: last draw within
                                   1e-4 of the float32 restatement (tests/_causal_hmc_traj_ref.py) on >= 97 % of the rows, the step
                                   equal bit for bit on those rows, acc_count off by at most the number of other rows; n_steps equal
                                   on >= 97 % of the rows.  The float32 restatement follows its float64 twin on 100 % of the rows of
                                   the same cases (tests/test_causal_hmc_traj_host.py).
  the defect and its cure          median lag-1 autocorrelation of the draws, printed with two digits: one chain of the 16 that
                                   leaves the restatement's accept history moves the median over the 160 series by about 1e-3, so
                                   two digits are what a float32 run reproduces; the float64 and the float32 restatement agree to
                                   four.  The margin is the float64 restatement's own gap less the two roundings (0.01).
The models are those of tests/test_gpu_causal_hmc.py at p = 20, both first-layer tilings (q + 1 = 11 and 19)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_traj_ref as TR  # noqa: E402
import _causal_partial_ref as PR  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402

from bayesgm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = TR.TARGET
P = 20
KT = {1: [1, 1, 1, 7], 2: [3, 3, 6, 6]}
KEYS = ("draws", "state", "logp", "grad", "acc_count", "row_step")
XS = np.linspace(0.0, 3.0, 5)
T_CAP, L_CAP = 0.13, 6                               # 0.05 -> 3 steps, 0.03 -> 5 steps (test_causal_hmc_traj_host.py: no tie)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _setup(kt1, binary, n, seed, mixed=False):
    m = _model(seed, KT[kt1], P, binary)
    x, y, v = _data(n, P, seed + 1, binary)
    if mixed:
        x, y = PR.mixed_panel(x, y, seed + 2)
    return m, _engine(m), x, y, v


def _fixed(torch, eng, x, y, v, step, L, keep, seed, T=None, jitter=False, row_base=0, count=True):
    """`keep` retained transitions from the initial state under frozen steps `step` [n] (hmc_run, one launch) -> dict of KEYS + n_steps"""
    from bayesgm_amd.engine import _f32
    dev, n, q = eng.device, v.shape[0], eng.q
    x_, y_, v_ = (_f32(t, dev) for t in (x, y, v))
    out = dict(state=torch.empty((n, q), device=dev), logp=torch.empty(n, device=dev), grad=torch.empty((n, q), device=dev),
               row_step=_f32(np.zeros(n, np.float32) + np.asarray(step, np.float32), dev).clone(),
               acc_count=torch.zeros(keep, device=dev, dtype=torch.int32), draws=torch.empty((keep, n, q), device=dev),
               n_steps=torch.zeros(n, device=dev, dtype=torch.int32))
    on = T is not None or jitter
    if on:
        eng.set_hmc_trajectory(T, jitter, out["n_steps"] if count else None)
    try:
        eng.hmc_run(x_.reshape(-1), y_.reshape(-1), v_, out["state"], out["logp"], out["grad"], out["row_step"], 0, keep, 0, L, seed, init=True,
                    row_base=row_base, acc_count=out["acc_count"], draws=out["draws"], n_keep=keep)
    finally:
        if on:
            eng.set_hmc_trajectory(None)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. the option changes nothing when it does not bind
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = [
    ("plain-kt1", 1, False, {}), ("plain-kt2", 2, True, {}),
    ("mass-kt1", 1, False, dict(mass=True)), ("mass-kt2", 2, True, dict(mass=True)),
    ("partial-kt1", 1, False, dict(partial=True)), ("partial-kt2", 2, True, dict(partial=True)), ("partial-mass-kt2", 2, False, dict(partial=True, mass=True)),
    ("adrf-kt1", 1, False, dict(effect=_lib.EFFECT_ADRF)), ("adrf-mass-kt2", 2, False, dict(effect=_lib.EFFECT_ADRF, mass=True)),
    ("ite-kt2", 2, True, dict(effect=_lib.EFFECT_ITE)), ("ite-mass-kt1", 1, True, dict(effect=_lib.EFFECT_ITE, mass=True)),
    ("ite-partial-kt2", 2, True, dict(effect=_lib.EFFECT_ITE, partial=True)), ("ite-partial-mass-kt1", 1, True, dict(effect=_lib.EFFECT_ITE, partial=True, mass=True)),
    ("rows-kt1", 1, False, dict(rows=True)), ("rows-mass-kt2", 2, False, dict(rows=True, mass=True)),
    ("rows-partial-kt2", 2, False, dict(rows=True, partial=True)), ("rows-partial-mass-kt1", 1, False, dict(rows=True, partial=True, mass=True)),
]


@pytest.mark.parametrize("name,kt1,binary,opt", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_an_option_that_does_not_bind_changes_nothing(torch, name, kt1, binary, opt):
    """(0, 0, NULL) runs the existing kernels; a cap that never binds (T = 1e9) runs the TRAJ twins: both equal the run without the
    option bit for bit while adapting, on every twin (plain, fused ADRF / ITE, per-row moments; metric; observation pattern)."""
    n, burn, keep, L, seed = 33, 8, 6, 4, 4711
    m, eng, x, y, v = _setup(kt1, binary, n, 71, mixed=bool(opt.get("partial")))
    kw = dict(want_draws=True, adapt=TARGET, chunk=5, partial=bool(opt.get("partial")))
    keys = KEYS
    if opt.get("mass"):
        kw["mass_scale"] = torch.from_numpy(np.exp(0.3 * np.random.RandomState(5).randn(n, eng.q)).astype(np.float32))
    if "effect" in opt:
        kw.update(effect=opt["effect"], x_values=None if binary else XS)
        keys = keys + (("ite",) if binary else ("adrf",))
    if opt.get("rows"):
        kw.update(row_effects=True, x_values=XS, row_draws=True)
        keys = keys + ("row_mean", "row_sd", "row_draws")
    base = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, **kw)
    eng.set_hmc_trajectory(None, False, None)
    off = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, **kw)
    free = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, max_trajectory=1e9, **kw)
    for k in keys:
        assert torch.equal(base[k], off[k]), k
        assert torch.equal(base[k], free[k]), k
    assert "n_steps" not in off and bool(torch.all(free["n_steps"] == L * keep)) and bool(torch.all(free["row_leapfrog"] == float(L)))
    assert float(base["row_step"].min()) < float(base["row_step"].max()) and 0 < int(base["acc_count"].sum())
    assert bool(torch.isfinite(base["draws"]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. a uniform cap equals a shorter trajectory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 33])
@pytest.mark.parametrize("kt1,binary", [(1, False), (2, True)], ids=["kt1", "kt2"])
def test_a_uniform_cap_is_a_shorter_trajectory(torch, kt1, binary, n):
    keep, seed = 6, 99
    m, eng, x, y, v = _setup(kt1, binary, n, 31)
    capped = _fixed(torch, eng, x, y, v, 0.05, L_CAP, keep, seed, T=T_CAP)
    short = _fixed(torch, eng, x, y, v, 0.05, 3, keep, seed)
    for k in KEYS:
        assert torch.equal(capped[k], short[k]), k
    assert bool(torch.all(capped["n_steps"] == 3 * keep)) and bool(torch.all(short["n_steps"] == 0))
    long = _fixed(torch, eng, x, y, v, 0.05, L_CAP, keep, seed)
    assert not torch.equal(long["draws"], short["draws"]) and 0 < int(capped["acc_count"].sum())
    # without the counter the chain is the same
    silent = _fixed(torch, eng, x, y, v, 0.05, L_CAP, keep, seed, T=T_CAP, count=False)
    assert torch.equal(silent["draws"], capped["draws"]) and bool(torch.all(silent["n_steps"] == 0))


# ---------------------------------------------------------------------------------------------------------------------
# 3. mixed caps inside a tile, and a tile of 3 next to a tile of 5
# ---------------------------------------------------------------------------------------------------------------------
def _steps(layout, n):
    rows = np.arange(n)
    five = (rows % 2 == 1) if layout == "interleaved" else ((rows // 16) % 2 == 1)
    return np.where(five, 0.03, 0.05).astype(np.float32), five


@pytest.mark.parametrize("layout", ["interleaved", "by-tile"])
@pytest.mark.parametrize("kt1,binary,opt", [(1, False, {}), (2, True, {}), (2, False, dict(mass=True, partial=True))], ids=["kt1", "kt2", "kt2-mass-partial"])
def test_mixed_caps(torch, kt1, binary, opt, layout):
    """Rows at step 0.05 take 3 of the 6 steps, rows at 0.03 take 5: each row equals the existing kernel's run at its own count
    and step, bit for bit -- a lane past its count must stand still while its wave goes on (interleaved), and a wave must stop at
    its own largest count (by tile: the early exit)."""
    n, keep, seed = 49, 5, 1234
    m, eng, x, y, v = _setup(kt1, binary, n, 41, mixed=bool(opt.get("partial")))
    step, five = _steps(layout, n)
    scale = torch.from_numpy(np.exp(0.3 * np.random.RandomState(6).randn(n, eng.q)).astype(np.float32)).to(eng.device) if opt.get("mass") else None
    ctx = eng._partial_rows(bool(opt.get("partial")), torch.from_numpy(x.ravel()), torch.from_numpy(y.ravel()))
    with ctx:
        try:
            if scale is not None:
                eng.set_hmc_mass(scale)
            mixed = _fixed(torch, eng, x, y, v, step, L_CAP, keep, seed, T=T_CAP)
            three = _fixed(torch, eng, x, y, v, 0.05, 3, keep, seed)
            fives = _fixed(torch, eng, x, y, v, 0.03, 5, keep, seed)
        finally:
            eng.set_hmc_mass(None)
    five_t = torch.from_numpy(five).to(eng.device)
    assert torch.equal(mixed["n_steps"], torch.where(five_t, 5 * keep, 3 * keep).int())
    for k in ("state", "logp", "grad", "row_step"):
        assert torch.equal(mixed[k][~five_t], three[k][~five_t]), k
        assert torch.equal(mixed[k][five_t], fives[k][five_t]), k
    assert torch.equal(mixed["draws"][:, ~five_t], three["draws"][:, ~five_t]) and torch.equal(mixed["draws"][:, five_t], fives["draws"][:, five_t])
    assert not torch.equal(three["draws"][:, five_t], fives["draws"][:, five_t])
    assert 0 < int(mixed["acc_count"].sum())


# ---------------------------------------------------------------------------------------------------------------------
# 4. against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True], ids=["cap", "cap-jitter"])
@pytest.mark.parametrize("case", TR.PARITY_CASES, ids=["kt1", "kt2"])
def test_chain_step_and_counts_match_the_restatement(torch, case, jitter):
    Pr = TR.PARITY
    m, (x, y, v) = TR.parity_inputs(case)
    eng = _engine(m)
    kw = dict(want_draws=True, chunk=7, adapt=TARGET, max_trajectory=Pr["max_trajectory"], jitter=jitter)
    out = eng.hmc_sample(x, y, v, Pr["burn_in"], Pr["n_keep"], Pr["step0"], Pr["n_leapfrog"], Pr["seed"], **kw)
    again = eng.hmc_sample(x, y, v, Pr["burn_in"], Pr["n_keep"], Pr["step0"], Pr["n_leapfrog"], Pr["seed"], **kw)
    for k in KEYS + ("n_steps",):
        assert torch.equal(out[k], again[k]), k
    ref = TR.parity_run(case, jitter)
    draws, acc, step = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy().astype(np.int64), out["row_step"].cpu().numpy()
    n_steps = out["n_steps"].cpu().numpy()
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    same = n_steps == ref["n_steps"]
    print("rows equal to the restatement: %.4f; n_steps equal: %.4f; acceptance %.3f; mean L_i %.3f of %d"
          % (row_ok.mean(), same.mean(), acc.sum() / float(acc.size * case["n"]), n_steps.mean() / Pr["n_keep"], Pr["n_leapfrog"]))
    assert row_ok.mean() >= 0.97, row_ok.mean()
    assert same.mean() >= 0.97, same.mean()
    assert np.array_equal(step[row_ok], ref["step"][row_ok])
    assert np.abs(acc - ref["acc"].sum(axis=1)).max() <= int((~row_ok).sum())
    assert n_steps.dtype == np.int32 and n_steps.min() >= Pr["n_keep"] and n_steps.max() < Pr["n_keep"] * Pr["n_leapfrog"]
    # (the mean is a float32 quotient made on the device: two roundings of 2^-24 each against the exact one)
    np.testing.assert_allclose(out["row_leapfrog"].cpu().numpy().astype(np.float64), n_steps / float(Pr["n_keep"]), rtol=2.0 ** -22, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. cuts, windows and the second trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt1,binary", [(1, False), (2, True)], ids=["kt1", "kt2"])
def test_cuts_and_windows_change_no_bit(torch, kt1, binary):
    n, burn, keep, L, seed = 49, 7, 6, 6, 2024
    m, eng, x, y, v = _setup(kt1, binary, n, 51)
    kw = dict(want_draws=True, adapt=TARGET, max_trajectory=0.35, jitter=True)
    full = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, **kw)
    cut = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, chunk=5, **kw)             # launches [0, 5), [5, 10), [10, 13)
    one = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, chunk=1, **kw)
    for k in KEYS + ("n_steps",):
        assert torch.equal(full[k], cut[k]), k
        assert torch.equal(full[k], one[k]), k
    s = 21                                                                            # a window that starts inside a tile
    part = eng.hmc_sample(x[s:], y[s:], v[s:], burn, keep, 0.1, L, seed, row_base=s, **kw)
    assert torch.equal(full["draws"][:, s:], part["draws"])
    for k in ("state", "logp", "grad", "row_step", "n_steps"):
        assert torch.equal(full[k][s:], part[k]), k
    assert len(torch.unique(full["n_steps"])) > 2 and int(full["n_steps"].max()) < L * keep


def test_beyond_one_trip_of_the_tile_loop(torch):
    """More 16-row tiles than wave slots and a ragged last tile (tests/test_gpu_causal_hmc.py, _two_trip_panel) against a partition
    of the rows, each part within one trip and with its own row_base: bit for bit, n_steps included."""
    from tests.test_gpu_causal_hmc import _two_trip_panel
    burn, keep, L, seed = 3, 2, 4, 4242
    eng, m, x, y, v, n, slots = _two_trip_panel(torch, 65)
    kw = dict(want_draws=True, adapt=TARGET, max_trajectory=0.25, jitter=True)
    full = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, **kw)
    cuts = [0, n // 3 // 16 * 16 + 7, 2 * n // 3 // 16 * 16, n]
    assert cuts[1] % 16 != 0 and all((e - s + 15) // 16 <= slots for s, e in zip(cuts[:-1], cuts[1:]))
    parts = [eng.hmc_sample(x[s:e], y[s:e], v[s:e], burn, keep, 0.1, L, seed, row_base=s, **kw) for s, e in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(full["draws"], torch.cat([p["draws"] for p in parts], dim=1))
    for k in ("state", "logp", "grad", "row_step", "n_steps"):
        assert torch.equal(full[k], torch.cat([p[k] for p in parts], dim=0)), k
    assert torch.equal(full["acc_count"], sum(p["acc_count"] for p in parts))
    assert bool(torch.isfinite(full["draws"]).all()) and 0 < int(full["acc_count"].sum()) < (burn + keep) * n
    assert int(full["n_steps"].min()) >= keep and int(full["n_steps"].max()) <= L * keep and len(torch.unique(full["n_steps"])) > 2


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_kernels_without_a_twin_refuse_and_bad_arguments_are_named(torch):
    n, burn, keep, L, seed = 20, 3, 4, 3, 7
    m, eng, x, y, v = _setup(1, False, n, 61)
    mb, engb, xb, yb, vb = _setup(2, True, n, 63)
    labels = np.arange(n) % 2
    for setting, word in (((1.0, False, None), "max_trajectory"), ((None, True, None), "jitter"),
                          ((None, False, torch.zeros(n, device=eng.device, dtype=torch.int32)), "n_steps_dev")):
        for e in (eng, engb):
            e.set_hmc_trajectory(*setting)
        with pytest.raises(RuntimeError, match=r"bgm_causal_hmc_run_row_tails failed \(-4\).*tail-buffer kernels.*%s is set" % word):
            eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, row_effects=True, x_values=XS, row_tails=2)
        with pytest.raises(RuntimeError, match=r"bgm_causal_hmc_run_group_effects failed \(-4\).*label-sum kernels.*%s is set" % word):
            engb.hmc_sample(xb, yb, vb, burn, keep, 0.1, L, seed, effect=_lib.EFFECT_GROUP_ITE, labels=labels, n_labels=2)
        for e in (eng, engb):
            e.set_hmc_trajectory(None)
    # the handles are usable afterwards, on the refused routes too
    assert eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, row_effects=True, x_values=XS, row_tails=2)["tails"].shape == (2, 2, len(XS), n)
    assert engb.hmc_sample(xb, yb, vb, burn, keep, 0.1, L, seed, effect=_lib.EFFECT_GROUP_ITE, labels=labels, n_labels=2)["group_sums"].shape == (2, keep)
    assert eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, max_trajectory=0.25)["n_steps"].shape == (n,)
    # the engine names the route before anything is launched
    with pytest.raises(ValueError, match="row_tails"):
        eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, row_effects=True, x_values=XS, row_tails=2, max_trajectory=1.0)
    with pytest.raises(ValueError, match="EFFECT_GROUP_ITE"):
        engb.hmc_sample(xb, yb, vb, burn, keep, 0.1, L, seed, effect=_lib.EFFECT_GROUP_ITE, labels=labels, n_labels=2, jitter=True)
    # bad arguments: BGM_E_INVALID naming the argument, nothing stored
    lib = eng.lib
    for args, word in (((-1.0, 0), "max_trajectory"), ((float("nan"), 0), "max_trajectory"), ((float("inf"), 1), "max_trajectory"),
                       ((1.0, 2), "jitter"), ((0.0, -1), "jitter")):
        assert lib.bgm_causal_hmc_set_trajectory(eng.h, args[0], args[1], None) == -1
        assert word in lib.bgm_last_error().decode()
    plain = eng.hmc_sample(x, y, v, burn, keep, 0.1, L, seed, want_draws=True)
    assert "n_steps" not in plain and bool(torch.isfinite(plain["draws"]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. the class
# ---------------------------------------------------------------------------------------------------------------------
def _causal(tmp_path, m, binary=False, seed=3):
    from bayesgm_amd.models import CausalBGM
    params = dict(dataset="t", output_dir=str(tmp_path), save_res=False, save_model=False, binary_treatment=binary, use_bnn=False,
                  z_dims=KT[1], v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
                  e_units=[64] * 5, dz_units=[64, 32, 8], kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, mixing_check=False)
    model = CausalBGM(params, random_seed=seed)
    model.set_weights(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
    return model


def _seed_of(model):
    return (model._base_seed * 1000003 + model._seed_counter) & 0x7FFFFFFFFFFFFFFF


def _check_leapfrog(model, n, L):
    lf = model.hmc_row_leapfrog_
    assert lf.shape == (n,) and lf.dtype == np.float32 and np.all(lf >= 1.0) and np.all(lf <= L) and lf.min() < L


def test_class_continuous(torch, tmp_path):
    m = OC.init_model(0, KT[1], P)
    n, burn, keep, L = 70, 20, 12, 6
    x, y, v = _data(n, P, 8)
    data = (x, y, v)
    opt = dict(max_trajectory=0.35, jitter_leapfrog=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = _causal(tmp_path, m)
        draws = a.hmc_sampler(data, n_keep=keep, burn_in=burn, step_size=0.1, n_leapfrog=L, **opt)
        ref = a.engine.hmc_sample(x, y, v, burn, keep, 0.1, L, _seed_of(a), want_draws=True, adapt=TARGET, max_trajectory=0.35, jitter=True)
        assert np.array_equal(ref["draws"].cpu().numpy(), draws) and np.array_equal(ref["row_leapfrog"].cpu().numpy(), a.hmc_row_leapfrog_)
        _check_leapfrog(a, n, L)
        plain = _causal(tmp_path, m)
        assert not np.array_equal(plain.hmc_sampler(data, n_keep=keep, burn_in=burn, step_size=0.1, n_leapfrog=L), draws)
        assert plain.hmc_row_leapfrog_ is None
        # predict: the draws route in one block is the fused route, bit for bit, with the options as without
        kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, x_values=XS, verbose=0, sampler="hmc", step_size=0.1, n_leapfrog=L, **opt)
        b, c = _causal(tmp_path, m), _causal(tmp_path, m)
        eff_b, int_b = b.predict(data, **kw)
        eff_c, int_c = c.predict(data, fused_effects=True, **kw)
        assert np.array_equal(eff_b, eff_c) and np.array_equal(int_b, int_c) and np.array_equal(b.hmc_row_leapfrog_, c.hmc_row_leapfrog_)
        assert np.array_equal(b.hmc_row_step_, c.hmc_row_step_) and np.all(np.isfinite(eff_b))
        _check_leapfrog(b, n, L)
        d = _causal(tmp_path, m)
        eff_d, _ = d.predict(data, **{k: w for k, w in kw.items() if k not in opt})
        assert d.hmc_row_leapfrog_ is None and not np.array_equal(eff_d, eff_b)
        # predict_individual: blocks by draw_budget_bytes change no bit
        kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=L, interval="quantile", **opt)
        e, f = _causal(tmp_path, m), _causal(tmp_path, m)
        mean_e, bounds_e = e.predict_individual(data, XS, **kw)
        mean_f, bounds_f = f.predict_individual(data, XS, draw_budget_bytes=4 * keep * len(XS) * 32, **kw)      # 32-row blocks
        assert np.array_equal(mean_e, mean_f) and np.array_equal(bounds_e, bounds_f) and np.array_equal(e.hmc_row_leapfrog_, f.hmc_row_leapfrog_)
        assert np.array_equal(e.individual_sd_, f.individual_sd_) and mean_e.shape == (n, len(XS))
        _check_leapfrog(e, n, L)
        # predict_new: the rows the cap is for
        g, h = _causal(tmp_path, m), _causal(tmp_path, m)
        mean_g, bounds_g = g.predict_new(v, None, XS, **kw)
        mean_h, bounds_h = h.predict_new(v, None, XS, draw_budget_bytes=4 * keep * len(XS) * 32, **kw)
        assert np.array_equal(mean_g, mean_h) and np.array_equal(bounds_g, bounds_h) and np.array_equal(g.hmc_row_leapfrog_, h.hmc_row_leapfrog_)
        assert np.all(np.isfinite(mean_g)) and np.all(bounds_g[..., 0] <= bounds_g[..., 1])
        _check_leapfrog(g, n, L)


def test_class_binary(torch, tmp_path):
    m = OC.init_model(0, KT[1], P, binary_treatment=True)
    n, burn, keep, L = 70, 20, 12, 6
    x, y, v = _data(n, P, 8, True)
    data = (x, y, v)
    kw = dict(alpha=0.05, n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=L, max_trajectory=0.35, jitter_leapfrog=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c = (_causal(tmp_path, m, True) for _ in range(3))
        ite_a, int_a = a.predict(data, sampler="hmc", **kw)
        ite_b, int_b = b.predict(data, sampler="hmc", draw_budget_bytes=4 * keep * sum(KT[1]) * 32, **kw)      # 32-row blocks
        ite_c, int_c = c.predict(data, sampler="hmc", fused_effects=True, **kw)
        for ite, bounds, model in ((ite_b, int_b, b), (ite_c, int_c, c)):
            assert np.array_equal(ite_a, ite) and np.array_equal(int_a, bounds) and np.array_equal(a.hmc_row_leapfrog_, model.hmc_row_leapfrog_)
        assert ite_a.shape == (n,) and np.all(np.isfinite(ite_a))
        _check_leapfrog(a, n, L)
        d, e = _causal(tmp_path, m, True), _causal(tmp_path, m, True)
        x_some = x.ravel().copy()
        x_some[::4] = np.nan
        mean_d, bounds_d = d.predict_new(v, x_some, interval="quantile", **kw)
        mean_e, bounds_e = e.predict_new(v, x_some, interval="quantile", draw_budget_bytes=4 * keep * 32, **kw)
        assert np.array_equal(mean_d, mean_e) and np.array_equal(bounds_d, bounds_e) and np.array_equal(d.hmc_row_leapfrog_, e.hmc_row_leapfrog_)
        _check_leapfrog(d, n, L)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the defect and its cure
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cap_cures_the_periodic_trajectory(torch):
    """New units (x and y unobserved: the posterior is close to the prior) under a frozen step with eps x L = 6.3, about 2 pi: a
    trajectory returns to its start and the draws barely move.  max_trajectory = pi / 2 (2 of the 6 steps) cures it.  The bar comes
    from the float64 restatement on the same panel (tests/test_causal_hmc_traj_host.py checks that it shows the gap on its own)."""
    D = TR.DEFECT
    m, (x, y, v) = TR.defect_inputs()
    eng = _engine(m)
    ref = {c: np.median(TR.lag1(TR.defect_run(c)["draws"])) for c in (False, True)}
    got, steps = {}, {}
    for capped in (False, True):
        out = eng.hmc_sample(x, y, v, 0, D["n_keep"], D["step"], D["n_leapfrog"], D["seed"], want_draws=True, adapt=None, partial=True,
                             max_trajectory=D["max_trajectory"] if capped else None)
        got[capped] = np.median(TR.lag1(out["draws"].cpu().numpy()))
        steps[capped] = out.get("n_steps")
    print("median lag-1 autocorrelation, uncapped / max_trajectory = pi / 2: GPU %+.4f / %+.4f, float64 restatement %+.4f / %+.4f"
          % (got[False], got[True], ref[False], ref[True]))
    assert steps[False] is None and bool(torch.all(steps[True] == 2 * D["n_keep"]))
    margin = (ref[False] - ref[True]) - 0.01
    assert margin > 1.0
    assert got[True] < got[False] - margin, (got, ref)
    for capped in (False, True):
        assert "%+.2f" % got[capped] == "%+.2f" % ref[capped], (capped, got[capped], ref[capped])
