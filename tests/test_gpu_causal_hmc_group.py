"""The individual treatment effect of a binary treatment summed by row label inside the HMC sampler (csrc/causal_hmc_gfx_kernels.h,
bgm_causal_hmc_run_group_effects; hmc_sample(effect=EFFECT_GROUP_ITE), CausalBGM.predict_average) and the same sums from a stored
ITE matrix (bgm_ite_group_sums), against the ITE route: hmc_sample(effect=EFFECT_ITE) with the same seed, reduced in float64 NumPy.

Bars
  chain          bit-identity with the run without effects (draws, state, logp, grad, row_step, acc_count, mass_scale)
  label sums     a row's value is the ITE route's value bit for bit, so the fused sum of label c at draw d is a float32 summation of
                 the k = (rows with label c) values ite[i, d] in some fixed association, rounded once more to float32 by the slot
                 reduction: at most k roundings on partial sums no larger than sum_i |ite[i, d]|, hence
                     |fused - float64 sum| <= gamma_k * sum_i |ite[i, d]|,  gamma_k = k u / (1 - k u),  u = 2**-24
                 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4).  Derived, not measured; the largest observed
                 ratio is printed.  A label no row carries sums to exactly 0.0.
  launch cuts    bit-identity, group_partial included
  oracle         label averages of oracle.causal.infer_from_latent_posterior (float64, sample_y=False) on the returned draws against
                 the fused averages: 2e-4 absolute, the bar tests/test_gpu_causal.py applies to engine.effects per row -- an average
                 of values inside that bar is inside it.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402

from bayesgm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.75
BURN, KEEP, LEAP, STEP0 = 10, 12, 3, 0.1
SHAPES = [dict(z_dims=[1, 1, 1, 7], p=20), dict(z_dims=[3, 3, 6, 6], p=20)]      # both first-layer tilings (KT1 = 1, 2)
KEYS = ("draws", "state", "logp", "grad", "row_step", "acc_count")
N = 200                                                                             # 13 tiles, the last one of 8 rows
U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _slots(eng, n):
    """wave slots of the effect kernels for n rows: the leading dimension of group_partial"""
    import ctypes as C
    ns = C.c_int32()
    _lib.check(eng.lib.bgm_causal_evaluate_slots(eng.h, n, C.byref(ns)), "bgm_causal_evaluate_slots")
    return ns.value


def _gamma(k):
    return k * U / (1.0 - k * U)


def _ite(eng, x, y, v, burn, keep, leap, seed, sample_y=True, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, adapt=TARGET, effect=_lib.EFFECT_ITE, sample_y=sample_y, **kw)


def _group(eng, x, y, v, burn, keep, leap, seed, labels, n_labels, sample_y=True, **kw):
    return eng.hmc_sample(x, y, v, burn, keep, STEP0, leap, seed, adapt=TARGET, effect=_lib.EFFECT_GROUP_ITE, labels=labels,
                          n_labels=n_labels, sample_y=sample_y, **kw)


def _check_sums(got, ite, labels, n_labels):
    """got [n_labels, n_keep] (tensor) against the float64 sums of ite [n, n_keep] over every label's rows -> largest |error| / bound"""
    got = got.double().cpu().numpy()
    ite = (ite.cpu().numpy() if hasattr(ite, "cpu") else np.asarray(ite)).astype(np.float64)
    labels = np.asarray(labels)
    assert got.shape == (n_labels, ite.shape[1]) and np.all(np.isfinite(got))
    worst = 0.0
    for c in range(n_labels):
        rows = labels == c
        k = int(rows.sum())
        if k == 0:
            assert np.all(got[c] == 0.0), ("a label no row carries", c)
            continue
        ref, bound = ite[rows].sum(axis=0), _gamma(k) * np.abs(ite[rows]).sum(axis=0)
        err = np.abs(got[c] - ref)
        assert np.all(err <= bound), (c, k, float(err.max()), float(bound.min()))
        if k == 1:
            assert np.all(err == 0.0)
        worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
    return worst


def _same_chain(torch, plain, other):
    for k in KEYS + (("mass_scale",) if "mass_scale" in plain else ()):
        assert torch.equal(plain[k], other[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 1. + 2. the chain is unchanged and the sums are those of the ITE route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", [None, "diag"], ids=["identity", "diag"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "q%d" % sum(s["z_dims"]))
def test_chain_unchanged_and_sums_are_the_ite_route(torch, shape, mass):
    seed, burn = 99, (BURN if mass is None else 24)
    m = _model(31, shape["z_dims"], shape["p"], True)
    x, y, v = _data(N, shape["p"], 32, True)
    eng = _engine(m)
    labels = np.random.RandomState(7).randint(0, 5, N)          # label 5 of 6 stays empty
    kw = dict(mass=mass) if mass else {}
    plain = eng.hmc_sample(x, y, v, burn, KEEP, STEP0, LEAP, seed, want_draws=True, adapt=TARGET, **kw)
    assert 0 < int(plain["acc_count"].sum()) < (burn + KEEP) * N
    for sample_y in (True, False):
        ite = _ite(eng, x, y, v, burn, KEEP, LEAP, seed, sample_y, **kw)["ite"]
        grp = _group(eng, x, y, v, burn, KEEP, LEAP, seed, labels, 6, sample_y, want_draws=True, **kw)
        _same_chain(torch, plain, grp)
        assert "ite" not in grp and grp["group_partial"].shape == (_slots(eng, N), KEEP, 6)
        worst = _check_sums(grp["group_sums"], ite, labels, 6)
        print("label sums against the ITE route (q = %d, mass %s, sample_y %s): %.3f of the bound" % (sum(shape["z_dims"]), mass, sample_y, worst))
    nodraws = _group(eng, x, y, v, burn, KEEP, LEAP, seed, labels, 6, False, **kw)
    assert nodraws["draws"] is None and torch.equal(nodraws["group_partial"], grp["group_partial"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. tile shapes where the label walk can go wrong
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 17, 33])
def test_label_layouts_within_a_tile(torch, n):
    """one label per tile (one reduction), 16 distinct labels in a tile (16 reductions), a change exactly at the tile boundary, a
    ragged last tile of one row (n = 17, 33) whose 15 padding lanes carry the clamped last row's label, labels nobody carries"""
    burn, keep, leap, seed = 4, 3, 2, 11
    m = _model(33, [1, 1, 1, 7], 20, True)
    x, y, v = _data(n, 20, 34, True)
    eng = _engine(m)
    ite = _ite(eng, x, y, v, burn, keep, leap, seed)["ite"]
    r = np.arange(n)
    layouts = [("one label", np.zeros(n, np.int64), 1),
               ("change at the tile boundary", (r // 16) % 2, 2),
               ("16 distinct labels per tile", (r % 16) * 4 + 1 + (r // 16) % 2, 64),      # 0 and 63 stay empty
               ("scattered", np.random.RandomState(n).randint(0, 3, n) * 31, 64),
               ("last row alone in its label", np.where(r == n - 1, 63, 5), 64)]
    for name, labels, n_labels in layouts:
        grp = _group(eng, x, y, v, burn, keep, leap, seed, labels, n_labels)
        _check_sums(grp["group_sums"], ite, labels, n_labels)
        if name == "last row alone in its label":      # (a padding lane adding the clamped row once more would double it)
            assert torch.equal(grp["group_sums"][63], ite[n - 1]), name


def test_more_tiles_than_slots(torch):
    """16 x slots + 17 rows: every wave slot adds a second tile into its partial sums and one a ragged third of one row"""
    burn, keep, leap, seed = 3, 2, 2, 4242
    m = _model(65, [1, 1, 1, 7], 20, True)
    eng = _engine(m)
    slots = _slots(eng, 1 << 20)
    n = 16 * slots + 17
    assert _slots(eng, n) == slots and (n + 15) // 16 == slots + 2
    x, y, v = _data(n, 20, 66, True)
    ite = _ite(eng, x, y, v, burn, keep, leap, seed)["ite"]
    rs = np.random.RandomState(1)
    for labels, n_labels in ((rs.randint(0, 7, n), 8), (np.arange(n) * 16 // n, 16), (2 * (np.arange(n) % 3) + x.reshape(-1).astype(np.int64), 6)):
        grp = _group(eng, x, y, v, burn, keep, leap, seed, labels, n_labels)
        assert grp["group_partial"].shape == (slots, keep, n_labels)
        print("more tiles than slots, %d labels: %.3f of the bound" % (n_labels, _check_sums(grp["group_sums"], ite, labels, n_labels)))


# ---------------------------------------------------------------------------------------------------------------------
# 4. launch cuts and row windows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "q%d" % sum(s["z_dims"]))
def test_launch_cuts_and_row_windows(torch, shape):
    seed = 4711
    m = _model(41, shape["z_dims"], shape["p"], True)
    x, y, v = _data(N, shape["p"], 42, True)
    eng = _engine(m)
    labels = np.random.RandomState(9).randint(0, 4, N)
    one = _group(eng, x, y, v, BURN, KEEP, LEAP, seed, labels, 4, want_draws=True)
    cut = _group(eng, x, y, v, BURN, KEEP, LEAP, seed, labels, 4, want_draws=True, chunk=7)      # cuts at 7 | 14 across burn_in = 10, and at 21
    _same_chain(torch, one, cut)
    assert torch.equal(one["group_partial"], cut["group_partial"]) and torch.equal(one["group_sums"], cut["group_sums"])
    # rows [a, e) alone with their global row index: the sums of the same global rows of the full run's ITE
    a, e = 23, 171
    ite = _ite(eng, x, y, v, BURN, KEEP, LEAP, seed)["ite"]
    part = _group(eng, x[a:e], y[a:e], v[a:e], BURN, KEEP, LEAP, seed, labels[a:e], 4, want_draws=True, row_base=a)
    assert torch.equal(part["draws"], one["draws"][:, a:e])
    _check_sums(part["group_sums"], ite[a:e], labels[a:e], 4)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the sums from a stored matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keep", [1, 12])
@pytest.mark.parametrize("n", [1, 16, 1000])
def test_ite_group_sums(torch, n, n_keep):
    eng = _engine(_model(33, [1, 1, 1, 7], 20, True))
    rs = np.random.RandomState(n + n_keep)
    ite = (rs.randn(n, n_keep) * 5.0).astype(np.float32)
    dev = torch.from_numpy(ite).cuda()
    r = np.arange(n)
    for labels, n_labels in ((np.zeros(n, np.int64), 1), ((r // 16) % 2, 2), ((r % 16) * 4 + 1, 64), (rs.randint(0, 5, n), 6)):
        got = eng.ite_group_sums(dev, labels, n_labels)
        assert got.dtype == torch.float64
        _check_sums(got, ite, labels, n_labels)
        assert torch.equal(got, eng.ite_group_sums(dev, torch.from_numpy(labels), n_labels))
    with pytest.raises(ValueError, match="labels must lie in"):
        eng.ite_group_sums(dev, np.full(n, 2), 2)
    with pytest.raises(ValueError, match="n_labels must be in"):
        eng.ite_group_sums(dev, np.zeros(n, np.int64), 65)


# ---------------------------------------------------------------------------------------------------------------------
# 6. one anchor outside the project's own kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "q%d" % sum(s["z_dims"]))
def test_label_averages_match_the_float64_oracle_on_the_returned_draws(torch, shape):
    seed = 5
    m = _model(51, shape["z_dims"], shape["p"], True)
    x, y, v = _data(N, shape["p"], 52, True)
    labels = 2 * np.random.RandomState(3).randint(0, 3, N) + x.reshape(-1).astype(np.int64)      # (group, arm), as predict_average
    out = _group(_engine(m), x, y, v, BURN, KEEP, LEAP, seed, labels, 6, sample_y=False, want_draws=True)
    ref = OC.infer_from_latent_posterior(OC.cast_model(m, np.float64), out["draws"].cpu().numpy().astype(np.float64), None, False, seed,
                                         burn_in=BURN)                                            # [n_keep, n]
    got = out["group_sums"].double().cpu().numpy()
    worst = 0.0
    for c in range(6):
        rows = labels == c
        assert rows.sum() > 0
        worst = max(worst, float(np.abs(got[c] / rows.sum() - ref[:, rows].mean(axis=1)).max()))
    print("label averages against the float64 oracle: %.3g" % worst)
    assert worst <= 2e-4


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals of the library and of the engine
# ---------------------------------------------------------------------------------------------------------------------
def _raw(torch, eng, x, y, v, labels, n_labels, n_keep=5, partial=None):
    f = dict(device="cuda", dtype=torch.float32)
    n, q = v.shape[0], eng.q
    xt, yt, vt = (torch.from_numpy(a).cuda() for a in (x.reshape(-1), y.reshape(-1), v))
    state, grad, logp, step = torch.empty(n, q, **f), torch.empty(n, q, **f), torch.empty(n, **f), torch.full((n,), 0.1, **f)
    lab = torch.from_numpy(np.asarray(labels, np.int32)).cuda()
    partial = torch.zeros(_slots(eng, n), n_keep, max(1, min(n_labels, 64)), **f) if partial is None else partial
    eng.hmc_run_group_effects(xt, yt, vt, state, logp, grad, step, 0, 10, 5, 2, 7, labels=lab, n_labels=n_labels, group_partial=partial,
                              init=True, n_keep=n_keep)
    return partial


def test_refusals(torch):
    x, y, v = _data(40, 20, 52, True)
    labels = np.zeros(40, np.int64)
    cont = _engine(_model(51, [1, 1, 1, 7], 20))
    with pytest.raises(RuntimeError, match=r"\(-1\).*continuous treatment.*BGM_EFFECT_ADRF"):
        _raw(torch, cont, x, y, v, labels, 2)
    with pytest.raises(ValueError, match="binary treatment"):
        cont.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, effect=_lib.EFFECT_GROUP_ITE, labels=labels, n_labels=2)
    eng = _engine(_model(51, [1, 1, 1, 7], 20, True))
    for bad in (0, 65):
        with pytest.raises(RuntimeError, match=r"\(-1\).*n_labels must be in \[1, 64\]; got %d" % bad):
            _raw(torch, eng, x, y, v, labels, bad)
        with pytest.raises(ValueError, match="n_labels must be in"):
            eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, effect=_lib.EFFECT_GROUP_ITE, labels=labels, n_labels=bad)
    with pytest.raises(RuntimeError, match=r"\(-1\).*beyond burn_in \+ n_keep"):
        _raw(torch, eng, x, y, v, labels, 2, n_keep=4)
    for bad in (np.full(40, 2), np.full(40, -1), np.zeros(39, np.int64), np.zeros(40, np.float32), None):      # checked on the host, before a launch
        with pytest.raises(ValueError, match="labels"):
            eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, effect=_lib.EFFECT_GROUP_ITE, labels=bad, n_labels=2)
    with pytest.raises(ValueError, match="labels belong to"):
        eng.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7, effect=_lib.EFFECT_ITE, labels=labels, n_labels=2)
    assert bool(_raw(torch, eng, x, y, v, labels, 2).any())                                         # the handle stays usable
    # a generator too deep for the fused LDS budget: the error of hmc_run_effects, under this entry point's name
    deep = _engine(_model(71, [1, 1, 1, 7], 20, True, g_units=(64,) * 7), g_units=[64] * 7)
    with pytest.raises(RuntimeError, match=r"\(-4\).*178320 B.*draws route") as fused:
        _ite(deep, x, y, v, 5, 5, 2, 7)
    with pytest.raises(RuntimeError, match=r"\(-4\).*178320 B.*draws route") as group:
        _group(deep, x, y, v, 5, 5, 2, 7, labels, 2)
    assert str(group.value).replace("bgm_causal_hmc_run_group_effects", "bgm_causal_hmc_run_effects") == str(fused.value)
    assert deep.hmc_sample(x, y, v, 5, 5, 0.1, 2, 7)["row_step"].shape == (40,)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the class surface
# ---------------------------------------------------------------------------------------------------------------------
Z_DIMS, P = [3, 3, 3, 1], 50
N_CLS, BURN_CLS, KEEP_CLS = 150, 30, 20


def _causal(tmp_path, m, seed=3, **kw):
    from bayesgm_amd.models import CausalBGM
    params = dict(dataset="t", output_dir=str(tmp_path), save_res=False, save_model=False, binary_treatment=True, use_bnn=False,
                  z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
                  e_units=[64] * 5, dz_units=[64, 32, 8], kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, mixing_check=False, **kw)
    model = CausalBGM(params, random_seed=seed)
    model.set_weights(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
    return model


def _seed_of(model):
    return (model._base_seed * 1000003 + model._seed_counter) & 0x7FFFFFFFFFFFFFFF


def _mean_bound(ite, rows):
    """|average over `rows` and the draws, computed as predict_average does (float32 label sums per draw, then float64) minus the
    float64 mean over `rows` of predict's per-row means (float32 means over the n_keep draws)| is at most
        (gamma_k + gamma_{n_keep + 1}) * mean over rows and draws of |ite|:
    gamma_k for the label sums (the bound at the top of this file, averaged over the draws), gamma_{n_keep + 1} for a float32 sum
    of n_keep values and its division, row by row; the float64 steps of both sides are below 1e-15 relative."""
    ite = np.abs(ite[rows].astype(np.float64))
    return (_gamma(int(rows.sum())) + _gamma(ite.shape[1] + 1)) * float(ite.mean())


def test_predict_average_hmc(torch, tmp_path):
    m = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    x, y, v = data = _data(N_CLS, P, 8, True)
    arm = x.reshape(-1) > 0.5
    groups = np.random.RandomState(2).randint(0, 3, N_CLS) * 10 - 10          # -10, 0, 10 scattered over the rows
    kw = dict(alpha=0.05, n_mcmc=KEEP_CLS, burn_in=BURN_CLS, verbose=0, step_size=0.1, n_leapfrog=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c = (_causal(tmp_path, m) for _ in range(3))
        assert a.average_effects_ is None
        ate, bounds = a.predict_average(data, estimand="ate", **kw)
        row_mean, _ = b.predict(data, sampler="hmc", fused_effects=True, **kw)
        ite = b.engine.hmc_sample(x, y, v, BURN_CLS, KEEP_CLS, 0.1, 3, _seed_of(b), adapt=TARGET, effect=_lib.EFFECT_ITE)["ite"].cpu().numpy()
        cate, cbounds = c.predict_average(data, estimand="ate", groups=groups, **kw)
    assert np.allclose(ite.mean(axis=1), row_mean, rtol=1e-5, atol=1e-6)      # (the same run: the bound below is taken from its values)
    everyone = np.ones(N_CLS, bool)
    assert isinstance(ate, float) and bounds.shape == (2,) and bounds[0] <= ate <= bounds[1]
    err, bound = abs(ate - row_mean.astype(np.float64).mean()), _mean_bound(ite, everyone)
    print("predict_average against mean(predict's ITE): %.3g, bound %.3g" % (err, bound))
    assert err <= bound
    assert a._seed_counter == b._seed_counter == c._seed_counter == 1
    assert np.array_equal(a.hmc_row_step_, b.hmc_row_step_) and a.hmc_row_mass_ is None
    res = a.average_effects_
    assert res["groups"] is None and np.array_equal(res["counts"], [[(~arm).sum(), arm.sum()]])
    for name in ("ate", "att", "atc"):
        assert res[name].shape == (1,) and res[name + "_interval"].shape == (1, 2) and res[name + "_draws"].shape == (1, KEEP_CLS)
        assert res[name + "_draws"].dtype == np.float64 and np.all(np.isfinite(res[name + "_draws"]))
        assert res[name + "_interval"][0, 0] <= res[name][0] <= res[name + "_interval"][0, 1]
    n0, n1 = res["counts"][0]
    assert np.allclose((n0 + n1) * res["ate_draws"], n1 * res["att_draws"] + n0 * res["atc_draws"], rtol=1e-12, atol=1e-12)
    for name, rows in (("att", arm), ("atc", ~arm)):
        assert abs(res[name][0] - row_mean[rows].astype(np.float64).mean()) <= _mean_bound(ite, rows), name
    # subgroups: every group's ATE is that group's slice of the ungrouped ITE means
    assert cate.shape == (3,) and cbounds.shape == (3, 2) and list(c.average_effects_["groups"]) == [-10, 0, 10]
    assert c.average_effects_["ate_draws"].shape == (3, KEEP_CLS) and c.average_effects_["counts"].sum() == N_CLS
    for i, g in enumerate((-10, 0, 10)):
        rows = groups == g
        assert abs(cate[i] - row_mean[rows].astype(np.float64).mean()) <= _mean_bound(ite, rows), g
        assert cbounds[i, 0] <= cate[i] <= cbounds[i, 1]
        assert np.array_equal(c.average_effects_["counts"][i], [(rows & ~arm).sum(), (rows & arm).sum()])
    # the groups' sums add up to the panel's
    cnt = c.average_effects_["counts"].sum(axis=1, keepdims=True)
    total = (c.average_effects_["ate_draws"] * cnt).sum(axis=0) / N_CLS
    assert np.all(np.abs(total - res["ate_draws"][0]) <= 2 * _gamma(N_CLS) * np.abs(ite.astype(np.float64)).mean(axis=0))      # (both within gamma_n of the exact sums)


def test_predict_average_mh_and_a_group_without_treated_rows(torch, tmp_path):
    m = OC.init_model(0, Z_DIMS, P, binary_treatment=True)
    x, y, v = data = _data(N_CLS, P, 8, True)
    arm = x.reshape(-1) > 0.5
    kw = dict(alpha=0.05, n_mcmc=KEEP_CLS, burn_in=BURN_CLS, verbose=0, q_sd=0.5)
    groups = np.where(arm, 0, np.arange(N_CLS) % 2)                             # group 1 holds control rows only
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c = (_causal(tmp_path, m) for _ in range(3))
        att, bounds = a.predict_average(data, estimand="att", sampler="mh", **kw)
        row_mean, _ = b.predict(data, **kw)
        ite = b.engine.mh_sample(x, y, v, BURN_CLS, KEEP_CLS, 0.5, _seed_of(b), effect=_lib.EFFECT_ITE)["ite"].cpu().numpy()
        with pytest.raises(ValueError, match=r"estimand='att' is undefined for groups \[1\]"):
            c.predict_average(data, estimand="att", sampler="mh", groups=groups, **kw)
    assert np.allclose(ite.mean(axis=1), row_mean, rtol=1e-5, atol=1e-6)
    assert a._seed_counter == b._seed_counter == c._seed_counter == 1 and a.hmc_row_step_ is None
    res = a.average_effects_
    for name, rows in (("ate", np.ones(N_CLS, bool)), ("att", arm), ("atc", ~arm)):
        err, bound = abs(res[name][0] - row_mean[rows].astype(np.float64).mean()), _mean_bound(ite, rows)
        assert err <= bound, (name, err, bound)
    assert att == res["att"][0] and bounds[0] <= att <= bounds[1]
    res = c.average_effects_                                                    # left behind although the estimand asked for is undefined
    assert np.isnan(res["att"][1]) and np.all(np.isnan(res["att_draws"][1])) and np.isfinite(res["att"][0])
    assert np.all(np.isfinite(res["ate"])) and np.all(np.isfinite(res["atc"])) and res["counts"][1, 1] == 0
