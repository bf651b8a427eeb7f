"""The per-chain proposal scale of the MH sampler on the GPU (csrc/causal_kernels.h ROWADAPT, bgm_causal_set_row_scale) against the
NumPy restatement (tests/_row_adapt_ref.py), and the properties that make it usable: nothing else changes, a chain depends on its
own row only, the effect paths keep their invariants, predict does not depend on bs and can be diagnosed.

Tolerances are those of the tests whose checks are repeated here under row adaptation:
  chains against the oracle        tests/test_gpu_causal.py::test_mh_chain_matches_oracle_chain: rows equal within 1e-4 on >= 99 %
                                   (a uniform within rounding of the acceptance ratio flips a decision); a row counted equal made
                                   the oracle's decisions, so its scale must equal the oracle's BIT FOR BIT
  Gram against direct likelihood   tests/test_gpu_mh_gram_likelihood.py: states within 1e-4 on >= 99 % of the rows, acceptance counts
                                   within max(2, n // 50), cached log posterior within 2e-6 |ref| + 2e-4 of float64
  acceptance on the concentrated   target +/- 0.05, the reference's `tolerance` default (base.py:821)
  panel
everything else is bit-identity."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _row_adapt_ref import concentrated_model, concentrated_panel, row_adapt_sampler  # noqa: E402
from oracle import causal as OC  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = 0.25


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


def _table(burn, target=TARGET):
    from bayesgm_amd.row_adapt import row_adapt_factors
    return row_adapt_factors(burn, target)


# ---------------------------------------------------------------------------------------------------------------------
# 1. parity with the restatement (the shapes and the criterion of test_mh_chain_matches_oracle_chain)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=200),
                                  dict(z_dims=[3, 3, 6, 6], p=100, binary=True, n=150),
                                  dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=40),
                                  dict(z_dims=[1, 1, 1, 7], p=50, binary=False, n=60),
                                  dict(z_dims=[2, 2, 2, 6], p=150, binary=True, n=50)])
def test_chain_and_scale_match_restatement(torch, case):
    burn, keep, q_sd, seed = 25, 35, 0.3, 1234567890123
    m = _model(21, case["z_dims"], case["p"], case["binary"])
    x, y, v = _data(case["n"], case["p"], 22, case["binary"])
    eng = _engine(m)
    out = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, want_draws=True, chunk=17, row_adapt=TARGET)  # odd chunking on purpose
    draws, acc, scale = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy(), out["row_scale"].cpu().numpy()
    up, dn = _table(burn)
    ref = row_adapt_sampler(m, (x, y, v), burn, keep, q_sd, seed, up, dn)
    assert draws.shape == ref["draws"].shape == (keep, case["n"], sum(case["z_dims"]))
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    print("rows equal to the restatement: %.4f; scale q05 / median / q95 %.4f / %.4f / %.4f"
          % (row_ok.mean(), *np.quantile(scale, [0.05, 0.5, 0.95])))
    assert row_ok.mean() >= 0.99, row_ok.mean()
    assert scale.dtype == np.float32 and np.array_equal(scale[row_ok], ref["scale"][row_ok])
    assert np.ptp(scale) > 0                                                    # the chains adapted, and not all alike
    assert np.abs(acc.astype(np.int64) - ref["acc"].sum(axis=1)).max() <= max(2, case["n"] // 50)
    assert np.all(np.abs(out["state"].cpu().numpy()[row_ok] - ref["state"][row_ok]) <= 1e-4)
    assert np.array_equal(out["state"].cpu().numpy(), draws[-1])
    lp = eng.logpost(x.ravel(), y.ravel(), v, out["state"]).cpu().numpy()
    assert np.abs(lp - out["logp"].cpu().numpy()).max() <= 1e-3
    # determinism + chunking invariance: one launch, same seed -> identical bits, scales included
    out2 = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, want_draws=True, row_adapt=TARGET)
    assert torch.equal(out2["draws"], out["draws"]) and torch.equal(out2["row_scale"], out["row_scale"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. a neutral table changes nothing; a handle that set and cleared the scale equals one that never did
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=150),      # Gram form, 13 tiles
                                  dict(z_dims=[3, 3, 6, 6], p=100, binary=True, n=100),       # Gram form, two-K-tile first layer, ITE
                                  dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=70)])       # direct form (2 tiles)
@pytest.mark.parametrize("cache", [True, "wave", False])
def test_neutral_table_is_the_fixed_scale_run(torch, case, cache):
    from bayesgm_amd import _lib
    burn, keep, q_sd, seed = 20, 30, 0.4, 4711
    m = _model(23, case["z_dims"], case["p"], case["binary"])
    x, y, v = _data(case["n"], case["p"], 24, case["binary"])
    kw = dict(effect=_lib.EFFECT_ITE) if case["binary"] else dict(effect=_lib.EFFECT_ADRF, x_values=np.linspace(0.0, 2.0, 7))
    kw.update(want_draws=True, chunk=19)
    fresh = _engine(m)
    fresh.set_outcome_cache(cache)
    want = fresh.mh_sample(x, y, v, burn, keep, q_sd, seed, **kw)
    eng = _engine(m)
    eng.set_outcome_cache(cache)
    ones = np.ones(burn, np.float32)
    got = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, row_adapt_table=(ones, ones), **kw)
    after = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, **kw)          # the setter was cleared
    assert bool(torch.all(got["row_scale"] == float(np.float32(q_sd))))
    for k in ("state", "logp", "draws", "acc_count", "ite" if case["binary"] else "adrf"):
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(after[k], want[k]), k
    # an empty table too: nothing is ever multiplied
    none = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, row_adapt_table=(ones[:0], ones[:0]), **kw)
    assert torch.equal(none["draws"], want["draws"]) and bool(torch.all(none["row_scale"] == float(np.float32(q_sd))))


# ---------------------------------------------------------------------------------------------------------------------
# 3. a chain is a function of (seed, global row, its data): row windows and launch segments
# ---------------------------------------------------------------------------------------------------------------------
def test_rows_and_segments_are_independent(torch):
    from bayesgm_amd import _lib
    burn, keep, q_sd, seed = 40, 30, 0.8, 99
    m = _model(31, [1, 1, 1, 7], 200)
    x, y, v = _data(256, 200, 32)
    xs = np.linspace(0.0, 3.0, 5)
    eng = _engine(m)
    full = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, want_draws=True, row_adapt=TARGET)
    part = eng.mh_sample(x[64:128], y[64:128], v[64:128], burn, keep, q_sd, seed, want_draws=True, row_base=64, row_adapt=TARGET)
    assert torch.equal(full["draws"][:, 64:128], part["draws"]) and torch.equal(full["row_scale"][64:128], part["row_scale"])
    assert torch.equal(full["logp"][64:128], part["logp"])
    # ragged window that starts inside a 16-row tile
    part = eng.mh_sample(x[70:101], y[70:101], v[70:101], burn, keep, q_sd, seed, want_draws=True, row_base=70, row_adapt=TARGET)
    assert torch.equal(full["draws"][:, 70:101], part["draws"]) and torch.equal(full["row_scale"][70:101], part["row_scale"])
    # one launch = the same run cut at arbitrary iterations, three of them inside burn-in: the scale travels in scale_dev
    dev = eng.device
    xd, yd, vd = (torch.from_numpy(a).to(dev) for a in (x.reshape(-1), y.reshape(-1), v))
    n, total = 256, burn + keep
    state = torch.empty((n, 10), device=dev)
    logp = torch.empty(n, device=dev)
    acc = torch.zeros(total, device=dev, dtype=torch.int32)
    draws = torch.empty((keep, n, 10), device=dev)
    scale = torch.full((n,), float("nan"), device=dev)
    up, dn = (torch.from_numpy(t).to(dev) for t in _table(burn))
    eng.set_row_scale(scale, up, dn)
    try:
        cuts = [0, 1, 8, 23, 40, 41, 57, total]
        for b, e in zip(cuts[:-1], cuts[1:]):
            eng.mh_run(xd, yd, vd, state, logp, b, e - b, burn, q_sd, seed, init=(b == 0), acc_count=acc, draws=draws, n_keep=keep)
            if e == 23:
                mid = scale.clone()
    finally:
        eng.set_row_scale(None)
    assert torch.equal(draws, full["draws"]) and torch.equal(scale, full["row_scale"]) and torch.equal(acc, full["acc_count"])
    assert not torch.equal(mid, scale) and bool(torch.isfinite(mid).all())          # it was still adapting at iteration 23
    # segments with an effect: chunks of the whole sampler, ADRF sums included
    one = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, effect=_lib.EFFECT_ADRF, x_values=xs, row_adapt=TARGET)
    cut = eng.mh_sample(x, y, v, burn, keep, q_sd, seed, effect=_lib.EFFECT_ADRF, x_values=xs, row_adapt=TARGET, chunk=13)
    assert torch.equal(one["adrf"], cut["adrf"]) and torch.equal(one["row_scale"], full["row_scale"]) and torch.equal(cut["state"], full["state"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. effects: the outcome-cache modes stay bit-identical, the two likelihood forms agree
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=333),
                                  dict(z_dims=[3, 3, 6, 6], p=100, binary=True, n=130),
                                  dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=50),
                                  dict(z_dims=[1, 1, 1, 7], p=20, binary=True, n=50)])
def test_outcome_cache_modes_are_bit_identical(torch, case):
    from bayesgm_amd import _lib
    burn, keep, seed = 30, 40, 5
    m = _model(41, case["z_dims"], case["p"], case["binary"])
    x, y, v = _data(case["n"], case["p"], 42, case["binary"])
    kw = dict(effect=_lib.EFFECT_ITE) if case["binary"] else dict(effect=_lib.EFFECT_ADRF, x_values=np.linspace(0.0, 3.0, 20))
    key = "ite" if case["binary"] else "adrf"
    outs = {}
    for cache in (True, "wave", False):
        eng = _engine(m)
        eng.set_outcome_cache(cache)
        outs[cache] = eng.mh_sample(x, y, v, burn, keep, 1.0, seed, want_draws=True, row_adapt=TARGET, **kw)
        served, total = eng.outcome_cache_stats()
        print("outcome cache %r: served %d of %d" % (cache, served, total))
    for cache in ("wave", False):
        for k in (key, "draws", "row_scale", "state"):
            assert torch.equal(outs[cache][k], outs[True][k]), (cache, k)
    # the effects are those of the draws (tests/test_gpu_causal.py: <= 2e-4 against the float64 oracle on the same draws)
    ref = OC.infer_from_latent_posterior(OC.cast_model(m, np.float64), outs[True]["draws"].cpu().numpy().astype(np.float64),
                                         None if case["binary"] else np.linspace(0.0, 3.0, 20), True, seed, burn_in=burn)
    got = outs[True][key].cpu().numpy()
    assert np.abs((got.T if case["binary"] else got) - ref).max() <= 2e-4


@pytest.mark.parametrize("case", [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=300),
                                  dict(z_dims=[2, 2, 2, 6], p=150, binary=True, n=130),
                                  dict(z_dims=[1, 1, 1, 7], p=50, binary=False, n=100)])
@pytest.mark.parametrize("cache", [True, "wave"])
def test_gram_and_direct_forms_agree(torch, case, cache):
    from bayesgm_amd import _lib
    from tests.test_gpu_mh_gram_likelihood import _pair, _ref_logp
    m = _model(31, case["z_dims"], case["p"], case["binary"])
    x, y, v = _data(case["n"], case["p"], 32, case["binary"])
    n = case["n"]
    kw = dict(effect=_lib.EFFECT_ITE) if case["binary"] else dict(effect=_lib.EFFECT_ADRF, x_values=np.linspace(0.0, 2.0, 6))
    outs = []
    for eng in _pair(m):
        eng.set_outcome_cache(cache)
        outs.append(eng.mh_sample(x, y, v, 30, 30, 0.3, 987654321, want_draws=True, chunk=23, row_adapt=TARGET, **kw))
    (out_g, out_d) = outs
    sg, sd = out_g["state"].cpu().numpy(), out_d["state"].cpu().numpy()
    same = np.all(np.abs(sg - sd) <= 1e-4, axis=1)
    assert same.mean() >= 0.99, same.mean()
    assert np.array_equal(out_g["row_scale"].cpu().numpy()[same], out_d["row_scale"].cpu().numpy()[same])
    acc_g, acc_d = out_g["acc_count"].cpu().numpy().astype(np.int64), out_d["acc_count"].cpu().numpy().astype(np.int64)
    assert np.abs(acc_g - acc_d).max() <= max(2, n // 50)
    for out, s in ((out_g, sg), (out_d, sd)):
        ref = _ref_logp(m, x, y, v, s)
        err = np.abs(out["logp"].cpu().numpy() - ref)
        assert np.all(err <= 2e-6 * np.abs(ref) + 2e-4), (err.max(), np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------------
# 5. the class surface
# ---------------------------------------------------------------------------------------------------------------------
Z_DIMS, P, N = [3, 3, 3, 1], 50, 128


def _causal(tmp_path, m, seed=3, **kw):
    from bayesgm_amd.models import CausalBGM
    params = dict(dataset="t", output_dir=str(tmp_path), save_res=False, save_model=False, binary_treatment=False, use_bnn=False,
                  z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
                  e_units=[64] * 5, dz_units=[64, 32, 8], kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, **kw)
    for k in ("sigma_v", "sigma_x", "sigma_y"):
        if k in m:
            params[k] = m[k]
    model = CausalBGM(params, random_seed=seed)
    model.set_weights(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
    return model


def test_predict_does_not_depend_on_bs_and_can_be_diagnosed(torch, tmp_path):
    from bayesgm_amd.diagnostics import chain_diagnostics
    m = OC.init_model(0, Z_DIMS, P)
    rs = np.random.RandomState(8)
    n = 512
    v = rs.randn(n, P).astype(np.float32)
    x = rs.exponential(size=(n, 1)).astype(np.float32)
    y = (x + rs.randn(n, 1)).astype(np.float32)
    data = (x, y, v)
    xs = np.linspace(0.0, 3.0, 5)
    kw = dict(alpha=0.05, n_mcmc=200, burn_in=300, x_values=xs, verbose=0, row_adapt=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c = _causal(tmp_path, m), _causal(tmp_path, m), _causal(tmp_path, m)
        eff_a, int_a = a.predict(data, bs=100, diagnose_rows=64, **kw)
        eff_b, int_b = b.predict(data, bs=10000, **kw)
        eff_c, int_c = c.predict(data, bs=10000, **dict(kw, row_adapt=False))
    assert np.array_equal(eff_a, eff_b) and np.array_equal(int_a, int_b)
    assert np.array_equal(a.mh_row_scale_, b.mh_row_scale_) and a.mh_row_scale_.shape == (n,) and a.mh_row_scale_.dtype == np.float32
    assert c.mh_row_scale_ is None and not np.array_equal(eff_c, eff_b)
    assert b.mcmc_diagnostics_ is None and a._seed_counter == b._seed_counter
    print("acceptance: per row %.4f, fixed q_sd = 1 %.4f; scales q05 / median / q95 %.3f / %.3f / %.3f"
          % (b.last_acceptance_rate, c.last_acceptance_rate, *np.quantile(b.mh_row_scale_, [0.05, 0.5, 0.95])))
    # q_sd <= 0 / None no longer means the block-wide rule under row adaptation: the chains start from 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eff_d, _ = _causal(tmp_path, m).predict(data, bs=77, **dict(kw, q_sd=None))
    assert np.array_equal(eff_d, eff_b)
    # the diagnostics are those of the chains predict ran (checked as tests/test_gpu_chain_diag.py does for a fixed scale)
    d = a.mcmc_diagnostics_
    wins = a._diagnose_windows(n, 64)
    assert d.rows.shape == (64,) and np.array_equal(d.rows, np.concatenate([np.arange(s, e) for s, e in wins]))
    seed = (a._base_seed * 1000003 + a._seed_counter) & 0x7FFFFFFFFFFFFFFF
    outs = [a.engine.mh_sample(x[s:e], y[s:e], v[s:e], 300, 200, 1.0, seed, want_draws=True, row_base=s, row_adapt=TARGET) for s, e in wins]
    want = chain_diagnostics(torch.cat([o["draws"] for o in outs], dim=1))
    for k in ("mean", "sd", "rhat", "ess", "mcse", "moves", "flags"):
        assert np.array_equal(getattr(d, k), getattr(want, k), equal_nan=True), k
    assert np.array_equal(np.concatenate([o["row_scale"].cpu().numpy() for o in outs]), a.mh_row_scale_[d.rows])
    # and the sampler method
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s1, s2 = _causal(tmp_path, m), _causal(tmp_path, m)
        d1 = s1.metropolis_hastings_sampler(data, q_sd=None, initial_q_sd=0.7, burn_in=100, n_keep=50, adaptive_sd='row')
        d2 = s2.metropolis_hastings_sampler(data, q_sd=0.7, burn_in=100, n_keep=50, adaptive_sd='row', target_acceptance_rate=0.25)
    assert np.array_equal(d1, d2) and np.array_equal(s1.mh_row_scale_, s2.mh_row_scale_) and s1.mh_row_scale_.shape == (n,)
    ref = a.engine.mh_sample(x, y, v, 100, 50, 0.7, (s1._base_seed * 1000003 + s1._seed_counter) & 0x7FFFFFFFFFFFFFFF, want_draws=True,
                             row_adapt=0.25)
    assert np.array_equal(ref["draws"].cpu().numpy(), d1)


def test_concentrated_panel_reaches_the_target_and_loses_its_stuck_chains(torch, tmp_path):
    """The second CPU panel of tests/test_row_adapt_host.py through predict: 128 rows generated by the model with sigma_v = 0.02,
    sigma_x = sigma_y = 0.1, 1000 + 1000 iterations.  Measured on the CPU restatement: acceptance 0.0013 at the fixed scale 1 with
    a third of the chains never moving, 0.2465 and none with the per-row scale."""
    m = concentrated_model(0, Z_DIMS, P)
    data = concentrated_panel(m, N, 1)
    xs = np.linspace(0.0, 3.0, 5)
    kw = dict(alpha=0.05, n_mcmc=1000, burn_in=1000, x_values=xs, verbose=0, diagnose_rows=N, q_sd=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fixed, adapt = _causal(tmp_path, m, mixing_check=False), _causal(tmp_path, m, mixing_check=False)
        fixed.predict(data, **kw)
        adapt.predict(data, row_adapt=True, **kw)
    sf, sa = fixed.mcmc_diagnostics_.summary(), adapt.mcmc_diagnostics_.summary()
    s = adapt.mh_row_scale_
    print("fixed q_sd = 1: acceptance %.4f, constant series %.3f, ESS median %.1f; per row: acceptance %.4f, constant series %.3f, "
          "ESS median %.1f, scales q05 / median / q95 %.4f / %.4f / %.4f"
          % (fixed.last_acceptance_rate, sf["share_constant"], sf["ess_median"], adapt.last_acceptance_rate, sa["share_constant"],
             sa["ess_median"], *np.quantile(s, [0.05, 0.5, 0.95])))
    assert abs(adapt.last_acceptance_rate - TARGET) <= 0.05, adapt.last_acceptance_rate
    assert sa["share_constant"] == 0.0 and np.all(adapt.mcmc_diagnostics_.moves > 0)
    assert sf["share_constant"] > 0.0
    assert np.all(s > 1e-4) and np.all(s < 1e2)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_paths_refuse(torch):
    from bayesgm_amd import _lib
    from bayesgm_amd.engine import CausalEngine
    from oracle import identifiable as OI
    x, y, v = _data(40, 20, 52)
    m = _model(51, [1, 1, 1, 7], 20)
    run = lambda eng, *d: eng.mh_sample(*(d or (x, y, v)), 10, 10, 0.5, 7, row_adapt=TARGET)
    # split precision
    eng = _engine(m)
    for mode in ("bf16x3", "f16x3"):
        eng.set_precision(mode)
        with pytest.raises(RuntimeError, match=r"\(-?\d+\).*split-precision"):
            run(eng)
    eng.set_precision("fp32")
    assert run(eng)["row_scale"].shape == (40,)          # the refusal cleared the setter and left the handle usable
    assert torch.equal(eng.mh_sample(x, y, v, 10, 10, 0.5, 7, want_draws=True)["draws"], _engine(m).mh_sample(x, y, v, 10, 10, 0.5, 7, want_draws=True)["draws"])
    # conditional latent prior
    rs = np.random.RandomState(33)
    pn = OI.init_prior_net(rs, 5, 10)
    eng.set_prior(torch.from_numpy(rs.randint(0, 5, 40).astype(np.int32)).cuda(), torch.from_numpy(OI.prior_table(pn, 10)).cuda())
    with pytest.raises(RuntimeError, match="conditional latent prior"):
        run(eng)
    eng.set_prior(None, None)
    # hidden widths outside the compiled families: the general-width engine
    mw = _model(53, [1, 1, 1, 7], 20, g_units=(32, 32), f_units=(32, 8), h_units=(32, 8))
    with pytest.raises(RuntimeError, match="general-width engine"):
        run(_engine(mw, g_units=[32, 32], f_units=[32, 8], h_units=[32, 8]))
    # default widths, no LDS-resident shape: the streamed-fragment kernels
    mp = _model(54, [1, 1, 1, 7], 300)
    with pytest.raises(RuntimeError, match="streamed-fragment"):
        run(_engine(mp), *_data(40, 300, 55))
    # block-wide and per-chain adaptation exclude each other; the start scale must be positive
    with pytest.raises(ValueError, match="exclude"):
        eng.mh_sample(x, y, v, 10, 10, None, 7, adaptive=True, row_adapt=TARGET)
    with pytest.raises(ValueError, match="positive"):
        eng.mh_sample(x, y, v, 10, 10, None, 7, row_adapt=TARGET)
    # the setter itself, and the Bayesian-network sampler on a handle that carries a scale
    lib, h = eng.lib, eng.h
    buf = torch.ones(40, device=eng.device)
    assert lib.bgm_causal_set_row_scale(h, C.c_void_p(buf.data_ptr()), None, None, 5, 1e-4, 1e2) != 0 and b"n_table" in lib.bgm_last_error()
    assert lib.bgm_causal_set_row_scale(h, C.c_void_p(buf.data_ptr()), None, None, 0, 0.0, 1e2) != 0 and b"s_min" in lib.bgm_last_error()
    assert lib.bgm_causal_set_row_scale(h, C.c_void_p(buf.data_ptr()), None, None, 0, 1e-4, 1e2) == 0
    try:
        rc = lib.bgm_bnn_mh_run(h, C.byref(_lib.BnnMhArgs()), None)
        assert rc != 0 and b"Bayesian networks" in lib.bgm_last_error()
    finally:
        assert lib.bgm_causal_set_row_scale(h, None, None, None, 0, 0.0, 0.0) == 0
