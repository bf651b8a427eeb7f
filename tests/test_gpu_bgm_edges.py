"""The BGM posterior kernels (bgm_bgm_logpost, bgm_bgm_hmc_run, bgm_bgm_predict_draws; csrc/bgm_kernels.h, csrc/bgm_api.hip)
beyond one pass of their LDS-resident variants and at the edges of bgm_layout (csrc/bgm_state.h), against the float64 NumPy
oracle (oracle/bgm.py).

Part A -- more row tiles (predict: more (tile, draw) work items) than one workgroup per CU x 8 waves holds, so the pass loop
`for (ps = 0; ps < passes; ++ps)` of the resident variants (p = 20: 2 head tiles, p = 100: 7 head tiles) runs a second and a ragged
third pass; the encoder's tile loop (csrc/aux_kernels.hip) at the same row count.
Part B -- 33 rows at the first / last width of each resident shape, their nearest streamed ("wide") neighbours, latent widths 1 and
16, and missing-data patterns that sit on a 16-column tile boundary.

Tolerances are those of tests/test_gpu_bgm.py: log-posterior <= 2e-6*|ref| + 2e-4, gradient <= 2e-5*max|ref| + 2e-5, predictive
draws <= 2e-4, HMC rows <= 5e-4 (fixed step, rows with an accept decision within 5e-3 of its uniform excepted) and <= 2e-3 (adapted
step, 30 transitions).  Every check prints its worst error / bar ratio before it asserts (pytest -s shows them).

Fragile chains (an accept decision with |log u - log_ratio| < 5e-3 in the float64 oracle alone, counted on the CPU): part A 0 of the
24 sampled rows in both cases at 256 CUs.  Part B, per case of EDGE_CASES in order, of 33 chains: 5, 3, 1, 7, 7, 1, 4, 4, 4, 8, 8, 4, 5.
Only the two three-layer cases have a data seed with at most one (5 001 seeds tried per case): a 0.02-step trajectory's energy error is
~1e-4, so a decision is that close whenever its uniform exceeds exp(-5e-3), which 14 % of the chains meet within 30 transitions whatever
the data, the sampler seed being fixed.  What a float32 kernel can flip is a decision within ~1e-5; the recorded seeds keep every
decision at least 6.6e-4 away (the smallest margin per case is 6.6e-4 .. 2.6e-3), and the assertion stays "at most one row".
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bgm as OB  # noqa: E402

W = 8     # restates BGM_WAVES of csrc/bgm_api.hip (waves per workgroup of the resident kernels; ENC_WAVES of aux_kernels.hip is 8 too)


def _model(seed, q, p, n_hidden=5, units=None):
    m = OB.init_model(seed, q, p, g_units=tuple(units) if units else (64,) * n_hidden)
    rs = np.random.RandomState(seed + 7)
    g = m["g"]
    g["bn"].update(gamma=(1 + 0.1 * rs.randn(q)).astype(np.float32), beta=(0.1 * rs.randn(q)).astype(np.float32),
                   mean=(0.2 * rs.randn(q)).astype(np.float32), var=(0.5 + rs.rand(q)).astype(np.float32))
    g["trunk"] = [(W_, (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W_, b in g["trunk"]]
    g["mean"] = (g["mean"][0], (0.1 * rs.randn(p)).astype(np.float32))
    g["var"] = (g["var"][0], (0.1 * rs.randn(p)).astype(np.float32))
    return m


def _data(n, p, seed, miss=0.2):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, p).astype(np.float32)
    x[rs.rand(n, p) < miss] = np.nan
    x[0, :] = np.nan          # a row with nothing observed (prior only)
    if n > 1:
        x[1, :] = rs.randn(p)  # a fully observed row
    return x


def _engine(m):
    from bayesgm_amd.engine import BgmEngine
    eng = BgmEngine(m["x_dim"], m["z_dim"], g_units=[W_.shape[1] for W_, _ in m["g"]["trunk"]])
    eng.set_weights(m["g"])
    return eng


def _n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ref_logpost(m, z, x):
    obs, clean = OB.obs_mask_of(x)
    return OB.log_posterior_and_grad(OB.cast_model(m, np.float64), z.astype(np.float64), clean.astype(np.float64), obs.astype(np.float64))


def _check_logpost(tag, lp, gr, ref_lp, ref_gr, z, prior_rows):
    """The bars of test_bgm_logpost_and_gradient_match_oracle; rows without an observed feature: posterior = prior."""
    r_lp = (np.abs(lp - ref_lp) / (2e-6 * np.abs(ref_lp) + 2e-4)).max()
    r_gr = np.abs(gr - ref_gr).max() / (2e-5 * np.abs(ref_gr).max() + 2e-5)
    r_p0 = max(abs(lp[i] + 0.5 * (z[i] ** 2).sum()) / 1e-5 for i in prior_rows)
    r_p1 = max(np.abs(gr[i] + z[i]).max() / 1e-6 for i in prior_rows)
    print("RATIO %s logpost %.3f gradient %.3f prior-row logpost %.3f prior-row gradient %.3f" % (tag, r_lp, r_gr, r_p0, r_p1))
    assert r_lp <= 1.0, np.abs(lp - ref_lp).max()
    assert r_gr <= 1.0, np.abs(gr - ref_gr).max()
    assert r_p0 < 1.0 and r_p1 <= 1.0, (r_p0, r_p1)


# =============================================================================================================================
# A. Beyond one pass of the resident variants
# =============================================================================================================================
A_CASES = [dict(p=20, nh=5, q=10), dict(p=100, nh=3, q=10)]           # NTX = 2 and NTX = 7
A_IDS = ["p20-h5", "p100-h3"]
A_HMC = dict(burn=4, keep=3, L=3, seed=9, step=0.05)


def _rows_a(n_cus):
    """Two full passes of 16 * W * n_cus rows and a third in which only two tiles exist, the last of them with one row."""
    return 2 * 16 * W * n_cus + 17


@functools.lru_cache(maxsize=None)
def _panel_a(p, nh, q, n_cus):
    """(model, x, z), computed once per case and left unchanged.  _data plus: the last row of the panel all-missing, the first row of
    the last full pass fully observed."""
    n = _rows_a(n_cus)
    m = _model(101, q, p, nh)
    x = _data(n, p, 102)
    rs = np.random.RandomState(103)
    x[n - 1, :] = np.nan
    x[16 * W * n_cus, :] = rs.randn(p)
    z = rs.randn(n, q).astype(np.float32)
    return m, x, z


def _sampled_rows_a(n_cus):
    """24 rows, 8 from each pass; the first row of pass 1 and the last row of the panel among them."""
    per = 16 * W * n_cus
    n = _rows_a(n_cus)
    rs = np.random.RandomState(7)
    a = rs.choice(per, 8, replace=False)
    b = np.r_[per, per + 1 + rs.choice(per - 1, 7, replace=False)]
    c = np.r_[n - 1, 2 * per + rs.choice(16, 7, replace=False)]
    return np.sort(np.concatenate([a, b, c]))


def _oracle_chains_a(m, x, idx, q, burn, keep, L, seed, step):
    """Float64 chains of the rows idx at a fixed step size, as test_bgm_wide_panel_properties builds them: (final states, fragile)."""
    obs, clean = OB.obs_mask_of(x[idx])
    ref, fragile = [], np.zeros(len(idx), bool)
    m64 = OB.cast_model(m, np.float64)
    for k, i in enumerate(idx):
        xk, mk = clean[k:k + 1].astype(np.float64), obs[k:k + 1].astype(np.float64)
        z = OB.hmc_init_state(1, q, seed, int(i)).astype(np.float64)
        lp, gr = OB.log_posterior_and_grad(m64, z, xk, mk)
        for it in range(burn + keep):
            u = OB.R.uniforms(np.array([int(i)]), it, OB.R.TAG_HACC, seed)
            z, lp, gr, lr, _ = OB.hmc_transition(m64, z, xk, mk, step, L, it, seed, int(i), lp, gr)
            fragile[k] |= bool(abs(np.log(u[0]) - lr[0]) < 5e-3)    # accept decision within fp32 rounding of the energy difference
        ref.append(z[0])
    return np.stack(ref), fragile


@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_logpost_beyond_one_pass(case):
    import torch
    n_cus = _n_cus()
    p, q = case["p"], case["q"]
    m, x, z = _panel_a(p, case["nh"], q, n_cus)
    n = len(x)
    assert (n + 15) // 16 > 2 * W * n_cus                # more tiles than two passes of the grid hold
    eng = _engine(m)
    xd, zd = torch.from_numpy(x).cuda(), torch.from_numpy(z).cuda()
    lp_d, gr_d = eng.logpost(zd, xd, want_grad=True)
    lp0_d = eng.logpost(zd, xd)
    assert torch.equal(lp_d, lp0_d)
    for lo, hi in ((0, 64), (n - 64, n)):                # each its own one-pass call
        lp_s, gr_s = eng.logpost(zd[lo:hi].contiguous(), xd[lo:hi].contiguous(), want_grad=True)
        assert torch.equal(lp_s, lp_d[lo:hi]) and torch.equal(gr_s, gr_d[lo:hi]), (lo, hi)
    ref_lp, ref_gr = _ref_logpost(m, z, x)
    _check_logpost("A p=%d" % p, lp_d.cpu().numpy(), gr_d.cpu().numpy(), ref_lp, ref_gr, z, (0, n - 1))


@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_hmc_beyond_one_pass(case):
    import torch
    n_cus = _n_cus()
    p, q = case["p"], case["q"]
    burn, keep, L, seed, step_size = (A_HMC[k] for k in ("burn", "keep", "L", "seed", "step"))
    m, x, _ = _panel_a(p, case["nh"], q, n_cus)
    n, per = len(x), 16 * W * n_cus
    assert (n + 15) // 16 > 2 * W * n_cus
    eng = _engine(m)
    xd = torch.from_numpy(x).cuda()

    def run(lo, hi):
        n_ = hi - lo
        state = torch.empty((n_, q), device="cuda"); logp = torch.empty(n_, device="cuda"); grad = torch.empty((n_, q), device="cuda")
        step = torch.full((1,), step_size, device="cuda")
        acc = torch.zeros(burn + keep, device="cuda", dtype=torch.int32)
        draws = torch.empty((keep, n_, q), device="cuda")
        eng.hmc_run(xd[lo:hi], state, logp, grad, step, 0, burn + keep, burn, L, seed, init=True, row_base=lo, acc_count=acc, draws=draws)
        return state, logp, grad, acc, draws
    s1, l1, g1, a1, d1 = run(0, n)
    # a partition into three runs of one pass each, every run with its own row_base; the first cut lies inside a tile
    cuts = [0, per - 7, 2 * per - 7, n]
    assert cuts[1] % 16 != 0 and all(0 < b - a <= per for a, b in zip(cuts, cuts[1:]))
    acc_sum = torch.zeros_like(a1)
    for lo, hi in zip(cuts, cuts[1:]):
        s, l, g, a, d = run(lo, hi)
        assert torch.equal(s, s1[lo:hi]) and torch.equal(l, l1[lo:hi]) and torch.equal(g, g1[lo:hi]) and torch.equal(d, d1[:, lo:hi]), (lo, hi)
        acc_sum += a
    assert torch.equal(a1, acc_sum)
    idx = _sampled_rows_a(n_cus)
    assert len(idx) == 24 and per in idx and n - 1 in idx and [int(((idx >= k * per) & (idx < (k + 1) * per)).sum()) for k in range(3)] == [8, 8, 8]
    ref, fragile = _oracle_chains_a(m, x, idx, q, burn, keep, L, seed, step_size)
    ok = ~fragile
    assert ok.sum() >= 20, fragile
    err = np.abs(s1.cpu().numpy()[idx][ok] - ref[ok]).max(axis=1)
    print("RATIO A p=%d HMC rows %.3f (fragile %d of 24)" % (p, err.max() / 5e-4, int(fragile.sum())))
    assert err.max() <= 5e-4, err


@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_predict_beyond_one_pass(case):
    """predict_draws exposes row_base, so the split into two one-pass calls is part of the test."""
    import torch
    n_cus = _n_cus()
    p, q, d = case["p"], case["q"], 6
    n = 16 * (W * n_cus // d + 3) + 5
    assert (n + 15) // 16 * d > W * n_cus                # more (tile, draw) work items than one pass of the grid holds
    m = _model(131, q, p, case["nh"])
    rs = np.random.RandomState(132)
    draws = rs.randn(d, n, q).astype(np.float32)
    eng = _engine(m)
    ref = OB.predict_on_posteriors(OB.cast_model(m, np.float64), draws.astype(np.float64), seed=9, burn_in=13)
    dd = torch.from_numpy(draws).cuda()
    _, full = eng.predict_draws(dd, 13, 9, want_full=True)
    cut = n // 2 + 3
    assert cut % 16 != 0 and all((k + 15) // 16 * d <= W * n_cus for k in (cut, n - cut))
    for lo, hi in ((0, cut), (cut, n)):
        _, part = eng.predict_draws(dd[:, lo:hi].contiguous(), 13, 9, want_full=True, row_base=lo)
        assert torch.equal(part, full[:, lo:hi]), (lo, hi)
    err = np.abs(full.cpu().numpy() - ref).max()
    # compact cells for a ragged missing pattern
    miss = rs.rand(n, p) < 0.1
    slot = np.where(miss, np.cumsum(miss, axis=1) - 1, -1).astype(np.int32)
    k = int(miss.sum(axis=1).max())
    cells, _ = eng.predict_draws(dd, 13, 9, slot=torch.from_numpy(slot).cuda(), k_slots=k)
    cells = cells.cpu().numpy().reshape(n, k, d)
    err_c = 0.0
    for i in list(range(48)) + list(range(n - 48, n)):
        c = np.where(miss[i])[0]
        if len(c):
            err_c = max(err_c, np.abs(cells[i, :len(c)] - ref[:, i, c].T).max())
    print("RATIO A p=%d predict full %.3f cells %.3f" % (p, err / 2e-4, err_c / 2e-4))
    assert err <= 2e-4 and err_c <= 2e-4, (err, err_c)


def test_encoder_beyond_one_pass():
    import torch
    from oracle import causal as OC
    from oracle.nets import mlp_forward
    from bayesgm_amd.engine import CausalEngine
    n_cus = _n_cus()
    z_dims, p = [1, 1, 1, 7], 20
    n = 2 * 16 * 8 * n_cus + 17
    assert (n + 15) // 16 > 2 * 8 * n_cus
    m = OC.init_model(11, z_dims, p)
    rs = np.random.RandomState(110)
    m["e"] = [(W_.astype(np.float32), (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W_, b in m["e"]]   # non-zero biases
    v = rs.randn(n, p).astype(np.float32)
    eng = CausalEngine(p, z_dims)
    eng.set_model(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
    vd = torch.from_numpy(v).cuda()
    got = eng.encode(vd)
    assert torch.equal(eng.encode(vd[n - 64:].contiguous()), got[n - 64:])
    ref = mlp_forward(OC.cast_model(m, np.float64)["e"], v.astype(np.float64))
    got = got.cpu().numpy()
    assert got.shape == ref.shape
    bar = 1e-5 * max(1.0, np.abs(ref).max())
    print("RATIO A encoder %.3f" % (np.abs(got - ref).max() / bar))
    assert np.abs(got - ref).max() <= bar


# =============================================================================================================================
# B. The edges of bgm_layout
# =============================================================================================================================
# bgm_layout: resident when ceil(p / 16) is 2 or 7 (p in 17..32 or 97..112) and the blob fits the LDS, streamed ("wide") otherwise;
# compiled depths 3 and 5, q <= 16.  p = 17 / 32: first / last width of the 2-tile shape; p = 97 / 112: first / last width of the
# 7-tile shape (at 32 and 112 the c < p mask is never false); p = 16, 33, 96, 113: their nearest neighbours, all wide; p = 20 / 100
# with q = 1 and q = 16 (every f < q mask true): resident.  xseed: the data seed of the HMC check -- of 12 (the
# existing test's) and 1000..1299 the one with the fewest chains whose accept decision lies within 5e-3 of its uniform in the float64
# oracle, no decision closer than 5e-4 (12 is kept where it meets the latter); the two three-layer cases: the first seed of 1000.. with
# at most one such chain.  Counts, and why the other cases cannot reach one: the docstring above.
EDGE_CASES = [
    dict(p=17, q=10, nh=5, resident=True, xseed=1110), dict(p=32, q=10, nh=5, resident=True, xseed=1019),
    dict(p=32, q=10, nh=3, resident=True, xseed=1146), dict(p=97, q=10, nh=5, resident=True, xseed=12),
    dict(p=112, q=10, nh=5, resident=True, xseed=12), dict(p=112, q=16, nh=3, resident=True, xseed=2102),
    dict(p=16, q=10, nh=5, resident=False, xseed=1217), dict(p=33, q=10, nh=5, resident=False, xseed=1009),
    dict(p=96, q=10, nh=5, resident=False, xseed=1191), dict(p=113, q=10, nh=5, resident=False, xseed=12),
    dict(p=20, q=1, nh=5, resident=True, xseed=12), dict(p=20, q=16, nh=5, resident=True, xseed=1065),
    dict(p=100, q=16, nh=5, resident=True, xseed=12),
]
EDGE_IDS = ["p%d-q%d-h%d" % (c["p"], c["q"], c["nh"]) for c in EDGE_CASES]
EDGE_HMC = dict(burn=20, keep=10, L=4, step=0.02, seed=77)


def _edge_panel(p, seed):
    """33 rows (two tiles and one ragged row): _data and four rows whose missing pattern sits on a tile boundary."""
    x = _data(29, p, seed)
    rs = np.random.RandomState(seed + 1)
    extra = rs.randn(4, p).astype(np.float32)
    c0 = 16 * ((p + 15) // 16 - 1)                       # first column of the last 16-wide tile
    keep = np.zeros((4, p), bool)
    keep[0, p - 1] = True                                # only column p - 1 observed
    keep[1, 0] = True                                    # only column 0 observed
    keep[2, :c0] = True                                  # exactly the columns of the last tile missing
    keep[3, c0] = True                                   # exactly the first column of the last tile observed
    extra[~keep] = np.nan
    return np.concatenate([x, extra])


def _prior_rows(x):
    return [i for i in range(len(x)) if np.isnan(x[i]).all()]


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_edge_logpost_and_gradient_match_oracle(case):
    p, q = case["p"], case["q"]
    m = _model(1, q, p, case["nh"])
    x = _edge_panel(p, 2)
    assert x.shape == (33, p) and 0 in _prior_rows(x)
    z = np.random.RandomState(3).randn(33, q).astype(np.float32)
    eng = _engine(m)
    lp, gr = eng.logpost(z, x, want_grad=True)
    lp0 = eng.logpost(z, x)
    lp, gr, lp0 = lp.cpu().numpy(), gr.cpu().numpy(), lp0.cpu().numpy()
    assert np.array_equal(lp, lp0)
    ref_lp, ref_gr = _ref_logpost(m, z, x)
    _check_logpost("B p=%d q=%d h=%d" % (p, q, case["nh"]), lp, gr, ref_lp, ref_gr, z, _prior_rows(x))


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_edge_hmc_chain_and_step_adaptation_match_oracle(case):
    p, q = case["p"], case["q"]
    burn, keep, L, step, seed = (EDGE_HMC[k] for k in ("burn", "keep", "L", "step", "seed"))
    m = _model(11, q, p, case["nh"])
    x = _edge_panel(p, case["xseed"])
    eng = _engine(m)
    out = eng.hmc_sample(x, keep, burn, step_size=step, n_leapfrog=L, seed=seed)
    obs, clean = OB.obs_mask_of(x)
    ref, info = OB.hmc_sampler(OB.cast_model(m, np.float64), clean.astype(np.float64), obs.astype(np.float64), keep, burn, step, L, seed,
                               return_info=True)
    draws = out["draws"].cpu().numpy()
    assert draws.shape == ref.shape
    err = np.abs(draws[-1] - ref[-1]).max(axis=1)
    print("RATIO B p=%d q=%d h=%d HMC rows %.3f (second worst %.3f)" % (p, q, case["nh"], err.max() / 2e-3, np.sort(err)[-2] / 2e-3))
    assert (err > 2e-3).sum() <= 1, err                  # at most one chain of the 33 may leave the oracle's
    assert abs(float(out["step"].item()) / info["step"] - 1) < 1e-5      # same *1.01 / /1.01 schedule


@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_edge_predictive_draws_match_oracle(case):
    import torch
    p, q = case["p"], case["q"]
    m = _model(31, q, p, case["nh"])
    draws = np.random.RandomState(32).randn(6, 33, q).astype(np.float32)
    eng = _engine(m)
    ref = OB.predict_on_posteriors(OB.cast_model(m, np.float64), draws.astype(np.float64), seed=9, burn_in=13)
    _, full = eng.predict_draws(torch.from_numpy(draws).cuda(), 13, 9, want_full=True)
    err = np.abs(full.cpu().numpy() - ref).max()
    print("RATIO B p=%d q=%d h=%d predict %.3f" % (p, q, case["nh"], err / 2e-4))
    assert err <= 2e-4


@pytest.mark.parametrize("case", [c for c in EDGE_CASES if c["resident"]], ids=[i for i, c in zip(EDGE_IDS, EDGE_CASES) if c["resident"]])
def test_edge_resident_agrees_with_wide(case, monkeypatch):
    p, q = case["p"], case["q"]
    m = _model(1, q, p, case["nh"])
    x = _edge_panel(p, 2)
    z = np.random.RandomState(3).randn(33, q).astype(np.float32)
    lp_r, gr_r = _engine(m).logpost(z, x, want_grad=True)
    monkeypatch.setenv("BGM_FORCE_WIDE", "1")
    lp_w, gr_w = _engine(m).logpost(z, x, want_grad=True)
    e_lp, e_gr = (lp_r - lp_w).abs().max().item(), (gr_r - gr_w).abs().max().item()
    print("RATIO B p=%d q=%d h=%d resident-wide logpost %.3f gradient %.3f" % (p, q, case["nh"], e_lp / 1e-4, e_gr / 1e-4))
    assert e_lp <= 1e-4 and e_gr <= 1e-4


def test_latent_width_outside_the_compiled_table_is_served():
    """q = 17 needs two 16-wide latent tiles; the blob kernels are compiled for one.  gxb_wanted (csrc/gx_bgm_api.hip) sends z_dim > 16
    to the general-width engine, so the shape is served -- to the bars tests/test_gpu_widths.py sets for that engine."""
    q, p, n = 17, 20, 33
    m = _model(1, q, p, 5)
    x = _edge_panel(p, 2)
    z = np.random.RandomState(3).randn(n, q).astype(np.float32)
    eng = _engine(m)
    lp, gr = eng.logpost(z, x, want_grad=True)
    lp0 = eng.logpost(z, x)
    lp, gr, lp0 = lp.cpu().numpy(), gr.cpu().numpy(), lp0.cpu().numpy()
    assert np.abs(lp - lp0).max() <= 1e-5 * np.abs(lp).max()
    ref_lp, ref_gr = _ref_logpost(m, z, x)
    _check_logpost("B q=17 (general-width engine)", lp, gr, ref_lp, ref_gr, z, _prior_rows(x))
