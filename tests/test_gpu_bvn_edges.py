"""The Bayesian BGM kernels behind the bgm_bvn_* entry points (csrc/bgmb_api.hip + bgmb_kernels.h, bgmf_api.hip + bgmf_kernels.h,
gx_flipout.h) at their routing and shape edges, against oracle/bgm_bnn.py in float64 with the same Philox streams.  Almost everything
that decides which code runs here is a run-time value computed on the host; tests/_bvn_edges_ref.py restates those plans and holds the
cases, tests/test_bvn_edges_host.py shows what each case reaches and the conditions on its inputs.

A: the routes of bgm_bvn_hmc_run.  33 rows, row_base 7, three leapfrog steps at a fixed step: the bootstrap and 2 transitions, then 3 more
   from the stored state with draws kept.  The four fp32 instantiations of bgmf_hmc_kernel with frozen and fresh noise; one predicate of
   bgmf_session off the chains each (q = 33, four hidden layers, a width of 63, a width of 65, the first p its LDS declines); the LDS tiles
   alone (padded widths, two head chunks of 192 + 128 columns at one workgroup per CU, T = 1, six hidden layers, the largest trunk that
   fits); the workspace kernel with frozen noise for what the tiles cannot hold ((257,), (256,) * 5, (512,)) and with fresh noise on widths
   that are no multiple of 64.  Every default run is bit-identical to the run with its planned route forced (BGM_BVN_NO_CHAINS per
   session; BGM_BVN_NO_TILES in one child process).
B: row counts.  bgm_bvn_logpost with gradient and the frozen workspace kernel (child process) at the panels that give tiles of 16, 32, 48
   and 64 rows, each with a last tile of one row, and at two full trips of every workgroup and a ragged third; the LDS tiles at two trips
   and a ragged third; sampled tiles meet the oracle and are bit-identical to the same rows launched alone.  bgm_bvn_decode at tiles of
   64, 64 and 2 rows inside a draw and more than two trips of its grid.
C: minibatch steps at 2, 65 and 4096 rows, a global batch of three times the local one, and the refusals.

Bars (those of tests/test_gpu_bgm_bnn.py, relative to max |ref| as its _rel): log posterior 1e-5, gradient 1e-4, decode 2e-5, step
gradients 2e-4, chain states 1e-3 absolute -- on EVERY row the oracle does not flag (a row is flagged when an accept decision lies
within 2 (1e-5 max|lp| + 1e-3) of its uniform, the rule of _gx_edges_ref.fragile_rows); accepted counts per transition within the number
of flagged rows.  Every check prints a BVN-EDGE line (pytest -s) with its worst error / bar ratio before it asserts.

Flagged rows (of 33) by case, from the oracle alone: chains q16 2 / 1 (frozen / fresh), q17 2 / 1, q1 0 / 0, q32 0 / 0; off-q33 1, off-nh4 2,
off-w63 1, off-w65 1, lds-last-p896 2, lds-first-p897 1; tiles 24-40 1, 130 1, 16 0, 32x6 0, 256x3 1; workspace frozen 1, 1, 1; fresh 0, 0.
Row-count panels at 256 compute units (sampled rows): rt16 0 of 33, rt32 1 of 65, rt48 0 of 97, rt64 0 of 129, trips 2 of 385, tile trips 3 of 193.
Measured on an MI355X (256 compute units): 41 tests in 9.3 s, the two child processes included; worst ratios chains 0.002, log posterior
0.012, gradient 0.001, decode 0.015, step gradients 0.357 (4096 rows); every accepted count equal to the oracle's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import bgm_bnn as OV
from oracle import bnn as OB
import _bvn_edges_ref as V
import _bvn_edges_helper as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_LP, BAR_GRAD, BAR_DECODE, BAR_STEP, BAR_STATE = 1e-5, 1e-4, 2e-5, 2e-4, 1e-3
f64 = lambda a: np.asarray(a, np.float64)


def _note(part, name, what, err, bar, extra=""):
    print("BVN-EDGE part=%s case=%s %s err=%.3e bar=%.3e ratio=%.3f%s" % (part, name, what, err, bar, err / bar, extra))


def _rel(part, name, what, got, ref, bar):
    """The file's relative error: max |got - ref| / max |ref|; printed, then asserted."""
    e = float(np.abs(f64(got) - f64(ref)).max() / (np.abs(ref).max() + 1e-30))
    _note(part, name, what, e, bar)
    assert e <= bar, (what, e, int(np.abs(f64(got) - f64(ref)).argmax()))


def _same(a, b, keys=H.CHAIN_KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _check_chain(part, name, got, r, rows_missing=()):
    """A run against chains64 `r` of the same rows: states and kept draws of every unflagged row, accepted counts per transition."""
    ok = ~r.flagged
    e = np.abs(got["state"][ok] - r.state[ok]).max()
    if got["draws"].size:
        e = max(e, np.abs(got["draws"][:, ok] - r.draws[:, ok]).max())
    _note(part, name, "chain", e, BAR_STATE, " flagged=%d accepted=%s oracle=%s" % (r.flagged.sum(), got["acc"].tolist(), r.acc.sum(axis=1).tolist()))
    assert e <= BAR_STATE
    assert np.abs(got["acc"] - r.acc.sum(axis=1)).max() <= r.flagged.sum()
    for i in rows_missing:          # no observed cell: the stored log posterior and gradient are the prior's at the stored state
        z = f64(got["state"][i])
        assert abs(got["logp"][i] + 0.5 * (z ** 2).sum()) <= BAR_LP * r.lp_max and np.abs(got["grad"][i] + z).max() <= BAR_GRAD * np.abs(r.grad).max()


@pytest.fixture(scope="module")
def cus():
    return H.n_cus()


def _child(tmp_path_factory, job):
    """The helper as a child process with the workspace kernel forced for frozen noise; one child at a time."""
    out = str(tmp_path_factory.mktemp("bvn_edges") / ("forced_%s.npz" % job))
    env = dict(os.environ, BGM_BVN_NO_TILES="1")
    env.pop("BGM_BVN_NO_CHAINS", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_bvn_edges_helper.py"), out, job], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


@pytest.fixture(scope="module")
def forced_a(tmp_path_factory):
    return _child(tmp_path_factory, "A")


@pytest.fixture(scope="module")
def forced_b(tmp_path_factory):
    return _child(tmp_path_factory, "B")


# ---------------------------------------------------------------------------------------------------------------------------
# A: routes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in V.A_CASES])
def test_route_case_follows_oracle_and_equals_its_forced_route(name, monkeypatch, forced_a):
    assert "BGM_BVN_NO_TILES" not in os.environ          # (read once per process: it would take every frozen case off its route)
    c = V.A_BY_NAME[name]
    r = V.ref_chain(name)
    want = V.route(c["q"], c["units"], c["p"], c["frozen"])
    assert want == c["want"] and r.flagged.sum() <= V.CAP_A * c["n"]
    monkeypatch.delenv("BGM_BVN_NO_CHAINS", raising=False)
    got = H.run_case(c)
    _check_chain("A", name, got, r, rows_missing=(V.ROW_MISSING,))
    monkeypatch.setenv("BGM_BVN_NO_CHAINS", "1")
    other = H.run_case(c)          # chains: the route below them; tiles / workspace: the planned route, the chains refused by name
    _check_chain("A", name + "/no-chains", other, r, rows_missing=(V.ROW_MISSING,))
    if want == "chains":
        print("BVN-EDGE part=A case=%s route=chains; %s forced: %s" % (name, V.route(c["q"], c["units"], c["p"], c["frozen"], no_chains=True),
                                                                        "identical" if _same(got, other) else "differs"))
    else:
        assert _same(got, other), "the default run is not the %s route" % want
    if c["frozen"]:
        ws = {k: forced_a["%s/%s" % (name, k)] for k in H.CHAIN_KEYS}
        _check_chain("A", name + "/no-tiles", ws, r, rows_missing=(V.ROW_MISSING,))
        if want == "workspace":
            assert _same(got, ws), "the default run is not the workspace route"
        else:
            print("BVN-EDGE part=A case=%s route=%s; workspace forced: %s" % (name, want, "identical" if _same(got, ws) else "differs"))


# ---------------------------------------------------------------------------------------------------------------------------
# B: row counts
# ---------------------------------------------------------------------------------------------------------------------------
def _small_panel(n, eng):
    x = V.panel(n, V.SMALL["p"], 31)
    return x, torch.from_numpy(np.array(x)).to(eng.device)


def _b_state(n):
    return np.random.RandomState(32).standard_normal((n, V.SMALL["q"])).astype(np.float32)


@pytest.mark.parametrize("name", ["rt16", "rt32", "rt48", "rt64", "trips"])
def test_logpost_row_counts(name, cus):
    n, rt, grid = H.b_panels(cus)[name]
    assert name == "trips" or int(name[2:]) == rt
    assert n % rt == 1 and (name != "trips" or (n + rt - 1) // rt == 2 * grid + 2)
    eng = H.engine(V.SMALL, True)
    try:
        x, xd = _small_panel(n, eng)
        z = _b_state(n)
        zd = torch.from_numpy(z).to(eng.device)
        lp, gr = eng.logpost(zd, xd, V.B_SEED, V.B_STREAM, row_base=V.B_ROW_BASE, want_grad=True)
        tiles = H.b_tiles(name, n, rt, grid)
        for t in tiles:          # the same rows as a launch of their own: bit-identical
            lo, hi = t * rt, min(n, (t + 1) * rt)
            lp_t, gr_t = eng.logpost(zd[lo:hi].contiguous(), xd[lo:hi].contiguous(), V.B_SEED, V.B_STREAM, row_base=V.B_ROW_BASE + lo, want_grad=True)
            assert torch.equal(lp[lo:hi], lp_t) and torch.equal(gr[lo:hi], gr_t), t
        assert torch.equal(eng.logpost(zd, xd, V.B_SEED, V.B_STREAM, row_base=V.B_ROW_BASE), lp)
        rows = np.arange(n) if name != "trips" else V.tile_rows(tiles, rt, n)          # the oracle on sampled tiles of the large panel
        ref_lp, ref_gr, _ = V.logpost_rows(V.case_net(V.SMALL), z, x, rows, V.B_SEED, V.B_STREAM, V.B_ROW_BASE)
        lp, gr = lp.cpu().numpy(), gr.cpu().numpy()
        _rel("B", name, "logpost", lp[rows], ref_lp, BAR_LP)
        _rel("B", name, "grad", gr[rows], ref_gr, BAR_GRAD)
        i = V.ROW_MISSING
        assert abs(lp[i] + 0.5 * (f64(z[i]) ** 2).sum()) <= BAR_LP * np.abs(ref_lp).max() and np.abs(gr[i] + z[i]).max() <= BAR_GRAD * np.abs(ref_gr).max()
        assert np.isfinite(lp).all() and np.isfinite(gr).all()
    finally:
        eng.close()


def _check_rows(part, name, n, rt, tiles, whole, alone):
    """whole: state / logp / grad / acc of the panel's launch; alone: {tile: the same of the tile's own launch}."""
    net = V.case_net(V.SMALL)
    x = V.panel(n, V.SMALL["p"], 31)
    assert np.isfinite(whole["state"]).all() and np.isfinite(whole["logp"]).all()
    rows = V.tile_rows(tiles, rt, n)
    r = V.chains64(net, x, rows, V.B_SEED, V.B_ROW_BASE, V.B_STEP, V.B_LEAP, V.B_ITERS, V.B_ITERS, True)
    assert r.flagged.sum() <= V.CAP_TRIPS * len(rows)
    acc = np.zeros(V.B_ITERS, np.int64)
    for t in tiles:
        lo, hi = t * rt, min(n, (t + 1) * rt)
        for k in ("state", "logp", "grad"):
            assert np.array_equal(whole[k][lo:hi], alone[t][k]), (t, k)
        acc += alone[t]["acc"]
    got = dict(state=whole["state"][rows], logp=whole["logp"][rows], grad=whole["grad"][rows], draws=np.empty(0), acc=acc)
    _check_chain(part, name, got, r, rows_missing=(int(np.where(rows == V.ROW_MISSING)[0][0]),))
    assert 0 < whole["acc"].min() and whole["acc"].max() < n


@pytest.mark.parametrize("name", ["rt16", "rt32", "rt48", "rt64", "trips"])
def test_frozen_workspace_kernel_row_counts(name, cus, forced_b):
    n, rt, grid = H.b_panels(cus)[name]
    tiles = H.b_tiles(name, n, rt, grid)
    whole = {k: forced_b["%s/%s" % (name, k)] for k in ("state", "logp", "grad", "acc")}
    alone = {t: {k: forced_b["%s/%d/%s" % (name, t, k)] for k in ("state", "logp", "grad", "acc")} for t in tiles}
    assert whole["state"].shape == (n, V.SMALL["q"])
    _check_rows("B", "workspace-" + name, n, rt, tiles, whole, alone)


def test_lds_tiles_over_several_trips(cus, monkeypatch):
    monkeypatch.delenv("BGM_BVN_NO_CHAINS", raising=False)
    g = V.gxf_plan(V.SMALL["q"], V.SMALL["units"], V.SMALL["p"])
    assert V.route(V.SMALL["q"], V.SMALL["units"], V.SMALL["p"], True) == "tiles" and "BGM_BVN_NO_TILES" not in os.environ
    n = V.rows_tiles_trips(cus, g.occ)
    grid = V.gxf_grid(n, cus, g.occ)
    assert (n + 31) // 32 == 2 * grid + 2
    tiles = H.b_tiles("tiles-trips", n, V.GX_ROWS, grid)
    eng = H.engine(V.SMALL, True)
    try:
        _, xd = _small_panel(n, eng)
        whole, alone = H.run_rows(eng, xd, tiles, V.GX_ROWS, n)
    finally:
        eng.close()
    _check_rows("B", "tiles-trips", n, V.GX_ROWS, tiles, whole, alone)


def test_decode_tiles_inside_a_draw_and_several_trips(cus):
    from bayesgm_amd.bvn_engine import STREAM_PREDICT
    q, p, n = V.SMALL["q"], V.SMALL["p"], V.D_ROWS
    nd = V.decode_draws(cus)
    tiles, grid = V.decode_grid(n, nd, cus)
    assert tiles == 3 * nd and tiles > 2 * grid
    net64 = OV.cast_vnet(V.case_net(V.SMALL), np.float64)
    post = np.random.RandomState(10).standard_normal((nd, n, q)).astype(np.float32)
    eng = H.engine(V.SMALL, True)
    try:
        slot = -np.ones((n, p), np.int32)
        slot[:, 4], slot[:, 36] = 0, 1
        sl = torch.from_numpy(slot).to(eng.device)
        kw = dict(burn_in=V.D_BURN, row_base=V.D_ROW_BASE)
        cells, full, var = eng.decode(post, V.D_SEED, STREAM_PREDICT + V.D_BLOCK, slot=sl, k_slots=2, want_full=True, want_var=True, **kw)
        ref = OV.predict_on_posteriors(net64, f64(post), V.D_SEED, block=V.D_BLOCK, row0=V.D_ROW_BASE, burn_in=V.D_BURN)
        full_h = full.cpu().numpy()
        _rel("B", "decode", "full", full_h, ref, BAR_DECODE)
        c = cells.cpu().numpy()
        np.testing.assert_array_equal(c[:, 0, :], full_h[:, :, 4].T)
        np.testing.assert_array_equal(c[:, 1, :], full_h[:, :, 36].T)
        ids = (np.arange(nd)[:, None] * n + np.arange(n)[None, :]).reshape(-1)
        m_ref, s2_ref = OV.decode(net64, f64(post).reshape(nd * n, q), V.D_SEED, STREAM_PREDICT + V.D_BLOCK, rows=ids)
        _rel("B", "decode", "var_full", var.cpu().numpy().reshape(nd * n, p), s2_ref, BAR_DECODE)
        _, mean_only = eng.decode(post, V.D_SEED, STREAM_PREDICT + V.D_BLOCK, want_full=True, add_noise=False, **kw)
        _rel("B", "decode", "mean", mean_only.cpu().numpy().reshape(nd * n, p), m_ref, BAR_DECODE)
        # a part of a row block: signs keyed d * stride + off + row
        few = post[:3]
        _, part = eng.decode(few, V.D_SEED, STREAM_PREDICT + V.D_BLOCK, want_full=True, sign_stride=1000, sign_off=40, **kw)
        ref_part = OV.predict_on_posteriors(net64, f64(few), V.D_SEED, block=V.D_BLOCK, row0=V.D_ROW_BASE, burn_in=V.D_BURN, bs=1000, off=40)
        _rel("B", "decode", "stride-off", part.cpu().numpy(), ref_part, BAR_DECODE)
        assert not np.array_equal(part.cpu().numpy(), full_h[:3])
        # sign row ids beyond 2^32 are refused by name; the engine stays usable
        assert V.decode_refused(n, 3, 1 << 31, 0)
        with pytest.raises(RuntimeError, match=r"2\^32"):
            eng.decode(few, V.D_SEED, STREAM_PREDICT + V.D_BLOCK, want_full=True, sign_stride=1 << 31, **kw)
        _, again = eng.decode(few, V.D_SEED, STREAM_PREDICT + V.D_BLOCK, want_full=True, sign_stride=1000, sign_off=40, **kw)
        assert torch.equal(again, part)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# C: minibatch steps at the batch edges
# ---------------------------------------------------------------------------------------------------------------------------
def _steps(B, max_batch, batch_global=None, name=None):
    from oracle.fit import adam_lr_t, B1, B2, ADAM_EPS
    name = name or "B%d" % B
    q, p, klw, lr_z = V.SMALL["q"], V.SMALL["p"], 0.01, 5e-3
    bg = batch_global or B
    rs = np.random.RandomState(1)
    N = B + 20
    z = rs.standard_normal((N, q)).astype(np.float32)
    x = rs.standard_normal((N, p)).astype(np.float32)
    idx = rs.choice(N, B, replace=False).astype(np.int32)
    eng = H.engine(V.SMALL, False, kl_weight=klw, max_batch=max_batch)
    try:
        dev = eng.device
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        xd, zd, idd = T(x), T(z), T(idx)
        seed, stream = (3 << 32) | 17, 6
        out = torch.zeros(2, device=dev)
        eng.theta_step(xd, zd, idd, 1e-3, seed, stream, batch_global=batch_global, apply=False, out=out)
        got = f64(eng.read(1))
        n64 = OV.cast_vnet(V.case_net(V.SMALL), np.float64)
        zb, xb = f64(z[idx]), f64(x[idx])
        loss, mse, g, _, c = OV.loss_and_grads(n64, zb, xb, OV.draw(n64, B, seed, stream, dtype=np.float64), inv_B=1.0 / bg)
        klv, gk = OV.vkl(n64)
        w = klw * B / bg          # the ranks' gradients are summed: the KL term counts once
        ref = np.concatenate([f64(a).ravel() for a in OV.flat_grads(OB.add_grads(g, gk, w))])
        _rel("C", name, "theta-grad", got, ref, BAR_STEP)
        o = out.cpu().numpy()
        _note("C", name, "loss", abs(o[0] - (loss + w * klv)), 1e-4 * abs(loss + w * klv) + 1e-4)
        assert abs(o[0] - (loss + w * klv)) <= 1e-4 * abs(loss + w * klv) + 1e-4
        _note("C", name, "mse", abs(o[1] - mse), 1e-4 * mse)
        assert abs(o[1] - mse) <= 1e-4 * mse
        OV.move_stats(n64, c)
        th = eng.read(0)
        np.testing.assert_allclose(th[2 * q:3 * q], n64["mean_mv"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(th[3 * q:4 * q], n64["var_mv"], rtol=1e-5, atol=1e-6)
        # the Z step: gradient of the batch rows through the first Adam step of fresh slots (sign-like: lr_t m / (sqrt(v) + eps))
        out_z = torch.zeros(1, device=dev)
        eng.z_step(xd, zd, idd, lr_z, seed, stream + 1, batch_global=batch_global, out=out_z)
        lz, _, _, dz, c2 = OV.loss_and_grads(n64, zb, xb, OV.draw(n64, B, seed, stream + 1, dtype=np.float64), inv_B=1.0 / bg)
        dz = dz + zb / bg
        post = lz + (zb ** 2).sum() / 2 / bg
        _note("C", name, "z-loss", abs(out_z.item() - post), 1e-4 * abs(post) + 1e-4)
        assert abs(out_z.item() - post) <= 1e-4 * abs(post) + 1e-4
        lr_t = adam_lr_t(lr_z, 1)
        upd = lambda d: lr_t * (1 - B1) * d / (np.sqrt(1 - B2) * np.abs(d) + ADAM_EPS)
        z_new = zd.cpu().numpy()
        moved = f64(z_new[idx]) - zb
        # a gradient within the step-gradient bar of its reference moves the row by upd(dz +- gbar); float32 keeps z to an ulp of |z| <= 8
        gbar = BAR_STEP * np.abs(dz).max()
        lo_, hi_ = np.minimum(upd(dz - gbar), upd(dz + gbar)), np.maximum(upd(dz - gbar), upd(dz + gbar))
        slack = 2.0 ** -21 + 1e-6 * lr_t
        worst = max(0.0, np.maximum(-hi_ - moved, moved + lo_).max())          # how far outside [-upd(dz + gbar), -upd(dz - gbar)]
        _note("C", name, "z-update", worst, slack, " decided=%d of %d" % ((np.abs(dz) > gbar).sum(), dz.size))
        assert worst <= slack
        assert (np.abs(dz) > gbar).mean() > 0.9
        rest = np.setdiff1d(np.arange(N), idx)
        np.testing.assert_array_equal(z_new[rest], z[rest])
        OV.move_stats(n64, c2)
        th = eng.read(0)
        np.testing.assert_allclose(th[2 * q:3 * q], n64["mean_mv"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(th[3 * q:4 * q], n64["var_mv"], rtol=1e-5, atol=1e-6)
    finally:
        eng.close()


@pytest.mark.parametrize("B", V.C_BATCHES)
def test_minibatch_steps_at_the_batch_edges(B):
    _steps(B, max(32, B))


def test_minibatch_steps_of_a_rank_of_three():
    _steps(65, 65, batch_global=3 * 65, name="B65-of-195")


def test_batch_refusals_leave_the_session_usable():
    from bayesgm_amd.bvn_engine import BvnEngine
    q, p = V.SMALL["q"], V.SMALL["p"]
    eng = BvnEngine(p, q, g_units=V.SMALL["units"], max_batch=V.MAX_BATCH + 1)
    with pytest.raises(RuntimeError, match=r"max_batch must be in \[2, 4096\]"):
        eng.begin(V.case_net(V.SMALL))
    eng.close()
    eng = H.engine(V.SMALL, False, max_batch=64)
    try:
        dev = eng.device
        x, z = torch.zeros((40, p), device=dev), torch.zeros((40, q), device=dev)
        for who, step in (("bgm_bvn_theta_step", eng.theta_step), ("bgm_bvn_z_step", eng.z_step)):
            with pytest.raises(RuntimeError, match=who + ": bad argument"):
                step(x, z, torch.zeros(1, dtype=torch.int32, device=dev), 1e-3, 1, 0)          # a batch of one row
            with pytest.raises(RuntimeError, match=who + ": bad argument"):
                step(x, z, torch.zeros(65, dtype=torch.int32, device=dev), 1e-3, 1, 0)         # above max_batch
        before = eng.read(0)
        out = torch.zeros(2, device=dev)
        eng.theta_step(x, z, torch.arange(2, dtype=torch.int32, device=dev), 1e-3, 1, 0, apply=False, out=out)
        assert np.isfinite(out.cpu().numpy()).all() and np.isfinite(eng.read(1)).all()
        np.testing.assert_array_equal(eng.read(0)[4 * q:], before[4 * q:])
    finally:
        eng.close()
