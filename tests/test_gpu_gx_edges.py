"""The general-width engine (csrc/gx_api.hip, gx_device.h, gx_causal_kernels.h, gw_kernels.h, gx_fit_kernels.h) where its run-time
choices change: against the float64 NumPy oracle (oracle/causal.py, oracle/fit.py, oracle/nets.py) through CausalEngine, at the bars of
tests/test_gpu_widths.py (log posterior 1e-5 |ref| + 1e-3, ADRF 2e-4, ITE and stand-alone effects 5e-4, evaluate sums 1e-4 relative,
evaluate dose response 2e-4, fit gradients 5e-5 max|ref| + 1e-7 per net).  Every check prints its worst error / bar ratio before it
asserts (pytest -s shows them).

Part A -- the 32-row workgroup kernels (gx_causal_logpost_kernel, gx_causal_mh_kernel<0|1|2>, gx_causal_effects_kernel<1|2>,
gx_causal_eval_kernel, gx_encode_kernel) on small models past the row-tile-per-wave boundary: one hidden layer of 160, widths that are no
multiple of 32 beside narrow f / h (two of the four waves own no unit of an N = 32 layer), an outcome net that alone forces the path,
BGM_MAX_LAYERS hidden layers of g; continuous and binary treatment; p = 31 / 32 / 77, sum(z_dims) = 4 / 16 / 17, n = 1 / 31 / 32 / 33 /
65.  And r_test / mixed / w128 of test_gpu_widths.py through BOTH families (BGM_NO_GW=1 in a subprocess: the switch is read once per
process).
Part B -- BGM_GX_OCC=1 / BGM_GW_OCC=1 (one workgroup per CU) and panels of two full trips of the persistent tile loops plus a ragged
third: per-slot ADRF partials across trips, the per-slot outcome cache re-armed per tile, chain state reloaded by chunked calls, the
encoder's tile loop.
Part C -- the plan's boundaries: gw / workgroup at sum(z_dims) = 59 / 60 of a 128-wide model and at width 129; hidden width 576 (the
widest the 160 KB of LDS admit at sum(z_dims) = 10, p = 20) served, 577 refused by every entry point; forced dose batches 1..4 at dose
counts 1, 5, 9; z_dims with z0 + z2 = 0 refused by bgm_causal_configure.
Part D -- gx_causal_fit_kernel / fit_dw_kernel with minibatches of 256, 257 and 300 rows (two 256-row slices, the second ragged), then 17
rows in the same session.

Chains: tests/_gx_edges_ref.py fragile_rows runs the float64 chain and flags the rows with an accept decision within
2 (1e-5 max|lp| + 1e-3) of its uniform.  Every unflagged row's last draw equals the oracle's to 1e-4, at least 97 % of all rows do, and
acc_count differs per iteration by at most max(2, mismatching rows).  Flagged rows, counted on the CPU by tests/test_gx_edges_host.py
(cap: 15 % of a panel for chains of up to 35 iterations, 6 % for the 8-iteration multi-trip chains):
part A in the order of A_CASES 0/1, 0/1, 1/33, 3/33, 2/65, 2/33, 3/31, 1/32, 1/32, 1/65, 2/33, 3/31; both-families cases 2/64, 4/45, 4/65;
part C 0/33, 1/33, 0/33 (switch) and 1/33 (width 576); part B at 256 CUs 301 and 299 of 16 421 (workgroup, continuous / binary) and 528
of 32 789 (gw), none of them among the rows of the last two tiles of the workgroup panels, one among the gw panel's."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gx_edges_ref as G  # noqa: E402
from test_gpu_widths import _engine  # noqa: E402

from oracle import causal as OC  # noqa: E402
from oracle import fit as OF      # noqa: E402
from oracle.nets import mlp_forward  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GX_ROWS = 32      # restates GX_ROWS of csrc/gx_device.h
GW_ROWS = 16      # restates GW_ROWS of csrc/gw_kernels.h
GW_WAVES = 4      # restates GW_WAVES of csrc/gw_kernels.h
assert (GX_ROWS, GW_ROWS, GW_WAVES) == (G.GX_ROWS, G.GW_ROWS, G.GW_WAVES)

XS5 = np.linspace(0, 3, 5)
XS7 = np.linspace(0.1, 2.9, 7)


def _n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Ratios(object):
    """Worst error / bar per check: printed when added, asserted together at the end (one failing check does not hide the others)."""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def add(self, name, ratio, note=""):
        ratio = float(ratio)
        print("RATIO %s %s %.3f %s" % (self.tag, name, ratio, note))
        self.rows.append((name, ratio, note))

    def check(self):
        bad = [r for r in self.rows if not r[1] <= 1.0]
        assert not bad, (self.tag, bad)


def _workgroup_path(eng):
    d = eng.describe()
    return "gx_causal_mh_kernel" in d and "gw_causal_mh_kernel" not in d


def _gw_path(eng):
    return "gw_causal_mh_kernel" in eng.describe()


def _effect_kw(binary, xs):
    from bayesgm_amd import _lib
    return dict(effect=_lib.EFFECT_ITE) if binary else dict(effect=_lib.EFFECT_ADRF, x_values=xs)


def _check_logpost(R, eng, m, data, seed=3, name="logpost"):
    x, y, v = data
    z = np.random.RandomState(seed).randn(len(x), sum(m["z_dims"])).astype(np.float32)
    got = eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()
    m64, (x64, y64, v64, z64) = G._as64(m, x, y, v, z)
    ref = OC.log_posterior(m64, x64, y64, v64, z64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    R.add(name, (np.abs(got - ref) / (1e-5 * np.abs(ref) + 1e-3)).max(), "(max |lp| %.0f)" % np.abs(ref).max())
    return got, ref


def _check_chain(R, out, ref_state, flagged, ref_acc, cap, tail=None, name="chain"):
    """The three chain criteria (module docstring) and the condition on the inputs; tail: the rows of the last two tiles, which must
    contain unflagged rows that match."""
    n = len(ref_state)
    last = out["draws"].cpu().numpy()[-1].astype(np.float64)
    assert last.shape == ref_state.shape
    err = np.abs(last - ref_state).max(axis=1)
    row_ok = err <= 1e-4
    assert flagged.sum() <= cap * n, ("input condition: flagged rows", int(flagged.sum()), n)
    R.add(name + " unflagged rows", (err[~flagged].max() if (~flagged).any() else 0.0) / 1e-4, "(%d of %d rows flagged)" % (flagged.sum(), n))
    R.add(name + " share of rows off", (1.0 - row_ok.mean()) / 0.03, "(%d rows off)" % (~row_ok).sum())
    acc = out["acc_count"].cpu().numpy().astype(np.int64)
    assert acc.shape == ref_acc.shape
    R.add(name + " acc_count", np.abs(acc - ref_acc).max() / max(2, int((~row_ok).sum())), "(accepted %d of %d)" % (acc.sum(), n * len(acc)))
    if tail is not None:
        t = np.zeros(n, bool)
        t[tail] = True
        assert (t & ~flagged).any(), "no unflagged row in the last two tiles"
        R.add(name + " last two tiles", err[t & ~flagged].max() / 1e-4, "(%d unflagged rows)" % (t & ~flagged).sum())
    return row_ok


def _check_effects(R, eng, m, x, out, binary, xs, burn, seed, name="effects"):
    """Fused and stand-alone effects against infer_from_latent_posterior on the GPU's own draws."""
    draws = out["draws"].cpu().numpy()
    ref = OC.infer_from_latent_posterior(OC.cast_model(m, np.float64), draws.astype(np.float64), None if binary else xs, True, seed, burn_in=burn)
    if binary:
        R.add(name + " fused ITE", np.abs(out["ite"].cpu().numpy().T - ref).max() / 5e-4)
    else:
        R.add(name + " fused ADRF", np.abs(out["adrf"].cpu().numpy() - ref).max() / 2e-4)
    alone = eng.effects(x, out["draws"], burn, seed, x_values=None if binary else xs, sample_y=True).cpu().numpy()
    assert alone.shape == ref.shape
    R.add(name + " stand-alone", np.abs(alone - ref).max() / 5e-4)
    return ref


def _check_evaluate(R, eng, m, data, binary, xs, seed=33, name="evaluate"):
    import torch
    x, y, v = data
    n, p = v.shape
    z = np.random.RandomState(seed).randn(n, sum(m["z_dims"])).astype(np.float32)
    T = lambda a_: torch.from_numpy(np.ascontiguousarray(a_)).to(eng.device)
    sums, causal = eng.evaluate(T(x.ravel()), T(y.ravel()), T(v), T(z), x_values=None if binary else xs)
    sums = sums.cpu().numpy()
    gv, gx, gy = sums[0] / (n * p), sums[1] / n, sums[2] / n
    causal = causal.cpu().numpy() if binary else causal.cpu().numpy() / n
    m64 = OC.cast_model(m, np.float64)
    z64 = z.astype(np.float64)
    z0d, z1d, z2d, _ = m["z_dims"]
    mv = ((v - mlp_forward(m64["g"], z64)[:, :p]) ** 2).mean()
    h_out = mlp_forward(m64["h"], np.concatenate([z64[:, :z0d], z64[:, z0d + z1d:z0d + z1d + z2d]], axis=1))[:, 0]
    xp = 1.0 / (1.0 + np.exp(-h_out)) if binary else h_out
    mx = ((x[:, 0] - xp) ** 2).mean()
    fy = lambda xv: mlp_forward(m64["f"], np.concatenate([z64[:, :z0d + z1d], xv], axis=1))[:, 0]
    my = ((y[:, 0] - fy(x.astype(np.float64))) ** 2).mean()
    R.add(name + " sums", max(abs(gv - mv) / (1e-4 * mv), abs(gx - mx) / (1e-4 * max(mx, 1e-3)), abs(gy - my) / (1e-4 * my)))
    if binary:
        ref = fy(np.ones((n, 1))) - fy(np.zeros((n, 1)))
    else:
        ref = np.array([fy(np.full((n, 1), t)).mean() for t in xs])
    assert np.asarray(causal).shape == ref.shape
    R.add(name + " dose response" if not binary else name + " ITE", np.abs(np.asarray(causal) - ref).max() / 2e-4)


def _check_encode(R, eng, m, v, name="encode"):
    got = eng.encode(v).cpu().numpy()
    ref = mlp_forward(OC.cast_model(m, np.float64)["e"], v.astype(np.float64))
    assert got.shape == ref.shape
    R.add(name, np.abs(got - ref).max() / (1e-5 * np.abs(ref).max() + 1e-5))


@functools.lru_cache(maxsize=None)
def _oracle_chain(key, n_cus=0):
    """(case, units, model, data, final float64 state, flagged rows, accepted rows per iteration): computed once per case, left unchanged."""
    kind, k = key
    c = {"A": lambda: G.A_CASES[k], "AB": lambda: G.AB_CASES[k], "CS": lambda: G.C_SWITCH[k], "CW": lambda: G.C_WIDE,
         "B": lambda: G.b_case(n_cus, k)}[kind]()
    u, m, data = G.build(c)
    st, fl, acc = G.fragile_rows(m, data, c["burn"] + c["keep"], G.Q_SD, c["seed"])
    return c, u, m, data, st, fl, acc


# =============================================================================================================================
# A. The workgroup kernels at the shapes they can go wrong
# =============================================================================================================================
@pytest.mark.parametrize("k", range(len(G.A_CASES)), ids=[G.case_id(c) for c in G.A_CASES])
def test_workgroup_kernels_match_oracle(k):
    c, u, m, data, ref_state, flagged, ref_acc = _oracle_chain(("A", k))
    x, y, v = data
    binary = c["binary"]
    eng = _engine(m, u)
    assert _workgroup_path(eng), eng.describe()
    R = _Ratios(G.case_id(c))
    _check_logpost(R, eng, m, data)
    out = eng.mh_sample(x, y, v, c["burn"], c["keep"], G.Q_SD, c["seed"], want_draws=True, chunk=11, sample_y=True, **_effect_kw(binary, XS5))
    _check_chain(R, out, ref_state, flagged, ref_acc, G.CAP_35)
    _check_effects(R, eng, m, x, out, binary, XS5, c["burn"], c["seed"])
    _check_evaluate(R, eng, m, data, binary, XS7)
    _check_encode(R, eng, m, v)
    R.check()


def _ab_dump(path):
    """The both-families cases on whichever family this process runs -> npz (called in-process and from the BGM_NO_GW=1 subprocess)."""
    res = {}
    for i, c in enumerate(G.AB_CASES):
        u, m, (x, y, v) = G.build(c)
        eng = _engine(m, u)
        z = np.random.RandomState(3).randn(c["n"], sum(c["z_dims"])).astype(np.float32)
        out = eng.mh_sample(x, y, v, c["burn"], c["keep"], G.Q_SD, c["seed"], want_draws=True, chunk=11, sample_y=True, **_effect_kw(False, XS5))
        res.update({"lp%d" % i: eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy(), "draws%d" % i: out["draws"].cpu().numpy(),
                    "adrf%d" % i: out["adrf"].cpu().numpy(), "acc%d" % i: out["acc_count"].cpu().numpy(), "path%d" % i: eng.describe()})
    np.savez(path, **res)


def test_same_model_through_both_kernel_families(tmp_path):
    """r_test, mixed, w128 with continuous treatment as shipped (row-tile-per-wave kernels) and with BGM_NO_GW=1 (workgroup kernels, K
    blocks of 32 / 64 / 128 and the Normal treatment likelihood): two independent implementations, and each against the oracle."""
    _ab_dump(str(tmp_path / "gw.npz"))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_gx_edges as T; T._ab_dump(sys.argv[1])" % (
        ROOT, os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code, str(tmp_path / "gx.npz")], check=True, env=dict(os.environ, BGM_NO_GW="1"), timeout=600)
    a, b = np.load(str(tmp_path / "gw.npz")), np.load(str(tmp_path / "gx.npz"))
    R = _Ratios("both-families")
    for i, c in enumerate(G.AB_CASES):
        _, _, m, data, ref_state, flagged, ref_acc = _oracle_chain(("AB", i))
        pa, pb = str(a["path%d" % i]), str(b["path%d" % i])
        assert "gw_causal_mh_kernel" in pa, pa
        assert "gx_causal_mh_kernel" in pb and "gw_causal_mh_kernel" not in pb, pb
        assert flagged.sum() <= G.CAP_35 * c["n"]
        x, y, v = data
        z = np.random.RandomState(3).randn(c["n"], sum(c["z_dims"])).astype(np.float32)
        m64, (x64, y64, v64, z64) = G._as64(m, x, y, v, z)
        ref = OC.log_posterior(m64, x64, y64, v64, z64)
        tag = c["shape"]
        for fam, r in (("gw", a), ("gx", b)):
            R.add("%s %s logpost vs oracle" % (tag, fam), (np.abs(r["lp%d" % i] - ref) / (1e-5 * np.abs(ref) + 1e-3)).max())
            err = np.abs(r["draws%d" % i][-1] - ref_state).max(axis=1)
            R.add("%s %s chain vs oracle, unflagged rows" % (tag, fam), err[~flagged].max() / 1e-4, "(%d of %d flagged)" % (flagged.sum(), c["n"]))
        la, lb = a["lp%d" % i], b["lp%d" % i]
        R.add(tag + " logpost gw vs gx", (np.abs(la - lb) / (2e-6 * np.abs(la) + 2e-4)).max())
        da, db = a["draws%d" % i], b["draws%d" % i]
        R.add(tag + " draws gw vs gx, unflagged rows", np.abs(da - db)[:, ~flagged].max() / 1e-4,
              "(bit-identical: %s)" % np.array_equal(da, db))
        R.add(tag + " ADRF gw vs gx", np.abs(a["adrf%d" % i] - b["adrf%d" % i]).max() / 2e-4)
    R.check()


# =============================================================================================================================
# B. A second and a ragged third trip of the persistent tile loops
# =============================================================================================================================
def _engine_b(monkeypatch, c, u, m):
    monkeypatch.setenv("BGM_GX_OCC", "1")      # read when the engine's session is planned: n_cus workgroups
    monkeypatch.setenv("BGM_GW_OCC", "1")
    eng = _engine(m, u)
    assert (_gw_path(eng) if c["family"] == "gw" else _workgroup_path(eng)), eng.describe()
    per_slot = GX_ROWS if c["family"] == "gx" else GW_ROWS * GW_WAVES
    assert eng.mh_slots(c["n"]) == _n_cus() * (1 if c["family"] == "gx" else GW_WAVES)          # one workgroup per CU ...
    assert c["n"] > 2 * per_slot * _n_cus()                                                     # ... and more than two trips of them
    return eng


B_IDS = ["workgroup-cont", "workgroup-bin", "gw-cont"]


@pytest.mark.parametrize("k", range(3), ids=B_IDS)
def test_second_trip_logpost_and_chain(monkeypatch, k):
    c, u, m, data, ref_state, flagged, ref_acc = _oracle_chain(("B", k), _n_cus())
    x, y, v = data
    n, binary = c["n"], c["binary"]
    eng = _engine_b(monkeypatch, c, u, m)
    R = _Ratios("B %s n=%d" % (B_IDS[k], n))
    _check_logpost(R, eng, m, data)
    out = eng.mh_sample(x, y, v, c["burn"], c["keep"], G.Q_SD, c["seed"], want_draws=True, chunk=4, sample_y=True, **_effect_kw(binary, XS5))
    tail = np.arange((n - 1) // c["tile"] * c["tile"] - c["tile"], n)          # the rows of the last two tiles
    _check_chain(R, out, ref_state, flagged, ref_acc, G.CAP_8, tail=tail)
    _check_effects(R, eng, m, x, out, binary, XS5, c["burn"], c["seed"])
    R.check()


@pytest.mark.parametrize("k", [0, 1, 2], ids=B_IDS)
def test_second_trip_outcome_cache_is_bit_identical(monkeypatch, k):
    """q_sd = 1.5: chains stand still often enough that whole tiles are served from the per-slot cache, on tiles of every trip."""
    c, u, m, data, _, _, _ = _oracle_chain(("B", k), _n_cus())
    x, y, v = data
    n, keep = c["n"], 6
    eng = _engine_b(monkeypatch, c, u, m)
    res = {}
    for on in (True, False):
        eng.set_outcome_cache(on)
        eng.outcome_cache_stats(reset=True)
        out = eng.mh_sample(x, y, v, 4, keep, 1.5, 77, want_draws=True, chunk=4, sample_y=True, **_effect_kw(c["binary"], XS5))
        eff = (out["ite"] if c["binary"] else out["adrf"]).cpu().numpy()
        res[on] = (eff, out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy(), eng.outcome_cache_stats())
    eng.set_outcome_cache(True)
    print("B %s served from cache: %d of %d retained tile-iterations" % ((B_IDS[k],) + res[True][3]))
    assert res[True][3][0] > 0 and res[False][3][0] == 0
    assert res[True][3][1] == -(-n // 16) * keep and res[False][3][1] == -(-n // 16) * keep
    for a, b in zip(res[True][:3], res[False][:3]):
        assert np.array_equal(a, b)


def test_second_trip_evaluate(monkeypatch):
    c, u, m, data, _, _, _ = _oracle_chain(("B", 0), _n_cus())
    eng = _engine_b(monkeypatch, c, u, m)
    R = _Ratios("B evaluate n=%d" % c["n"])
    _check_evaluate(R, eng, m, data, False, XS7)
    R.check()


def test_second_trip_encode():
    """gx_encode_kernel runs min(4, 160 KB // lds_enc) workgroups per CU (gx_encode in csrc/gx_api.hip): 4 for r_test at p = 4."""
    u = G.SHAPES["r_test"]
    occ = G.plan(u, [1, 1, 1, 1], 4)["enc_occ"]
    assert occ == 4
    n = G.rows_b_enc(_n_cus(), occ)
    m = G._model(41, [1, 1, 1, 1], 4, False, **u)
    _, _, v = G._data(n, 4, 42)
    R = _Ratios("B encode n=%d" % n)
    _check_encode(R, _engine(m, u), m, v)
    R.check()


# =============================================================================================================================
# C. The plan's boundaries
# =============================================================================================================================
@pytest.mark.parametrize("k", range(3), ids=["w128-q59-gw", "w128-q60-workgroup", "w129-workgroup"])
def test_family_switch(k):
    """4 gw_wave_floats(gw_ld, q, ldf, 1) <= 24 KB: 24 576 B at (128, 128) and sum(z_dims) = 59, 24 704 B at 60; width 129 pads to 160."""
    c, u, m, data, ref_state, flagged, ref_acc = _oracle_chain(("CS", k))
    x, y, v = data
    eng = _engine(m, u)
    assert G.plan(u, c["z_dims"], c["p"])["gw"] == c["gw"]
    assert (_gw_path(eng) if c["gw"] else _workgroup_path(eng)), eng.describe()
    R = _Ratios(G.case_id(c))
    _check_logpost(R, eng, m, data)
    out = eng.mh_sample(x, y, v, c["burn"], c["keep"], G.Q_SD, c["seed"], want_draws=True, chunk=5, sample_y=True, **_effect_kw(False, XS5))
    _check_chain(R, out, ref_state, flagged, ref_acc, G.CAP_35)
    _check_effects(R, eng, m, x, out, False, XS5, c["burn"], c["seed"])
    R.check()


def _fit_grad_check(R, eng, m, arrays, dev_arrays, idx_np, name, grad=None):
    """fit_theta_grad of the minibatch idx_np against OF.*_loss_and_grads at the bars of test_fit_gradients_match_oracle; -> grad tensor."""
    import torch
    x, y, v, z = arrays
    xd, yd, vd, zd = dev_arrays
    B = len(idx_np)
    idx = torch.from_numpy(idx_np).to(eng.device)
    grad = torch.empty(eng.n_params, device=eng.device) if grad is None else grad
    loss = torch.zeros(8, device=eng.device, dtype=torch.float64)
    eng.fit_theta_grad(xd, yd, vd, zd, idx, B, grad, loss)
    m64 = OC.cast_model(m, np.float64)
    bz, bx, by, bv = (a[idx_np].astype(np.float64) for a in (z, x, y, v))
    lv, _, gg, _ = OF.g_loss_and_grads(m64, bz, bv)
    lx, _, gh, _ = OF.h_loss_and_grads(m64, bz, bx)
    ly, _, gf, _ = OF.f_loss_and_grads(m64, bz, bx, by)
    got = grad.cpu().numpy()
    parts = [_flat(gg), _flat(gf), _flat(gh)]
    assert got.size == sum(p_.size for p_ in parts)
    o = 0
    for net, part in zip("gfh", parts):
        R.add("%s d%s" % (name, net), np.abs(got[o:o + part.size] - part).max() / (5e-5 * np.abs(part).max() + 1e-7))
        o += part.size
    l = loss.cpu().numpy()
    R.add(name + " losses", np.abs(np.array([l[0] / B, l[2] / B, l[4] / B]) / np.array([lv, lx, ly]) - 1.0).max() / 5e-5)
    return grad, parts


def _flat(grads):
    return np.concatenate([np.concatenate([dW.ravel(), db.ravel()]) for dW, db in grads])


def test_widest_model_the_lds_admits():
    """Hidden width 576 for every net at sum(z_dims) = 10, p = 20: 154 240 B of the 160 KB (577 pads to 608: 170 624 B)."""
    import torch
    c, u, m, data, ref_state, flagged, ref_acc = _oracle_chain(("CW", 0))
    x, y, v = data
    pl = G.plan(u, c["z_dims"], c["p"])
    assert pl["served"] and pl["lds_bytes"] == 154240 and not pl["gw"]
    eng = _engine(m, u)
    assert _workgroup_path(eng), eng.describe()
    R = _Ratios(G.case_id(c))
    _check_logpost(R, eng, m, data)
    out = eng.mh_sample(x, y, v, c["burn"], c["keep"], G.Q_SD, c["seed"], want_draws=True, chunk=11, sample_y=True, **_effect_kw(False, XS5))
    _check_chain(R, out, ref_state, flagged, ref_acc, G.CAP_35)
    _check_effects(R, eng, m, x, out, False, XS5, c["burn"], c["seed"])
    _check_encode(R, eng, m, v)
    z = np.random.RandomState(9).randn(c["n"], sum(c["z_dims"])).astype(np.float32)
    dev = tuple(torch.from_numpy(a).to(eng.device) for a in (x.ravel(), y.ravel(), v, z))
    eng.fit_begin(c["n"], 20)
    assert "gx_causal_fit_kernel" in eng.describe(20)
    _fit_grad_check(R, eng, m, (x, y, v, z), dev, np.random.RandomState(3).choice(c["n"], 20, replace=False).astype(np.int32), "fit B=20")
    eng.fit_end()
    R.check()


def test_first_model_refused_says_so_at_every_entry_point():
    """Hidden width 577: every entry point answers with the engine's "too wide" error (the plan fails before anything is allocated or
    launched, gx_session), and the process goes on: a 576-wide engine made afterwards works."""
    import torch
    c = dict(G.C_WIDE, shape="w577")
    u, m, (x, y, v) = G.build(c)
    assert not G.plan(u, c["z_dims"], c["p"])["served"]
    eng = _engine(m, u)
    n, q = c["n"], sum(c["z_dims"])
    z = np.random.RandomState(3).randn(n, q).astype(np.float32)
    T = lambda a_: torch.from_numpy(np.ascontiguousarray(a_)).to(eng.device)
    draws = torch.zeros((2, n, q), device=eng.device)
    calls = dict(
        logpost=lambda: eng.logpost(x.ravel(), y.ravel(), v, z),
        mh_sample=lambda: eng.mh_sample(x, y, v, 2, 2, 0.3, 7, want_draws=True, **_effect_kw(False, XS5)),
        effects=lambda: eng.effects(x, draws, 0, 7, x_values=XS5),
        evaluate=lambda: eng.evaluate(T(x.ravel()), T(y.ravel()), T(v), T(z), x_values=XS7),
        encode=lambda: eng.encode(v),
        fit_begin=lambda: eng.fit_begin(n, 20),
    )
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="too wide"):
            call()
        print("refused: %s" % name)
    torch.cuda.synchronize()
    c2, u2, m2, data2, _, _, _ = _oracle_chain(("CW", 0))
    R = _Ratios("576 after the refusal")
    _check_logpost(R, _engine(m2, u2), m2, data2)
    R.check()


@pytest.mark.parametrize("case", [G.C_DOSE, G.C_DOSE_NARROW_F], ids=["w160", "odd"])
def test_forced_dose_batch(monkeypatch, case):
    """BGM_GX_DB = 1 .. 4 at 1, 5 and 9 doses (remainders 1, 2, 1 and a count below the batch).  The override holds where the batch fits
    the LDS: 1 .. 3 on w160 (4 stacks 4 x 32 rows of 200 floats twice: beyond 160 KB, the plan's own choice stays), 1 .. 4 on `odd`
    (f = (8, 4)).  A dose's arithmetic does not depend on what shares its pass."""
    u, m, (x, y, v) = G.build(case)
    burn, keep, seed = 6, 6, case["seed"]
    m64 = OC.cast_model(m, np.float64)
    R = _Ratios("dose batch %s" % case["shape"])
    res = {}
    for db in (1, 2, 3, 4):
        monkeypatch.setenv("BGM_GX_DB", str(db))
        print("BGM_GX_DB=%d: dose batch in effect %d" % (db, G.plan(u, case["z_dims"], case["p"], force_db=db)["db"]))
        eng = _engine(m, u)
        assert _workgroup_path(eng), eng.describe()
        for nd in (1, 5, 9):
            xs = np.linspace(0, 3, nd) if nd > 1 else np.array([1.3])
            for cache in ((False, True) if nd == 9 else (False,)):
                eng.set_outcome_cache(cache)
                out = eng.mh_sample(x, y, v, burn, keep, G.Q_SD, seed, want_draws=True, chunk=5, sample_y=True, **_effect_kw(False, xs))
                res[(db, nd, cache)] = (out["adrf"].cpu().numpy(), out["draws"].cpu().numpy())
            adrf, draws = res[(db, nd, False)]
            ref = OC.infer_from_latent_posterior(m64, draws.astype(np.float64), xs, True, seed, burn_in=burn)
            R.add("db=%d doses=%d fused ADRF" % (db, nd), np.abs(adrf - ref).max() / 2e-4)
            alone = eng.effects(x, draws, burn, seed, x_values=xs, sample_y=True).cpu().numpy()
            R.add("db=%d doses=%d stand-alone" % (db, nd), np.abs(alone - ref).max() / 5e-4)
        assert np.array_equal(res[(db, 9, True)][0], res[(db, 9, False)][0]) and np.array_equal(res[(db, 9, True)][1], res[(db, 9, False)][1])
    for nd in (1, 5, 9):
        for db in (2, 3, 4):
            assert np.array_equal(res[(db, nd, False)][1], res[(1, nd, False)][1])          # the chains do not know the dose batch
            d = np.abs(res[(db, nd, False)][0] - res[(1, nd, False)][0]).max()
            R.add("doses=%d ADRF db=%d vs db=1" % (nd, db), d / 1e-6, "(bit-identical: %s)" % (d == 0.0))
    R.check()


def test_treatment_net_without_input_is_refused():
    """z_dims with z0 + z2 = 0 would give h a zero-wide input (K = 0 in gx_dense_ld, whose pipeline always contracts one K block):
    bgm_causal_configure refuses it by name, nothing is launched."""
    from bayesgm_amd.engine import CausalEngine
    for units in (G.SHAPES["w160"], {}):
        with pytest.raises(RuntimeError, match=r"z_dims\[0\] \+ z_dims\[2\]"):
            CausalEngine(20, [0, 2, 0, 3], **{k_: list(v_) for k_, v_ in units.items()})
    CausalEngine(20, [0, 2, 1, 3], g_units=[160], f_units=[160], h_units=[160], e_units=[160])          # (one of them alone may be empty)


# =============================================================================================================================
# D. Fit minibatches of more than one 256-row slice of fit_dw_kernel
# =============================================================================================================================
D_CASES = [dict(shape="mixed", binary=False, p=77, z_dims=[2, 3, 4, 5]), dict(shape="w160", binary=True, p=37, z_dims=[1, 1, 1, 7])]


@pytest.mark.parametrize("case", D_CASES, ids=["mixed-cont", "w160-bin"])
def test_fit_slices(case):
    import torch
    n, cap = 700, 300
    u = G.SHAPES[case["shape"]]
    m = G._model(7, case["z_dims"], case["p"], case["binary"], **u)
    x, y, v = G._data(n, case["p"], 8, case["binary"])
    z = np.random.RandomState(9).randn(n, sum(case["z_dims"])).astype(np.float32)
    eng = _engine(m, u)
    dev = eng.device
    xd, yd, vd, zd = (torch.from_numpy(a).to(dev) for a in (x.ravel(), y.ravel(), v, z))
    R = _Ratios("fit %s" % case["shape"])
    eng.fit_begin(n, cap)
    assert "gx_causal_fit_kernel" in eng.describe(cap)
    rs = np.random.RandomState(3)
    for B in (256, 257, 300):
        idx_np = rs.choice(n, B, replace=False).astype(np.int32)
        g1, _ = _fit_grad_check(R, eng, m, (x, y, v, z), (xd, yd, vd, zd), idx_np, "B=%d" % B)
        g2 = torch.empty_like(g1)
        eng.fit_theta_grad(xd, yd, vd, zd, torch.from_numpy(idx_np).to(dev), B, g2)
        assert torch.equal(g1, g2), "B=%d: a second call with the same minibatch differs" % B
    idx17 = rs.choice(n, 17, replace=False).astype(np.int32)
    g_same, parts = _fit_grad_check(R, eng, m, (x, y, v, z), (xd, yd, vd, zd), idx17, "B=17 after 300")
    # the latent step at 300 rows: the gradient through the update of a fresh Adam state (test_theta_gradients_and_z_gradient_match_oracle)
    idx_np = rs.choice(n, cap, replace=False).astype(np.int32)
    idx = torch.from_numpy(idx_np).to(dev)
    zm = torch.zeros_like(zd); zv = torch.zeros_like(zd)
    z_before = zd.clone()
    loss = torch.zeros(8, device=dev, dtype=torch.float64)
    eng.fit_z_step(xd, yd, vd, zd, zm, zv, idx, cap, 1e-3, lazy=True, loss=loss)
    bz, bx, by, bv = (a[idx_np].astype(np.float64) for a in (z, x, y, v))
    lz_ref, dz_ref = OF.z_loss_and_grad(OC.cast_model(m, np.float64), bz, bx, by, bv)
    R.add("z step B=300 loss", abs(loss.cpu().numpy()[6] / cap / lz_ref - 1.0) / 5e-5)
    R.add("z step B=300 gradient", np.abs(zm.cpu().numpy()[idx_np] / 0.1 - dz_ref).max() / (5e-5 * np.abs(dz_ref).max() + 1e-8))
    untouched = np.setdiff1d(np.arange(n), idx_np)
    assert torch.equal(zd[untouched], z_before[untouched])
    eng.fit_end()
    # a fresh session at 17 rows: no row of the 300-row minibatches is left in the workspace the weight-gradient product reads
    eng2 = _engine(m, u)
    zd2 = torch.from_numpy(z).to(dev)
    eng2.fit_begin(n, 17)
    g_fresh, _ = _fit_grad_check(R, eng2, m, (x, y, v, z), (xd, yd, vd, zd2), idx17, "B=17 fresh")
    eng2.fit_end()
    a, b = g_same.cpu().numpy(), g_fresh.cpu().numpy()
    o = 0
    for net, part in zip("gfh", parts):
        d = np.abs(a[o:o + part.size] - b[o:o + part.size]).max()
        R.add("B=17 same session vs fresh d%s" % net, d / (5e-5 * np.abs(part).max() + 1e-7), "(bit-identical: %s)" % (d == 0.0))
        o += part.size
    R.check()
