"""BGM HMC with a step size per chain (bgm_bgm_hmc_run_rows, BgmEngine.hmc_run_rows / hmc_sample(row_adapt=), BGM.predict /
tfp_mcmc_sampler(row_adapt=)) on the GPU: frozen equal steps against the scalar-step kernel bit for bit, chains and steps against the
float32 NumPy restatement (tests/_bgm_row_step_ref.py) under test_gpu_bgm.py's own bars, and the properties that make a chain a
function of (seed, global row, the row's data) alone -- launch cuts, row subsets, a second pass of the persistent waves.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bgm_row_step_ref import PARITY, PARITY_CASES, hmc_sampler  # noqa: E402
from test_gpu_bgm import _bgm_params, _data, _engine, _model  # noqa: E402

from oracle import bgm as OB  # noqa: E402



def _run_rows(eng, x, burn, keep, L, seed, step0=0.02, target=0.75, cuts=(), row_base=0, adapt=True):
    """One run of hmc_run_rows over launches cut at `cuts` -> dict of device tensors (draws, state, logp, grad, step, acc_count, acc_prob)."""
    import torch
    dev = eng.device
    x = torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    n, total = x.shape[0], burn + keep
    state, grad = (torch.empty((n, eng.q), device=dev) for _ in range(2))
    logp = torch.empty(n, device=dev)
    step = torch.full((n,), float(step0), device=dev)
    acc_prob = torch.zeros(total, device=dev, dtype=torch.float64)
    acc_count = torch.zeros(total, device=dev, dtype=torch.int32)
    draws = torch.empty((keep, n, eng.q), device=dev)
    up, dn = eng.row_step_table(burn, target) if adapt else (None, None)
    marks = [0] + list(cuts) + [total]
    for a, b in zip(marks[:-1], marks[1:]):
        eng.hmc_run_rows(x, state, logp, grad, step, a, b - a, burn, L, seed, init=(a == 0), row_base=row_base, up=up, dn=dn,
                         acc_prob=acc_prob, acc_count=acc_count, draws=draws)
    return dict(draws=draws, state=state, logp=logp, grad=grad, step=step, acc_count=acc_count, acc_prob=acc_prob)


# ---- 1. frozen equal steps: the scalar-step kernel, bit for bit; one case per compiled family
FROZEN = [dict(p=20, n=50, nh=5, prec="fp32"),       # resident, 2 head tiles
          dict(p=100, n=50, nh=5, prec="fp32"),      # resident, 7 tiles
          dict(p=61, n=50, nh=5, prec="fp32"),       # streamed, p % 4 != 0
          dict(p=500, n=50, nh=5, prec="fp32"),      # streamed
          dict(p=20, n=17, nh=3, prec="fp32", q=3),
          dict(p=100, n=1, nh=3, prec="fp32"),
          dict(p=61, n=50, nh=5, prec="f16x3"),      # X4 false
          dict(p=500, n=50, nh=5, prec="f16x3"),     # X4 true
          dict(p=40, n=33, nh=3, prec="f16x3")]


@pytest.mark.parametrize("case", FROZEN, ids=lambda c: "p%d-n%d-nh%d-%s" % (c["p"], c["n"], c["nh"], c["prec"]))
def test_frozen_equal_steps_are_the_scalar_step_kernel_bit_for_bit(case):
    import torch
    q, p, n = case.get("q", 10), case["p"], case["n"]
    burn, keep, L, seed = 10, 10, 3, 77
    eng = _engine(_model(11, q, p, case["nh"]))
    eng.set_precision(case["prec"])
    x = torch.from_numpy(_data(n, p, 12)).to(eng.device)
    rows = _run_rows(eng, x, burn, keep, L, seed, adapt=False)
    dev = eng.device
    state, grad = (torch.empty((n, q), device=dev) for _ in range(2))
    logp = torch.empty(n, device=dev)
    step = torch.full((1,), 0.02, device=dev)
    acc_prob = torch.zeros(burn + keep, device=dev, dtype=torch.float64)
    acc_count = torch.zeros(burn + keep, device=dev, dtype=torch.int32)
    draws = torch.empty((keep, n, q), device=dev)
    eng.hmc_run(x, state, logp, grad, step, 0, burn + keep, burn, L, seed, init=True, acc_prob=acc_prob, acc_count=acc_count, draws=draws)
    for name, t in (("draws", draws), ("state", state), ("logp", logp), ("grad", grad), ("acc_count", acc_count), ("acc_prob", acc_prob)):
        assert torch.equal(rows[name], t), name
    assert torch.equal(rows["step"], torch.full((n,), 0.02, device=dev))
    assert int(acc_count.sum()) > 0


# ---- 2. chains and steps against the float32 restatement
@functools.lru_cache(maxsize=None)
def _parity_ref(i):
    c = PARITY_CASES[i]
    m, x = _model(11, c["q"], c["p"], c["nh"]), _data(c["n"], c["p"], 12)
    obs, clean = OB.obs_mask_of(x)
    ref = hmc_sampler(m, clean, obs, PARITY["n_mcmc"], PARITY["burn_in"], PARITY["step_size"], PARITY["n_leapfrog"], PARITY["seed"],
                      PARITY["target"])
    for v in ref.values():
        v.setflags(write=False)
    return m, x, ref


def _check_parity(i, prec):
    import torch
    m, x, ref = _parity_ref(i)
    n, burn, keep = len(x), PARITY["burn_in"], PARITY["n_mcmc"]
    eng = _engine(m)
    eng.set_precision(prec)
    a = dict(step_size=PARITY["step_size"], n_leapfrog=PARITY["n_leapfrog"], seed=PARITY["seed"], row_adapt=PARITY["target"])
    out = eng.hmc_sample(x, keep, burn, reduce_fn=lambda t: pytest.fail("reduce_fn called"), **a)
    assert "step" not in out and tuple(out["row_step"].shape) == (n,)
    draws, steps = out["draws"].cpu().numpy(), out["row_step"].cpu().numpy()
    assert draws.shape == ref["draws"].shape
    close = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 2e-3, axis=1).mean()
    same = (steps == ref["step"]).mean()
    dacc = np.abs(out["acc_count"].cpu().numpy().astype(np.int64) - ref["acc"].sum(axis=1)).max()
    print("%s p=%d n=%d: rows of the last draw within 2e-3 %.4f, steps bit-equal %.4f, acc_count worst |diff| %d of %d"
          % (prec, m["x_dim"], n, close, same, dacc, n))
    assert close >= 0.97, close
    assert same >= 0.97, same
    assert dacc <= 0.03 * n, dacc
    out2 = eng.hmc_sample(x, keep, burn, **a)
    assert torch.equal(out2["draws"], out["draws"]) and torch.equal(out2["row_step"], out["row_step"])


@pytest.mark.parametrize("i", range(len(PARITY_CASES)), ids=lambda i: "p%d-n%d-q%d" % tuple(PARITY_CASES[i][k] for k in "pnq"))
def test_chain_and_steps_match_the_restatement(i):
    _check_parity(i, "fp32")


@pytest.mark.parametrize("i", [2, 3], ids=lambda i: "p%d-n%d" % tuple(PARITY_CASES[i][k] for k in "pn"))
def test_chain_and_steps_match_the_restatement_in_split_precision(i):
    _check_parity(i, "f16x3")


# ---- 3. cuts, subsets, second pass
@pytest.mark.parametrize("p", [20, 40])      # resident / streamed
def test_launch_cuts_and_row_subsets_change_nothing(p):
    import torch
    n, burn, keep, L, seed = 100, 12, 8, 3, 9
    eng = _engine(_model(11, 10, p))
    x = _data(n, p, 12)
    one = _run_rows(eng, x, burn, keep, L, seed, step0=0.2)
    cut = _run_rows(eng, x, burn, keep, L, seed, step0=0.2, cuts=(5, 15))
    for name in ("draws", "state", "step", "logp", "grad", "acc_count"):
        assert torch.equal(one[name], cut[name]), name
    assert len(torch.unique(one["step"])) > 1
    sub = _run_rows(eng, x[37:90], burn, keep, L, seed, step0=0.2, row_base=37)
    assert torch.equal(sub["draws"], one["draws"][:, 37:90]) and torch.equal(sub["state"], one["state"][37:90])
    assert torch.equal(sub["step"], one["step"][37:90])


@pytest.mark.parametrize("p,waves", [(20, 8), (40, 12)])
def test_second_pass_and_ragged_last_tile(p, waves):
    """n = 16 x waves x CUs + 17: the first wave slots take a second row tile (and must reload its rows' steps), the last tile is ragged."""
    import torch
    eng = _engine(_model(11, 10, p))
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    n, burn, keep, L, seed = 16 * waves * cus + 17, 3, 3, 2, 4
    x = _data(n, p, 12)
    x[-17:, ::2] = 0.5            # (the rows of the second pass differ from the first pass's)
    whole = _run_rows(eng, x, burn, keep, L, seed, step0=0.3)
    cuts = [0, 16 * waves * cus // 3 + 5, n - 17 - 40, n]
    parts = [_run_rows(eng, x[a:b], burn, keep, L, seed, step0=0.3, row_base=a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(torch.cat([t["draws"] for t in parts], dim=1), whole["draws"])
    for name in ("state", "step", "logp"):
        assert torch.equal(torch.cat([t[name] for t in parts]), whole[name]), name
    assert torch.equal(sum(t["acc_count"] for t in parts), whole["acc_count"])
    assert len(torch.unique(whole["step"])) > 1


# ---- 4. the rule does its job
def test_per_chain_steps_sample_the_prior_and_reach_the_target():
    m = _model(21, 10, 20)
    x = np.full((512, 20), np.nan, np.float32)
    eng = _engine(m)
    burn, keep = 300, 200
    out = eng.hmc_sample(x, keep, burn, step_size=0.02, n_leapfrog=5, seed=5, row_adapt=0.75)
    d = out["draws"].cpu().numpy().reshape(-1, 10)
    steps = out["row_step"].cpu().numpy()
    acc = out["acc_count"].cpu().numpy()[burn:].sum() / (keep * 512)
    print("|mean| %.4f |var - 1| %.4f steps %.3f .. %.3f retained acceptance %.4f"
          % (np.abs(d.mean(0)).max(), np.abs(d.var(0) - 1).max(), steps.min(), steps.max(), acc))
    assert np.abs(d.mean(0)).max() < 0.03 and np.abs(d.var(0) - 1).max() < 0.06
    assert np.all(steps > np.float32(0.02))
    assert abs(acc - 0.75) < 0.05, acc
    out0 = eng.hmc_sample(x, 5, 0, step_size=0.02, n_leapfrog=5, seed=5, row_adapt=0.75)
    assert np.all(out0["row_step"].cpu().numpy() == np.float32(0.02)) and tuple(out0["draws"].shape) == (5, 512, 10)


# ---- 5. classes
def test_bgm_class_predict_and_sampler_with_per_chain_steps(tmp_path):
    from bayesgm_amd.models import BGM
    p, n, burn, keep, L, seed = 100, 150, 30, 20, 4, 5
    m = _model(41, 10, p)
    x = _data(n, p, 42)
    model = BGM(_bgm_params(tmp_path, p), random_seed=0)
    model.set_weights(m["g"])
    a = dict(alpha=0.1, n_mcmc=keep, burn_in=burn, step_size=0.02, num_leapfrog_steps=L, seed=seed)
    imp, interval = model.predict(x, row_adapt=True, **a)
    steps = model.hmc_row_step_
    assert steps.shape == (n,) and steps.dtype == np.float32 and len(np.unique(steps)) > 1
    # 32-row blocks in the sampling phase (k_slots = p: row 0 has nothing observed): the same bits
    imp_b, interval_b = model.predict(x, row_adapt=True, max_draw_bytes=32 * 4 * keep * (10 + p), **a)
    assert np.array_equal(imp, imp_b) and np.array_equal(steps, model.hmc_row_step_)
    assert all(np.array_equal(u, v) for u, v in zip(interval, interval_b))
    # the restatement's chain, the oracle's predictive draws
    obs, clean = OB.obs_mask_of(x)
    ref = hmc_sampler(m, clean, obs, keep, burn, 0.02, L, seed, 0.75)
    ref_imp = OB.predict_on_posteriors(m, ref["draws"], seed, burn_in=burn).mean(axis=0)
    d = np.where(obs, 0.0, np.abs(imp - ref_imp)).max(axis=1)
    print("rows with every imputed cell within 1e-4: %d of %d (worst %.3g); steps bit-equal %.4f" % ((d < 1e-4).sum(), n, d.max(), (steps == ref["step"]).mean()))
    assert (d < 1e-4).sum() >= n - 1, d
    assert np.array_equal(imp[obs], x[obs]) and not np.isnan(imp).any()
    # shapes as without the option, which leaves no steps behind
    imp0, interval0 = model.predict(x, **a)
    assert model.hmc_row_step_ is None
    assert imp0.shape == imp.shape and len(interval0) == len(interval) and all(u.shape == v.shape for u, v in zip(interval0, interval))
    model.mcmc_diagnostics_ = None
    z = model.tfp_mcmc_sampler(x, n_mcmc=keep, burn_in=burn, step_size=0.02, num_leapfrog_steps=L, seed=seed, row_adapt=0.8, diagnostics=True)
    assert z.shape == (keep, n, 10) and model.mcmc_diagnostics_ is not None and model.hmc_row_step_.shape == (n,)
    with pytest.raises(ValueError, match="row_adapt"):
        model.predict(x, row_adapt=1.0, **a)


def test_split_precision_class_predict_with_per_chain_steps(tmp_path):
    from bayesgm_amd.models import BGM
    p, n = 61, 40
    params = _bgm_params(tmp_path, p)
    params["hmc_precision"] = "f16x3"
    model = BGM(params, random_seed=0)
    model.set_weights(_model(41, 10, p)["g"])
    x = _data(n, p, 42)
    imp, _ = model.predict(x, n_mcmc=10, burn_in=10, step_size=0.02, num_leapfrog_steps=3, seed=5, row_adapt=True)
    assert imp.shape == (n, p) and not np.isnan(imp).any() and model.hmc_row_step_.shape == (n,)


# ---- 6. refusals
def test_general_width_engine_is_refused_and_the_handle_stays_usable():
    import torch
    from bayesgm_amd.engine import BgmEngine
    m = OB.init_model(3, 4, 20, g_units=(32, 32))
    eng = BgmEngine(20, 4, g_units=[32, 32])
    eng.set_weights(m["g"])
    x = torch.from_numpy(_data(33, 20, 12)).to(eng.device)
    with pytest.raises(RuntimeError, match=r"\(-4\).*general-width"):
        _run_rows(eng, x, 2, 2, 2, 1)
    out = eng.hmc_sample(x, 4, 4, step_size=0.02, n_leapfrog=2, seed=1)
    assert bool(torch.isfinite(out["draws"]).all())


def test_invalid_arguments_are_named():
    import torch
    eng = _engine(_model(11, 10, 20))
    dev = eng.device
    n = 20
    x = torch.from_numpy(_data(n, 20, 12)).to(dev)
    state, grad = (torch.empty((n, 10), device=dev) for _ in range(2))
    logp, step = torch.empty(n, device=dev), torch.full((n,), 0.02, device=dev)
    up, dn = eng.row_step_table(4, 0.75)

    def call(x=x, state=state, logp=logp, grad=grad, step=step, L=2, row_base=0, **kw):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, L, 1, init=True, row_base=row_base, **kw)

    class _Null(object):      # a NULL device pointer
        shape = (n, 20)

        @staticmethod
        def data_ptr():
            return None

    for kw, word in ((dict(up=up), "dn_dev"), (dict(dn=dn), "up_dev"), (dict(up=up, dn=dn, s_min=0.0), "s_min"),
                     (dict(up=up, dn=dn, s_min=1.0, s_max=0.5), "s_max"), (dict(up=up, dn=dn, s_max=float("inf")), "s_max"),
                     (dict(x=_Null()), "x_dev"), (dict(state=_Null()), "state_dev"), (dict(logp=_Null()), "logp_dev"),
                     (dict(grad=_Null()), "grad_dev"), (dict(step=_Null()), "step_dev"), (dict(L=0), "n_leapfrog"),
                     (dict(row_base=0xFFFFFFFF - 5), "row")):
        with pytest.raises(RuntimeError, match=r"\(-1\).*" + word):
            call(**kw)
    a = eng._hmc_args(x, state, logp, grad, step, 0, 4, 2, 2, 1, True, 0, None, None, None)      # n_table < 0 cannot come from a tensor
    import ctypes as C
    assert eng.lib.bgm_bgm_hmc_run_rows(eng.h, C.byref(a), C.c_void_p(up.data_ptr()), C.c_void_p(dn.data_ptr()), -1, 1e-4, 1e2, None) == -1
    assert b"n_table" in eng.lib.bgm_last_error()
    call(up=up, dn=dn)      # and the engine still samples
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state).all())
