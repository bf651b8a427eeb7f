"""BGM HMC with a number of leapfrog steps per chain (bgm_bgm_hmc_run_rows_traj, BgmEngine.hmc_run_rows / hmc_sample(max_trajectory=,
jitter=), BGM.predict / tfp_mcmc_sampler(max_trajectory=, jitter_leapfrog=)) on the GPU: with the options off, or a cap that never
binds, the per-chain-step kernel bit for bit; a uniform cap against a run with fewer steps bit for bit; rows of one tile with different
lengths; chains, steps and step counts against the float32 NumPy restatement (tests/_bgm_traj_ref.py) under the bars of
test_gpu_bgm_row_step.py; launch cuts, row subsets, a second pass; and the defect the options exist for -- a chain whose trajectory
spans a period returns to its start -- with its cure.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bgm_traj_ref import PARITY_CASES, TRAJ_PARITY, hmc_sampler  # noqa: E402
from test_gpu_bgm import _bgm_params, _data, _engine, _model  # noqa: E402
from test_gpu_bgm_row_step import FROZEN  # noqa: E402

from oracle import bgm as OB  # noqa: E402

# one shape per compiled family: FROZEN lacks the streamed 3-layer trunk in fp32 and the 3-layer split-precision kernel for p % 4 != 0
FAMILIES = FROZEN + [dict(p=61, n=33, nh=3, prec="fp32"), dict(p=61, n=33, nh=3, prec="f16x3")]
NAMES = ("draws", "state", "logp", "grad", "acc_count", "acc_prob", "step")
_fid = lambda c: "p%d-n%d-nh%d-%s" % (c["p"], c["n"], c["nh"], c["prec"])  # noqa: E731


def _run(eng, x, burn, keep, L, seed, step0=0.02, target=0.75, cuts=(), row_base=0, adapt=True, count=False, **traj):
    """One run of hmc_run_rows over launches cut at `cuts` -> dict of device tensors; step0 a number or [n] steps; count: n_steps of
    ALL iterations."""
    import torch
    dev = eng.device
    x = torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    n, total = x.shape[0], burn + keep
    state, grad = (torch.empty((n, eng.q), device=dev) for _ in range(2))
    logp = torch.empty(n, device=dev)
    step = torch.empty(n, device=dev)
    step[:] = torch.as_tensor(step0, dtype=torch.float32, device=dev)
    acc_prob = torch.zeros(total, device=dev, dtype=torch.float64)
    acc_count = torch.zeros(total, device=dev, dtype=torch.int32)
    draws = torch.empty((keep, n, eng.q), device=dev)
    n_steps = torch.zeros(n, device=dev, dtype=torch.int32) if count else None
    up, dn = eng.row_step_table(burn, target) if adapt else (None, None)
    marks = [0] + list(cuts) + [total]
    for a, b in zip(marks[:-1], marks[1:]):
        eng.hmc_run_rows(x, state, logp, grad, step, a, b - a, burn, L, seed, init=(a == 0), row_base=row_base, up=up, dn=dn,
                         acc_prob=acc_prob, acc_count=acc_count, draws=draws, n_steps=n_steps, **traj)
    return dict(draws=draws, state=state, logp=logp, grad=grad, step=step, acc_count=acc_count, acc_prob=acc_prob, n_steps=n_steps)


def _case(case, seed_m=11, seed_x=12):
    import torch
    eng = _engine(_model(seed_m, case.get("q", 10), case["p"], case["nh"]))
    eng.set_precision(case["prec"])
    return eng, torch.from_numpy(_data(case["n"], case["p"], seed_x)).to(eng.device)


def _same(a, b, names=NAMES, rows=None):
    import torch
    for name in names:
        u, v = a[name], b[name]
        if rows is not None and name not in ("acc_count", "acc_prob"):
            u, v = (t[:, rows] if name == "draws" else t[rows] for t in (u, v))
        assert torch.equal(u, v), name


# ---- 1. off is the old kernel
@pytest.mark.parametrize("case", FAMILIES, ids=_fid)
def test_options_off_and_a_cap_that_never_binds_are_the_per_chain_step_kernel_bit_for_bit(case):
    import ctypes as C
    import torch
    eng, x = _case(case)
    n, burn, keep, L, seed = case["n"], 6, 4, 3, 77
    old = _run(eng, x, burn, keep, L, seed, step0=0.1)
    # the new entry with (0, 0, NULL), called as the engine would
    dev = eng.device
    new = dict(state=torch.empty((n, eng.q), device=dev), grad=torch.empty((n, eng.q), device=dev), logp=torch.empty(n, device=dev),
               step=torch.full((n,), 0.1, device=dev), acc_prob=torch.zeros(burn + keep, device=dev, dtype=torch.float64),
               acc_count=torch.zeros(burn + keep, device=dev, dtype=torch.int32), draws=torch.empty((keep, n, eng.q), device=dev))
    up, dn = eng.row_step_table(burn, 0.75)
    a = eng._hmc_args(x, new["state"], new["logp"], new["grad"], new["step"], 0, burn + keep, burn, L, seed, True, 0, new["acc_prob"],
                      new["acc_count"], new["draws"])
    rc = eng.lib.bgm_bgm_hmc_run_rows_traj(eng.h, C.byref(a), C.c_void_p(up.data_ptr()), C.c_void_p(dn.data_ptr()), int(up.numel()), 1e-4, 1e2,
                                           0.0, 0, None, None)
    assert rc == 0, eng.lib.bgm_last_error()
    _same(old, new)
    # a cap that never binds, on the kernels that have the rule; the count is L per iteration
    far = _run(eng, x, burn, keep, L, seed, step0=0.1, max_trajectory=1e9, count=True)
    _same(old, far)
    assert torch.equal(far["n_steps"], torch.full((n,), L * (burn + keep), device=dev, dtype=torch.int32))
    assert int(old["acc_count"].sum()) > 0


# ---- 2. a uniform cap is a shorter run
@functools.lru_cache(maxsize=None)
def _short(i, L, step):
    """FAMILIES[i] with all steps `step`, frozen, at n_leapfrog = L."""
    eng, x = _case(FAMILIES[i])
    return _run(eng, x, 0, 8, L, 77, step0=step, adapt=False)


@pytest.mark.parametrize("i", range(len(FAMILIES)), ids=lambda i: _fid(FAMILIES[i]))
def test_a_uniform_cap_is_a_run_with_fewer_steps_bit_for_bit(i):
    import torch
    eng, x = _case(FAMILIES[i])
    n = FAMILIES[i]["n"]
    # 2 x 0.05 = 0.10 < 0.12 <= 0.15 = 3 x 0.05: three of the six steps
    capped = _run(eng, x, 0, 8, 6, 77, step0=0.05, adapt=False, max_trajectory=0.12, count=True)
    _same(capped, _short(i, 3, 0.05))
    assert torch.equal(capped["n_steps"], torch.full((n,), 3 * 8, device=eng.device, dtype=torch.int32))
    full = _run(eng, x, 0, 8, 6, 77, step0=0.05, adapt=False)
    assert not torch.equal(full["draws"], capped["draws"])


# ---- 3. mixed lengths inside one tile
MIXED = [i for i, c in enumerate(FAMILIES) if (c["p"], c["n"], c["nh"], c["prec"]) in
         ((100, 50, 5, "fp32"), (500, 50, 5, "fp32"), (20, 17, 3, "fp32"), (61, 50, 5, "f16x3"))]


@pytest.mark.parametrize("i", MIXED, ids=lambda i: _fid(FAMILIES[i]))
def test_rows_of_one_tile_take_different_numbers_of_steps(i):
    """Steps 0.05 / 0.03 by row under T = 0.12: L_i = 3 / 4 (4 x 0.03f == 0.12f exactly, and the compare is strict).  acc_count and
    acc_prob mix both kinds of rows and are not compared."""
    import torch
    assert len(MIXED) == 4
    eng, x = _case(FAMILIES[i])
    n = FAMILIES[i]["n"]
    dev = eng.device
    even = torch.arange(n, device=dev) % 2 == 0
    step0 = torch.where(even, 0.05, 0.03).float()
    mixed = _run(eng, x, 0, 8, 6, 77, step0=step0, adapt=False, max_trajectory=0.12, count=True)
    names = ("draws", "state", "logp", "grad", "step")
    _same(mixed, _short(i, 3, 0.05), names, rows=even)
    if n > 1:
        _same(mixed, _short(i, 4, 0.03), names, rows=~even)
    assert torch.equal(mixed["n_steps"], torch.where(even, 3 * 8, 4 * 8).int())


# ---- 4. parity with the restatement, adaptive
@functools.lru_cache(maxsize=None)
def _parity_ref(i, jitter):
    c, P = PARITY_CASES[i], TRAJ_PARITY
    m, x = _model(11, c["q"], c["p"], c["nh"]), _data(c["n"], c["p"], 12)
    obs, clean = OB.obs_mask_of(x)
    ref = hmc_sampler(m, clean, obs, P["n_mcmc"], P["burn_in"], P["step_size"], P["n_leapfrog"], P["seed"], P["target"], P["max_trajectory"],
                      jitter)
    for v in ref.values():
        v.setflags(write=False)
    return m, x, ref


def _check_parity(i, prec, jitter):
    import torch
    m, x, ref = _parity_ref(i, jitter)
    P = TRAJ_PARITY
    n, burn, keep = len(x), P["burn_in"], P["n_mcmc"]
    eng = _engine(m)
    eng.set_precision(prec)
    a = dict(step_size=P["step_size"], n_leapfrog=P["n_leapfrog"], seed=P["seed"], row_adapt=P["target"], max_trajectory=P["max_trajectory"],
             jitter=jitter)
    out = eng.hmc_sample(x, keep, burn, **a)
    assert tuple(out["row_step"].shape) == (n,) and out["n_steps"].dtype == torch.int32 and tuple(out["n_steps"].shape) == (n,)
    draws, steps, n_steps = out["draws"].cpu().numpy(), out["row_step"].cpu().numpy(), out["n_steps"].cpu().numpy()
    assert draws.shape == ref["draws"].shape
    close = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 2e-3, axis=1).mean()
    same = (steps == ref["step"]).mean()
    same_n = (n_steps == ref["n_steps"]).mean()
    dacc = np.abs(out["acc_count"].cpu().numpy().astype(np.int64) - ref["acc"].sum(axis=1)).max()
    print("%s p=%d n=%d jitter=%d: rows of the last draw within 2e-3 %.4f, steps bit-equal %.4f, n_steps equal %.4f, acc_count worst "
          "|diff| %d of %d, mean L_i %.2f" % (prec, m["x_dim"], n, jitter, close, same, same_n, dacc, n, n_steps.mean() / keep))
    assert close >= 0.97, close
    assert same >= 0.97, same
    assert same_n >= 0.97, same_n
    assert dacc <= 0.03 * n, dacc
    assert n_steps.min() >= keep and n_steps.max() <= keep * P["n_leapfrog"] and (len(np.unique(n_steps)) > 1 or n < 64)
    out2 = eng.hmc_sample(x, keep, burn, **a)
    assert all(torch.equal(out2[k], out[k]) for k in ("draws", "row_step", "n_steps", "acc_count"))


@pytest.mark.parametrize("jitter", [False, True], ids=["cap", "cap-jitter"])
@pytest.mark.parametrize("i", range(len(PARITY_CASES)), ids=lambda i: "p%d-n%d-q%d" % tuple(PARITY_CASES[i][k] for k in "pnq"))
def test_chain_steps_and_step_counts_match_the_restatement(i, jitter):
    _check_parity(i, "fp32", jitter)


@pytest.mark.parametrize("jitter", [False, True], ids=["cap", "cap-jitter"])
@pytest.mark.parametrize("i", [2, 3], ids=lambda i: "p%d-n%d" % tuple(PARITY_CASES[i][k] for k in "pn"))
def test_chain_steps_and_step_counts_match_the_restatement_in_split_precision(i, jitter):
    _check_parity(i, "f16x3", jitter)


# ---- 5. cuts, subsets, second pass
TRAJ = dict(max_trajectory=0.7, jitter=True)      # (steps from 0.2 adapt across 0.7 / l for several l: the caps differ by row and move in burn-in)


@pytest.mark.parametrize("p", [20, 40])      # resident / streamed
def test_launch_cuts_and_row_subsets_change_nothing(p):
    import torch
    n, burn, keep, L, seed = 100, 12, 8, 4, 9
    eng = _engine(_model(11, 10, p))
    x = _data(n, p, 12)
    one = _run(eng, x, burn, keep, L, seed, step0=0.2, count=True, **TRAJ)
    cut = _run(eng, x, burn, keep, L, seed, step0=0.2, cuts=(5, 15), count=True, **TRAJ)
    _same(one, cut, ("draws", "state", "step", "logp", "grad", "acc_count", "n_steps"))
    assert len(torch.unique(one["step"])) > 1 and len(torch.unique(one["n_steps"])) > 1
    assert int(one["n_steps"].min()) >= burn + keep and int(one["n_steps"].max()) < L * (burn + keep)
    sub = _run(eng, x[37:90], burn, keep, L, seed, step0=0.2, row_base=37, count=True, **TRAJ)
    assert torch.equal(sub["draws"], one["draws"][:, 37:90]) and torch.equal(sub["state"], one["state"][37:90])
    assert torch.equal(sub["step"], one["step"][37:90]) and torch.equal(sub["n_steps"], one["n_steps"][37:90])


@pytest.mark.parametrize("p,waves", [(20, 8), (40, 12)])
def test_second_pass_and_ragged_last_tile(p, waves):
    """n = 16 x waves x CUs + 17: the first wave slots take a second row tile (whose step count starts anew), the last tile is ragged."""
    import torch
    eng = _engine(_model(11, 10, p))
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    n, burn, keep, L, seed = 16 * waves * cus + 17, 3, 3, 3, 4
    x = _data(n, p, 12)
    x[-17:, ::2] = 0.5            # (the rows of the second pass differ from the first pass's)
    whole = _run(eng, x, burn, keep, L, seed, step0=0.3, count=True, **TRAJ)
    cuts = [0, 16 * waves * cus // 3 + 5, n - 17 - 40, n]
    parts = [_run(eng, x[a:b], burn, keep, L, seed, step0=0.3, row_base=a, count=True, **TRAJ) for a, b in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(torch.cat([t["draws"] for t in parts], dim=1), whole["draws"])
    for name in ("state", "step", "logp", "n_steps"):
        assert torch.equal(torch.cat([t[name] for t in parts]), whole[name]), name
    assert torch.equal(sum(t["acc_count"] for t in parts), whole["acc_count"])
    assert len(torch.unique(whole["step"])) > 1 and len(torch.unique(whole["n_steps"])) > 1


# ---- 6. the defect and its cure
def _lag1(d):
    """mean over rows and latents of the lag-1 autocorrelation of draws [T, n, q]"""
    c = d - d.mean(axis=0)
    return float(((c[1:] * c[:-1]).sum(axis=0) / (c * c).sum(axis=0)).mean())


@pytest.mark.parametrize("name,traj,bar", [("no cap", {}, lambda r: r > 0.8), ("max_trajectory = pi / 2", dict(max_trajectory=np.pi / 2), lambda r: r < 0.1),
                                           ("jitter only", dict(jitter=True), lambda r: r < 0.3)], ids=["no-cap", "cap", "jitter"])
def test_a_trajectory_of_one_period_returns_to_its_start_and_the_options_cure_it(name, traj, bar):
    """Rows with nothing observed sample N(0, I); step 0.6283 x 10 steps = one period 2 pi of every coordinate.  The restatement gives
    lag-1 autocorrelations of +0.960 (no cap), -0.206 (cap pi / 2: 3 steps), +0.075 (jitter only) at variance 1.00.

    Mean and variance are taken over all draws of all latents.  Per latent the bars 0.03 / 0.06 cannot hold for the chain without a
    cap: at autocorrelation 0.96 its 200 draws are worth 200 x 0.04 / 1.96 = 4, the 512 chains 2100, so a latent's mean has a standard
    deviation of 0.022 (the restatement: worst |mean| 0.071, worst |var - 1| 0.096 per latent, 0.001 and 0.0002 over all).  The two
    cured settings are held to the bars per latent as well (the restatement: 0.003 / 0.009 and 0.004 / 0.019)."""
    m = _model(21, 10, 20)
    x = np.full((512, 20), np.nan, np.float32)
    eng = _engine(m)
    out = _run(eng, x, 0, 200, 10, 5, step0=0.6283, adapt=False, count=bool(traj), **traj)      # (no options: the kernel as it was)
    d = out["draws"].cpu().numpy().astype(np.float64)
    r = _lag1(d)
    flat = d.reshape(-1, 10)
    acc = float(out["acc_count"].sum()) / (200 * 512)
    print("%s: lag-1 autocorrelation %.3f, acceptance %.3f, over all |mean| %.4f |var - 1| %.4f, per latent %.4f %.4f, mean L_i %.2f"
          % (name, r, acc, abs(flat.mean()), abs(flat.var() - 1), np.abs(flat.mean(0)).max(), np.abs(flat.var(0) - 1).max(),
             float(out["n_steps"].float().mean()) / 200 if traj else 10))
    assert bar(r), r
    assert abs(flat.mean()) < 0.03 and abs(flat.var() - 1) < 0.06
    if traj:
        assert np.abs(flat.mean(0)).max() < 0.03 and np.abs(flat.var(0) - 1).max() < 0.06


# ---- 7. classes and refusals
def test_bgm_class_predict_and_sampler_with_trajectories(tmp_path):
    from bayesgm_amd.models import BGM
    p, n, burn, keep, L, seed = 100, 150, 30, 20, 6, 5
    m = _model(41, 10, p)
    x = _data(n, p, 42)
    model = BGM(_bgm_params(tmp_path, p), random_seed=0)
    model.set_weights(m["g"])
    a = dict(alpha=0.1, n_mcmc=keep, burn_in=burn, step_size=0.02, num_leapfrog_steps=L, seed=seed, row_adapt=True, max_trajectory=0.4,
             jitter_leapfrog=True)
    imp, interval = model.predict(x, **a)
    steps, leaps = model.hmc_row_step_, model.hmc_row_leapfrog_
    assert leaps.shape == (n,) and leaps.dtype == np.float32 and len(np.unique(leaps)) > 1
    assert leaps.min() >= 1 and leaps.max() <= L
    # 32-row blocks in the sampling phase: the same bits
    imp_b, interval_b = model.predict(x, max_draw_bytes=32 * 4 * keep * (10 + p), **a)
    assert np.array_equal(imp, imp_b) and np.array_equal(steps, model.hmc_row_step_) and np.array_equal(leaps, model.hmc_row_leapfrog_)
    assert all(np.array_equal(u, v) for u, v in zip(interval, interval_b))
    # the restatement's chain and step counts
    obs, clean = OB.obs_mask_of(x)
    ref = hmc_sampler(m, clean, obs, keep, burn, 0.02, L, seed, 0.75, 0.4, True)
    same_n = (leaps == (ref["n_steps"] / np.float32(keep)).astype(np.float32)).mean()
    print("steps bit-equal %.4f, mean steps per transition equal %.4f, %.2f .. %.2f" % ((steps == ref["step"]).mean(), same_n, leaps.min(), leaps.max()))
    assert same_n >= 0.97 and (steps == ref["step"]).mean() >= 0.97
    assert np.array_equal(imp[obs], x[obs]) and not np.isnan(imp).any()
    # the sampler leaves the same record; without the options none
    z = model.tfp_mcmc_sampler(x, n_mcmc=keep, burn_in=burn, step_size=0.02, num_leapfrog_steps=L, seed=seed, row_adapt=True, max_trajectory=0.4,
                               jitter_leapfrog=True)
    assert z.shape == (keep, n, 10) and np.array_equal(model.hmc_row_leapfrog_, leaps) and np.array_equal(model.hmc_row_step_, steps)
    model.predict(x, alpha=0.1, n_mcmc=keep, burn_in=burn, step_size=0.02, num_leapfrog_steps=L, seed=seed, row_adapt=True)
    assert model.hmc_row_leapfrog_ is None and model.hmc_row_step_ is not None
    for kw in (dict(max_trajectory=0.4), dict(jitter_leapfrog=True)):
        with pytest.raises(ValueError, match="row_adapt"):
            model.predict(x, alpha=0.1, n_mcmc=keep, burn_in=burn, **kw)


def test_general_width_engine_is_refused_and_the_handle_stays_usable():
    import torch
    from bayesgm_amd.engine import BgmEngine
    m = OB.init_model(3, 4, 20, g_units=(32, 32))
    eng = BgmEngine(20, 4, g_units=[32, 32])
    eng.set_weights(m["g"])
    x = torch.from_numpy(_data(33, 20, 12)).to(eng.device)
    with pytest.raises(RuntimeError, match=r"\(-4\).*general-width"):
        _run(eng, x, 2, 2, 2, 1, max_trajectory=0.4, jitter=True)
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

    def call(x=x, L=2, **kw):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, L, 1, init=True, **kw)

    class _Null(object):      # a NULL device pointer
        shape = (n, 20)

        @staticmethod
        def data_ptr():
            return None

    for kw, word in ((dict(max_trajectory=-0.5), "max_trajectory"), (dict(max_trajectory=float("inf")), "max_trajectory"),
                     (dict(max_trajectory=float("nan")), "max_trajectory"), (dict(jitter=2), "jitter"), (dict(jitter=-1), "jitter"),
                     (dict(jitter=True, up=up), "dn_dev"), (dict(jitter=True, up=up, dn=dn, s_min=0.0), "s_min"),
                     (dict(jitter=True, x=_Null()), "x_dev"), (dict(max_trajectory=0.4, L=0), "n_leapfrog")):
        with pytest.raises(RuntimeError, match=r"hmc_run_rows_traj failed \(-1\).*" + word):
            call(**kw)
    with pytest.raises(ValueError, match="row_adapt"):
        eng.hmc_sample(x, 4, 4, max_trajectory=0.4)
    with pytest.raises(ValueError, match="max_trajectory"):
        eng.hmc_sample(x, 4, 4, row_adapt=0.75, max_trajectory=0.0)
    call(up=up, dn=dn, max_trajectory=0.4, jitter=True)      # and the engine still samples
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state).all())
