"""BGM imputation inside the per-chain HMC kernel (bgm_bgm_hmc_run_rows_impute, BgmEngine.hmc_run_rows(moments=) / hmc_sample(impute=),
BGM.predict(fused_predict=True)) on the GPU: the chain is the un-fused kernel's bit for bit; the predictive values are predict_draws'
on the stored draws; the moments are inside the derived bounds of tests/_bgm_impute_ref.py against float64 on the same latents; launch
cuts, row windows and a second pass change nothing; nothing but the missing cells is written; the class route against the blocked one.
"""
import functools
import os
import statistics
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bgm_impute_ref as IR  # noqa: E402
from test_gpu_bgm import _bgm_params, _data, _engine, _model  # noqa: E402

from oracle import bgm as OB  # noqa: E402

CHAIN = ("state", "logp", "grad", "step", "acc_count", "acc_prob")
TRAJ = dict(max_trajectory=0.25, jitter=True)      # (steps adapt from 0.1 across 0.25 / l: the caps differ by row)
GUARD = 257      # floats behind the planes and behind the cells


def _run(eng, x, burn, keep, L, seed, fused, cuts=(), row_base=0, slot=None, k_slots=0, add_noise=True, n_keep=None, traj=None,
         want_cells=True):
    """One run of hmc_run_rows over launches cut at `cuts` -> dict of device tensors.  fused: with moments (NaN beforehand, a NaN guard
    band behind them) and, with slot, cells (the same); else with draws."""
    import torch
    dev = eng.device
    x = torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    n, p, total = x.shape[0], x.shape[1], burn + keep
    state, grad = (torch.empty((n, eng.q), device=dev) for _ in range(2))
    logp = torch.empty(n, device=dev)
    step = torch.full((n,), 0.1, device=dev)
    acc_prob = torch.zeros(total, device=dev, dtype=torch.float64)
    acc_count = torch.zeros(total, device=dev, dtype=torch.int32)
    traj = dict(traj or {})
    n_steps = torch.zeros(n, device=dev, dtype=torch.int32) if traj else None
    up, dn = eng.row_step_table(burn, 0.75)
    out = dict(state=state, logp=logp, grad=grad, step=step, acc_count=acc_count, acc_prob=acc_prob, n_steps=n_steps)
    kw = {}
    if fused:
        buf = torch.full((3 * n * p + GUARD,), float("nan"), device=dev)
        out["moments"], out["guard"] = buf[:3 * n * p].view(3, n, p), buf[3 * n * p:]
        kw = dict(moments=out["moments"], n_keep=keep if n_keep is None else n_keep, add_noise=add_noise)
        if slot is not None and want_cells:
            cbuf = torch.full((n * k_slots * keep + GUARD,), float("nan"), device=dev)
            out["cells"], out["cells_guard"] = cbuf[:n * k_slots * keep].view(n * k_slots, keep), cbuf[n * k_slots * keep:]
            kw.update(cells=out["cells"], slot=torch.as_tensor(slot, dtype=torch.int32, device=dev).contiguous(), k_slots=k_slots)
    else:
        out["draws"] = torch.empty((keep, n, eng.q), device=dev)
        kw = dict(draws=out["draws"])
    marks = [0] + list(cuts) + [total]
    for a, b in zip(marks[:-1], marks[1:]):
        eng.hmc_run_rows(x, state, logp, grad, step, a, b - a, burn, L, seed, init=(a == 0), row_base=row_base, up=up, dn=dn,
                         acc_prob=acc_prob, acc_count=acc_count, n_steps=n_steps, **traj, **kw)
    torch.cuda.synchronize(dev)
    return out


def _setup(c, seed_m=11, seed_x=12):
    m = _model(seed_m, c.get("q", 10), c["p"], c["nh"])
    x = _data(c["n"], c["p"], seed_x, miss=IR.MISS)      # (row 0 has every cell missing, row 1 none)
    slot, k_slots = IR.slots_of(np.isnan(x))
    return m, x, slot, k_slots


@functools.lru_cache(maxsize=None)
def _runs(i, keep=IR.KEEP):
    """CASES[i]: the un-fused run (with draws), the fused one (moments and cells) and the float64 predictive values on the draws;
    computed once, shared, never written."""
    c = IR.CASES[i]
    m, x, slot, k_slots = _setup(c)
    eng = _engine(m)
    plain = _run(eng, x, IR.BURN, keep, IR.LEAP, 77, False)
    fused = _run(eng, x, IR.BURN, keep, IR.LEAP, 77, True, slot=slot, k_slots=k_slots)
    draws = plain["draws"].cpu().numpy()
    x64 = OB.predict_on_posteriors(OB.cast_model(m, np.float64), draws.astype(np.float64), seed=77, burn_in=IR.BURN)
    x64.setflags(write=False)
    return dict(m=m, x=x, slot=slot, k_slots=k_slots, eng=eng, plain=plain, fused=fused, x64=x64)


def _cells_of(cells, n, k_slots, keep):
    return cells.cpu().numpy().reshape(n, k_slots, keep)


def _used(miss, k_slots):
    return np.arange(k_slots)[None, :] < miss.sum(axis=1)[:, None]


_ids = dict(ids=lambda i: IR.case_id(IR.CASES[i]))


# ---- 1. the same chain
@pytest.mark.parametrize("traj", [None, TRAJ], ids=["plain", "cap-jitter"])
@pytest.mark.parametrize("i", range(len(IR.CASES)), **_ids)
def test_the_chain_is_the_unfused_kernels_bit_for_bit(i, traj):
    import torch
    if traj is None:
        r = _runs(i)
        plain, fused = r["plain"], r["fused"]
    else:
        m, x, slot, k_slots = _setup(IR.CASES[i])
        eng = _engine(m)
        plain = _run(eng, x, IR.BURN, IR.KEEP, IR.LEAP, 77, False, traj=traj)
        fused = _run(eng, x, IR.BURN, IR.KEEP, IR.LEAP, 77, True, slot=slot, k_slots=k_slots, traj=traj)
        assert torch.equal(plain["n_steps"], fused["n_steps"])
        assert int(plain["n_steps"].max()) <= IR.LEAP * (IR.BURN + IR.KEEP) and int(plain["n_steps"].min()) >= IR.BURN + IR.KEEP
    for name in CHAIN:
        assert torch.equal(plain[name], fused[name]), name
    assert int(plain["acc_count"].sum()) > 0 and bool(torch.isfinite(fused["state"]).all())


# ---- 2. the same values
@pytest.mark.parametrize("add_noise", [True, False], ids=["draw", "mean"])
@pytest.mark.parametrize("i", range(len(IR.CASES)), **_ids)
def test_cells_are_predict_draws_on_the_stored_draws_and_match_float64(i, add_noise):
    r = _runs(i)
    c, x, slot, k_slots, eng = IR.CASES[i], r["x"], r["slot"], r["k_slots"], r["eng"]
    import torch
    n, keep = c["n"], IR.KEEP
    fused = r["fused"] if add_noise else _run(eng, x, IR.BURN, keep, IR.LEAP, 77, True, slot=slot, k_slots=k_slots, add_noise=False)
    ref_cells, _ = eng.predict_draws(r["plain"]["draws"], IR.BURN, 77, slot=torch.from_numpy(slot).to(eng.device), k_slots=k_slots,
                                     add_noise=add_noise)
    got, ref = _cells_of(fused["cells"], n, k_slots, keep), _cells_of(ref_cells, n, k_slots, keep)
    miss = np.isnan(x)
    used = _used(miss, k_slots)
    assert np.array_equal(got[used], ref[used])
    assert np.isnan(got[~used]).all() and bool(torch.isnan(fused["cells_guard"]).all())
    # float64 on the same latents, the bar of test_predictive_draws_match_oracle_on_same_latents
    if add_noise:
        x64 = r["x64"]
    else:
        m64 = OB.cast_model(r["m"], np.float64)
        x64 = np.stack([OB.varnet_forward(m64["g"], z.astype(np.float64), training=False)[0] for z in r["plain"]["draws"].cpu().numpy()])
    worst = 0.0
    for row in range(n):
        cols = np.where(miss[row])[0]
        if len(cols):
            worst = max(worst, np.abs(got[row, :len(cols)] - x64[:, row, cols].T).max())
    print("%s add_noise=%d: worst |cell - float64| %.3g" % (IR.case_id(c), add_noise, worst))
    assert worst <= IR.VALUE_BAR


# ---- 3. the moments
def _check_moments(r, keep):
    x, mom = r["x"], r["fused"]["moments"].cpu().numpy()
    miss = np.isnan(x)
    mean_ref, var_ref, mean_bound, var_bound = IR.reference(r["x64"])
    mean, var = IR.mean_var(mom[0], mom[1], mom[2], keep)
    r_mean = (np.abs(mean - mean_ref) / mean_bound)[miss].max()
    r_var = (np.abs(var - var_ref) / var_bound)[miss].max()
    print("k = %d: worst |mean - ref| / bound %.3g, |var - ref| / bound %.3g; worst |mean - ref| %.3g" % (keep, r_mean, r_var,
                                                                                                        np.abs(mean - mean_ref)[miss].max()))
    assert r_mean <= 1.0 and r_var <= 1.0
    # plane 0 is the value at retained draw 0, and it is the cells' first column
    assert np.abs(mom[0] - r["x64"][0])[miss].max() <= IR.VALUE_BAR
    n, p = x.shape
    first = _cells_of(r["fused"]["cells"], n, r["k_slots"], keep)[:, :, 0]
    assert np.array_equal(first[_used(miss, r["k_slots"])], mom[0][miss])


@pytest.mark.parametrize("i", range(len(IR.CASES)), **_ids)
def test_moments_are_inside_the_derived_bounds_of_float64_on_the_same_latents(i):
    _check_moments(_runs(i), IR.KEEP)


def test_moments_are_inside_the_bounds_over_400_retained_draws():
    _check_moments(_runs(IR.CASES.index(IR.LONG), IR.KEEP_LONG), IR.KEEP_LONG)


# ---- 4. a row depends on itself only
@pytest.mark.parametrize("i", [0, 1, 3, 6], **_ids)
def test_launch_cuts_and_row_windows_change_nothing(i):
    import torch
    r = _runs(i)
    c, x, slot, k_slots, eng, one = IR.CASES[i], r["x"], r["slot"], r["k_slots"], r["eng"], r["fused"]
    total = IR.BURN + IR.KEEP
    cuts = tuple(range(4, total, 4))      # (4, 8): the second one lies inside the retained phase
    assert any(IR.BURN < t < total for t in cuts)
    cut = _run(eng, x, IR.BURN, IR.KEEP, IR.LEAP, 77, True, cuts=cuts, slot=slot, k_slots=k_slots)
    for name in CHAIN[:5] + ("moments", "cells"):
        assert torch.equal(one[name].view(torch.int32) if one[name].dtype == torch.float32 else one[name],
                           cut[name].view(torch.int32) if cut[name].dtype == torch.float32 else cut[name]), name
    a, b = (7, c["n"] - 5) if c["n"] > 20 else (0, c["n"])
    win = _run(eng, x[a:b], IR.BURN, IR.KEEP, IR.LEAP, 77, True, row_base=a, slot=slot[a:b], k_slots=k_slots)
    assert torch.equal(win["moments"].view(torch.int32), one["moments"][:, a:b].contiguous().view(torch.int32))
    assert torch.equal(win["cells"].view(torch.int32), one["cells"][a * k_slots:b * k_slots].view(torch.int32))
    assert torch.equal(win["state"], one["state"][a:b])


@pytest.mark.parametrize("p,waves", [(20, 8), (40, 12)])
def test_second_pass_and_ragged_last_tile(p, waves):
    """n = 16 x waves x CUs + 17: the first wave slots take a second row tile, the last tile is ragged; the planes and the cells of the
    rows of both passes are those of runs over row windows."""
    import torch
    eng = _engine(_model(11, 10, p))
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    n, burn, keep, L, seed = 16 * waves * cus + 17, 3, 3, 2, 4
    x = _data(n, p, 12, miss=IR.MISS)
    x[-17:, ::2] = np.nan            # (the rows of the second pass differ from the first pass's)
    slot, k_slots = IR.slots_of(np.isnan(x))
    whole = _run(eng, x, burn, keep, L, seed, True, slot=slot, k_slots=k_slots)
    marks = [0, 16 * waves * cus // 3 + 5, n - 17 - 40, n]
    parts = [_run(eng, x[a:b], burn, keep, L, seed, True, row_base=a, slot=slot[a:b], k_slots=k_slots) for a, b in zip(marks[:-1], marks[1:])]
    assert torch.equal(torch.cat([t["moments"] for t in parts], dim=1).view(torch.int32), whole["moments"].view(torch.int32))
    assert torch.equal(torch.cat([t["cells"] for t in parts]).view(torch.int32), whole["cells"].view(torch.int32))
    for name in ("state", "step", "logp"):
        assert torch.equal(torch.cat([t[name] for t in parts]), whole[name]), name
    mom = whole["moments"].cpu().numpy()
    miss = np.isnan(x)
    assert np.isfinite(mom[:, miss]).all() and np.isnan(mom[:, ~miss]).all() and bool(torch.isnan(whole["guard"]).all())
    assert np.isfinite(mom[:, -17:][:, miss[-17:]]).all() and (mom[2, -17:][miss[-17:]] > 0).any()


# ---- 5. nothing else is written
@pytest.mark.parametrize("c", [IR.CASES[0], IR.CASES[2], IR.CASES[6], dict(p=37, n=33, nh=5), IR.CASES[1]], ids=IR.case_id)
def test_only_the_missing_cells_are_written(c):
    """A store at a column c >= p of row r would land on the first cells of row r + 1 (or, from the last row, on the next plane or the
    guard band): every observed cell, the fully observed row among them, and the guard stay NaN; p = 61 and p = 37 end inside a tile."""
    import torch
    m, x, slot, k_slots = _setup(c)
    x[2:, :3] = 0.25      # (observed cells right behind every row's end)
    slot, k_slots = IR.slots_of(np.isnan(x))
    out = _run(_engine(m), x, IR.BURN, IR.KEEP, IR.LEAP, 77, True, slot=slot, k_slots=k_slots)
    mom = out["moments"].cpu().numpy()
    miss = np.isnan(x)
    assert np.isnan(mom[:, ~miss]).all() and np.isfinite(mom[:, miss]).all()
    assert np.isnan(mom[:, 1]).all() and not miss[1].any() and miss[0].all()
    assert bool(torch.isnan(out["guard"]).all()) and bool(torch.isnan(out["cells_guard"]).all())
    cells = _cells_of(out["cells"], c["n"], k_slots, IR.KEEP)
    used = _used(miss, k_slots)
    assert np.isfinite(cells[used]).all() and np.isnan(cells[~used]).all()


def test_hmc_sample_with_impute_returns_the_moments_and_no_draws():
    import torch
    r = _runs(0)
    out = r["eng"].hmc_sample(r["x"], IR.KEEP, IR.BURN, step_size=0.1, n_leapfrog=IR.LEAP, seed=77, row_adapt=0.75, impute=True)
    assert out["draws"] is None and tuple(out["moments"].shape) == (3,) + r["x"].shape
    assert torch.equal(out["moments"].view(torch.int32), r["fused"]["moments"].view(torch.int32))
    assert torch.equal(out["row_step"], r["fused"]["step"]) and torch.equal(out["state"], r["fused"]["state"])


# ---- 6. the class
@pytest.mark.parametrize("shared", [True, False], ids=["shared-pattern", "ragged"])
@pytest.mark.parametrize("p", [20, 61])
def test_class_fused_predict_against_the_blocked_route(tmp_path, p, shared):
    """The same seed through BGM.predict(row_adapt=True) in 32-row blocks and through fused_predict=True: the same chains, so the same
    predictive values; the fused mean is their float32 shifted sum.  d comes from the blocked route's own samples (return_samples)."""
    from bayesgm_amd.models import BGM
    n, burn, keep, L, seed, alpha = 70, 20, 60, 4, 5, 0.1
    m = _model(41, 10, p)
    if shared:
        x = np.random.RandomState(42).randn(n, p).astype(np.float32)
        x[:, [3, 17, p - 1]] = np.nan
    else:
        x = _data(n, p, 42, miss=IR.MISS)
    miss = np.isnan(x)
    k_slots = int(miss.sum(axis=1).max())
    model = BGM(_bgm_params(tmp_path, p), random_seed=0)
    model.set_weights(m["g"])
    a = dict(alpha=alpha, n_mcmc=keep, burn_in=burn, step_size=0.05, num_leapfrog_steps=L, seed=seed, row_adapt=True)
    blocked = 32 * 4 * keep * (10 + k_slots)
    imp_b, int_b = model.predict(x, max_draw_bytes=blocked, **a)
    steps_b = model.hmc_row_step_
    assert model.impute_sd_ is None
    full, _ = model.predict(x, max_draw_bytes=32 * 4 * keep * (10 + k_slots + p), return_samples=True, **a)
    assert np.array_equal(model.hmc_row_step_, steps_b)
    imp, interval = model.predict(x, fused_predict=True, **a)
    sd = model.impute_sd_
    assert np.array_equal(model.hmc_row_step_, steps_b) and model.hmc_row_leapfrog_ is None
    assert imp.shape == (n, p) and imp.dtype == np.float32 and sd.shape == (n, p) and sd.dtype == np.float32
    assert np.array_equal(imp[~miss], x[~miss]) and np.isnan(sd[~miss]).all() and np.isfinite(sd[miss]).all() and not np.isnan(imp).any()
    # the mean bound of _bgm_impute_ref without the values' own 2e-4: the values are the same
    x64 = full.astype(np.float64)
    d = x64 - x64[0]
    bound = IR.gamma(keep) * np.abs(d).mean(axis=0)
    err_b, err_64 = np.abs(imp.astype(np.float64) - imp_b), np.abs(imp - x64.mean(axis=0))
    print("p=%d %s: worst |fused - blocked| / bound %.3g, worst |fused - float64 mean of the samples| / bound %.3g, bound %.3g .. %.3g"
          % (p, "shared" if shared else "ragged", (err_b / bound)[miss].max(), (err_64 / bound)[miss].max(), bound[miss].min(), bound[miss].max()))
    assert (err_b <= bound)[miss].all()
    # the sd against the samples': the rounding terms of the variance bound (3 gamma_k sum d^2 / (k - 1)) and the sd's own float32
    # rounding (relative u on the sd: 2 u on the variance, 4 u allows for the products)
    var_bound = 3.0 * IR.gamma(keep) * (d * d).sum(axis=0) / (keep - 1) + 4.0 * IR.U * x64.var(axis=0, ddof=1)
    assert (np.abs(sd.astype(np.float64) ** 2 - x64.var(axis=0, ddof=1)) <= var_bound)[miss].all()
    # the interval is imputed -/+ z sd in the reference's layout
    z = np.float32(statistics.NormalDist().inv_cdf(1.0 - alpha / 2.0))
    lo, hi = imp - z * sd, imp + z * sd
    if shared:
        cols = np.where(miss[0])[0]
        assert isinstance(interval, np.ndarray) and interval.shape == (n, len(cols), 2) and int_b.shape == interval.shape
        assert np.array_equal(interval[..., 0], lo[:, cols]) and np.array_equal(interval[..., 1], hi[:, cols])
    else:
        assert isinstance(interval, list) and len(interval) == n and [len(v) for v in interval] == [len(v) for v in int_b]
        for row in range(n):
            cols = np.where(miss[row])[0]
            assert interval[row].shape == (len(cols), 2)
            assert np.array_equal(interval[row][:, 0], lo[row, cols]) and np.array_equal(interval[row][:, 1], hi[row, cols])
    # a normal interval around the same mean: it contains the mean and is as wide as 2 z sd
    assert model.last_acceptance_rate > 0.0


# ---- 7. refusals
def _buffers(eng, n, p):
    import torch
    dev = eng.device
    state, grad = (torch.empty((n, eng.q), device=dev) for _ in range(2))
    return state, torch.empty(n, device=dev), grad, torch.full((n,), 0.05, device=dev), torch.full((3, n, p), float("nan"), device=dev)


def test_general_width_and_split_precision_are_refused_by_name_and_the_handle_stays_usable():
    import torch
    from bayesgm_amd.engine import BgmEngine
    m = OB.init_model(3, 4, 20, g_units=(32, 32))
    eng = BgmEngine(20, 4, g_units=[32, 32])
    eng.set_weights(m["g"])
    x = torch.from_numpy(_data(33, 20, 12)).to(eng.device)
    state, logp, grad, step, mom = _buffers(eng, 33, 20)
    with pytest.raises(RuntimeError, match=r"hmc_run_rows_impute failed \(-4\).*fused imputation.*general-width"):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True, moments=mom)
    assert bool(torch.isnan(mom).all())
    out = eng.hmc_sample(x, 4, 4, step_size=0.02, n_leapfrog=2, seed=1)
    assert bool(torch.isfinite(out["draws"]).all())
    # split precision
    eng = _engine(_model(11, 10, 61))
    eng.set_precision("f16x3")
    x = torch.from_numpy(_data(33, 61, 12)).to(eng.device)
    state, logp, grad, step, mom = _buffers(eng, 33, 61)
    with pytest.raises(RuntimeError, match=r"hmc_run_rows_impute failed \(-4\).*fused imputation.*split precision"):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True, moments=mom)
    assert bool(torch.isnan(mom).all())
    eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state).all())
    eng.set_precision("fp32")
    eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True, moments=mom)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mom[:, torch.isnan(x)]).all())


def test_invalid_arguments_are_named():
    import ctypes as C
    import torch
    eng = _engine(_model(11, 10, 20))
    dev = eng.device
    n, p = 20, 20
    xn = _data(n, p, 12)
    x = torch.from_numpy(xn).to(dev)
    slot, k_slots = IR.slots_of(np.isnan(xn))
    slot = torch.from_numpy(slot).to(dev)
    state, logp, grad, step, mom = _buffers(eng, n, p)
    cells = torch.full((n * k_slots, 2), float("nan"), device=dev)

    def call(L=2, n_iters=4, **kw):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, n_iters, 2, L, 1, init=True, **kw)

    for kw, word in ((dict(moments=mom, cells=cells, k_slots=k_slots), "slot_dev"), (dict(moments=mom, n_keep=1), "n_keep"),
                     (dict(moments=mom, n_keep=0, n_iters=2), "n_keep"), (dict(moments=mom, max_trajectory=-0.5), "max_trajectory"),
                     (dict(moments=mom, jitter=2), "jitter"), (dict(moments=mom, L=0), "n_leapfrog"),
                     (dict(moments=mom, s_min=0.0), "s_min")):
        with pytest.raises(RuntimeError, match=r"hmc_run_rows_impute failed \(-1\).*" + word):
            call(**kw)
    # what the engine itself refuses: shapes that would let the kernel write out of bounds
    for kw, word in ((dict(cells=cells, slot=slot, k_slots=k_slots), "moments"), (dict(moments=mom[:, :-1]), "moments"),
                     (dict(moments=mom.double()), "moments"), (dict(moments=mom, cells=cells[:-1], slot=slot, k_slots=k_slots), "cells"),
                     (dict(moments=mom, cells=cells, slot=slot[:, :-1], k_slots=k_slots), "slot")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    # a NULL moments_dev at the C entry
    a = eng._hmc_args(x, state, logp, grad, step, 0, 4, 2, 2, 1, True, 0, None, None, None)
    rc = eng.lib.bgm_bgm_hmc_run_rows_impute(eng.h, C.byref(a), None, None, 0, 1e-4, 1e2, 0.0, 0, None, None, None, None, 0, 2, 1, None)
    assert rc == -1 and b"moments_dev" in eng.lib.bgm_last_error()
    assert bool(torch.isnan(mom).all()) and bool(torch.isnan(cells).all())
    call(moments=mom, cells=cells, slot=slot, k_slots=k_slots)      # and the engine still samples
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state).all()) and bool(torch.isfinite(mom[:, torch.isnan(x)]).all())
