"""BGM fused imputation with tail buffers (bgm_bgm_hmc_run_rows_impute_tails, BgmEngine.hmc_run_rows(tails=) / row_tail_quantiles /
hmc_sample(impute=True, tails=K), BGM.predict(fused_predict=True, interval='tails')) on the GPU.

Every bar is bit-identity: the tails are a selection of the run's own predictive values and the finisher applies the arithmetic of
bgm_row_mean_quantiles to them, so nothing is rounded differently on the two routes.  Cells and tails always come from ONE run.  The
buffers are NaN beforehand, with a NaN guard band behind the tails.  The cases are those of tests/_bgm_impute_ref.py (all six compiled
variants)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bgm_impute_ref as IR  # noqa: E402
from test_gpu_bgm import _bgm_params, _data, _engine, _model  # noqa: E402
from test_gpu_bgm_impute import CHAIN, GUARD, TRAJ, _setup  # noqa: E402

from oracle import bgm as OB  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

_ids = dict(ids=lambda i: IR.case_id(IR.CASES[i]))
LONG_I = IR.CASES.index(IR.LONG)
_ENG = {}


def _case(i):
    """(engine, x, slot, k_slots) of CASES[i], built once"""
    if i not in _ENG:
        m, x, slot, k_slots = _setup(IR.CASES[i])
        _ENG[i] = (_engine(m), x, slot, k_slots)
    return _ENG[i]


def _run(eng, x, slot, k_slots, burn, keep, L, seed, K=None, cuts=(), row_base=0, add_noise=True, traj=None, cells=True, stop=None):
    """One run of hmc_run_rows with moments (and cells, and with K the tails) over launches cut at `cuts`, up to iteration `stop`
    (default: all) -> dict of device tensors.  Every buffer is NaN beforehand; a NaN guard band lies behind the cells and the tails."""
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
    out["moments"] = torch.full((3, n, p), float("nan"), device=dev)
    kw = dict(moments=out["moments"], n_keep=keep, add_noise=add_noise, slot=torch.as_tensor(slot, dtype=torch.int32, device=dev).contiguous(),
              k_slots=k_slots)
    if cells:
        cbuf = torch.full((n * k_slots * keep + GUARD,), float("nan"), device=dev)
        out["cells"], out["cells_guard"] = cbuf[:n * k_slots * keep].view(n * k_slots, keep), cbuf[n * k_slots * keep:]
        kw.update(cells=out["cells"])
    if K is not None:
        size = 2 * K * n * k_slots
        tbuf = torch.full((size + GUARD,), float("nan"), device=dev)
        out["tails"], out["tails_guard"] = tbuf[:size].view(2, K, n, k_slots), tbuf[size:]
        kw.update(tails=out["tails"], k_tail=K)
    stop = total if stop is None else stop
    marks = [0] + [c for c in cuts if c < stop] + [stop]
    for a, b in zip(marks[:-1], marks[1:]):
        eng.hmc_run_rows(x, state, logp, grad, step, a, b - a, burn, L, seed, init=(a == 0), row_base=row_base, up=up, dn=dn,
                         acc_prob=acc_prob, acc_count=acc_count, n_steps=n_steps, **traj, **kw)
    torch.cuda.synchronize(dev)
    return out


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _used(x, k_slots):
    return np.arange(k_slots)[None, :] < np.isnan(x).sum(axis=1)[:, None]


def _set_check(out, x, k_slots, K, m, what=""):
    """check 2: as multisets tail 0 is the K smallest and tail 1 the K largest of every used series' cells; heap slot 0 is the threshold;
    nothing else of the buffer, nor the guard band, is written"""
    n = x.shape[0]
    cells = out["cells"].cpu().numpy().reshape(n, k_slots, m)
    tails = out["tails"].cpu().numpy()
    used = _used(x, k_slots)
    assert tails.shape == (2, K, n, k_slots), what
    srt = np.sort(cells[used], axis=-1)                       # [series, m]
    assert np.isfinite(srt).all(), what
    got = np.sort(tails[:, :, used], axis=1)                  # [2, K, series]
    assert np.array_equal(got[0].T, srt[:, :K]), what
    assert np.array_equal(got[1].T, srt[:, m - K:]), what
    assert np.array_equal(tails[0, 0][used], srt[:, K - 1]) and np.array_equal(tails[1, 0][used], srt[:, m - K]), what
    assert np.isnan(tails[:, :, ~used]).all() and np.isnan(out["tails_guard"].cpu().numpy()).all(), what
    return cells[used]


# ---- 1. the chain, the moments and the cells are the impute kernel's
@pytest.mark.parametrize("traj", [None, TRAJ], ids=["plain", "cap-jitter"])
@pytest.mark.parametrize("i", range(len(IR.CASES)), **_ids)
def test_chain_moments_and_cells_are_the_impute_kernels_bit_for_bit(i, traj):
    import torch
    eng, x, slot, k_slots = _case(i)
    plain = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, traj=traj)
    tails = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=3, traj=traj)
    for name in CHAIN + ("moments", "cells") + (("n_steps",) if traj else ()):
        assert torch.equal(_bits(plain[name]), _bits(tails[name])), name
    assert "tails" not in plain and int(plain["acc_count"].sum()) > 0 and bool(torch.isfinite(tails["state"]).all())
    no_cells = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=3, traj=traj, cells=False)      # the cells are not needed
    assert torch.equal(_bits(no_cells["tails"]), _bits(tails["tails"])) and torch.equal(_bits(no_cells["moments"]), _bits(tails["moments"]))


# ---- 2. the tails are the sorted cells
def _sets(i, m_ks, burn=IR.BURN):
    eng, x, slot, k_slots = _case(i)
    ties = 0
    for m, K in m_ks:
        for add_noise in (True, False):      # False: a rejected transition repeats the cell exactly
            out = _run(eng, x, slot, k_slots, burn, m, IR.LEAP, 77 + m, K=K, add_noise=add_noise)
            series = _set_check(out, x, k_slots, K, m, (m, K, add_noise))
            if not add_noise:
                ties += int((series[:, 1:] == series[:, :-1]).sum())
    return ties


@pytest.mark.parametrize("m_k", [(6, 6), (6, 1), (6, 3)], ids=lambda mk: "m%d-K%d" % mk)
@pytest.mark.parametrize("i", range(len(IR.CASES)), **_ids)
def test_tails_equal_the_sorted_cells_of_the_same_run(i, m_k):
    ties = _sets(i, [m_k])
    assert ties > 0 or IR.CASES[i]["n"] == 1      # (the runs without noise did hold repeated values; one chain of 5 transitions may not)


@pytest.mark.parametrize("m_k", [(40, 1), (40, 2), (400, 17)], ids=lambda mk: "m%d-K%d" % mk)
def test_tails_equal_the_sorted_cells_over_long_runs(m_k):
    assert _sets(LONG_I, [m_k]) > 0


def test_one_retained_draw():
    _sets(LONG_I, [(1, 1)])
    _sets(0, [(1, 1)])


# ---- 3. cuts and windows
@pytest.mark.parametrize("i", [0, 1, 3, 6], **_ids)
def test_launch_cuts_and_row_windows_leave_the_raw_buffers_unchanged(i):
    """K = 3 at m = 6, burn-in 4: the cuts every 4 iterations fall at retained draw 4 (after the fill), those every 1 inside it too"""
    import torch
    c = IR.CASES[i]
    eng, x, slot, k_slots = _case(i)
    total, K = IR.BURN + IR.KEEP, 3
    one = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=K)
    _set_check(one, x, k_slots, K, IR.KEEP)
    for every in (4, 1):
        cut = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=K, cuts=tuple(range(every, total, every)))
        for name in CHAIN[:5] + ("moments", "cells", "tails"):      # (NaN at the same untouched places: compared as bits)
            assert torch.equal(_bits(one[name]), _bits(cut[name])), (every, name)
    a, b = (7, c["n"] - 5) if c["n"] > 20 else (0, c["n"])
    win = _run(eng, x[a:b], slot[a:b], k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=K, row_base=a)
    assert torch.equal(_bits(win["tails"]), _bits(one["tails"][:, :, a:b].contiguous()))
    assert torch.equal(_bits(win["moments"]), _bits(one["moments"][:, a:b].contiguous()))


@pytest.mark.parametrize("p,waves", [(20, 8), (40, 12)])
def test_second_pass_and_ragged_last_tile(p, waves):
    """n = 16 x waves x CUs + 17: the first wave slots take a second row tile, the last tile is ragged; the tails of the rows of both
    passes are those of runs over row windows."""
    import torch
    eng = _engine(_model(11, 10, p))
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    n, burn, keep, L, seed, K = 16 * waves * cus + 17, 3, 3, 2, 4, 2
    x = _data(n, p, 12, miss=IR.MISS)
    x[-17:, ::2] = np.nan            # (the rows of the second pass differ from the first pass's)
    slot, k_slots = IR.slots_of(np.isnan(x))
    whole = _run(eng, x, slot, k_slots, burn, keep, L, seed, K=K)
    marks = [0, 16 * waves * cus // 3 + 5, n - 17 - 40, n]
    parts = [_run(eng, x[a:b], slot[a:b], k_slots, burn, keep, L, seed, K=K, row_base=a, cells=False) for a, b in zip(marks[:-1], marks[1:])]
    assert torch.equal(_bits(torch.cat([t["tails"] for t in parts], dim=2)), _bits(whole["tails"]))
    assert torch.equal(_bits(torch.cat([t["moments"] for t in parts], dim=1)), _bits(whole["moments"]))
    _set_check(whole, x, k_slots, K, keep)
    assert np.isfinite(whole["tails"][:, :, -17:].cpu().numpy()[:, :, _used(x[-17:], k_slots)]).all()


# ---- 4. nothing else is written
@pytest.mark.parametrize("c", [IR.CASES[0], IR.CASES[2], IR.CASES[6], dict(p=37, n=33, nh=5), IR.CASES[1]], ids=IR.case_id)
def test_only_the_series_of_missing_cells_are_written(c):
    """Unused slots of rows with fewer than k_slots missing cells, the fully observed row's series and the guard band stay NaN; p = 61
    and p = 37 end inside a tile (a push at a column c >= p would land on a neighbouring series); the burn-in writes nothing."""
    import torch
    m, x, slot, k_slots = _setup(c)
    x[2:, :3] = 0.25      # (observed cells right behind every row's end)
    slot, k_slots = IR.slots_of(np.isnan(x))
    eng = _engine(m)
    out = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=3)
    _set_check(out, x, k_slots, 3, IR.KEEP)
    tails = out["tails"].cpu().numpy()
    miss = np.isnan(x)
    used = _used(x, k_slots)
    assert not miss[1].any() and np.isnan(tails[:, :, 1]).all() and miss[0].all() and np.isfinite(tails[:, :, 0]).all()
    assert (~used).any() or c["n"] == 1
    assert np.isfinite(tails[:, :, used]).all() and np.isnan(tails[:, :, ~used]).all()
    assert bool(torch.isnan(out["tails_guard"]).all()) and bool(torch.isnan(out["cells_guard"]).all())
    mom = out["moments"].cpu().numpy()
    assert np.isnan(mom[:, ~miss]).all() and np.isfinite(mom[:, miss]).all()
    burn_only = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=3, stop=IR.BURN)
    assert bool(torch.isnan(burn_only["tails"]).all()) and bool(torch.isnan(burn_only["tails_guard"]).all())
    assert bool(torch.isnan(burn_only["moments"]).all()) and bool(torch.isfinite(burn_only["state"]).all())


# ---- 5. the finisher
@pytest.mark.parametrize("m,alpha", [(40, 0.05), (40, 0.5), (400, 0.05)])
def test_finisher_gives_the_bounds_of_row_mean_quantiles_on_the_cells(m, alpha):
    import torch
    eng, x, slot, k_slots = _case(LONG_I)
    K = HM.tail_size(alpha, m)
    assert 1 <= K - 1 and K + 1 <= m
    used = torch.from_numpy(_used(x, k_slots)).to(eng.device)
    q_lo, q_hi = alpha / 2.0, 1.0 - alpha / 2.0
    bounds = []
    for k in (K, K + 1, K - 1):
        out = _run(eng, x, slot, k_slots, IR.BURN, m, IR.LEAP, 78, K=k)
        _, lo_ref, hi_ref = eng.row_mean_quantiles(out["cells"], q_lo, q_hi)
        if k == K - 1:
            with pytest.raises(RuntimeError, match=r"bgm_row_tail_quantiles failed \(-1\).*k_tail must be in \[%d, m = %d\]" % (K, m)):
                eng.row_tail_quantiles(out["tails"], m, q_lo, q_hi)
            continue
        lo, hi = eng.row_tail_quantiles(out["tails"], m, q_lo, q_hi)
        assert tuple(lo.shape) == (x.shape[0], k_slots)
        assert torch.equal(lo[used], lo_ref.view(-1, k_slots)[used]) and torch.equal(hi[used], hi_ref.view(-1, k_slots)[used])
        assert bool(torch.isfinite(lo[used]).all()) and bool((lo[used] <= hi[used]).all())
        bounds.append((lo[used], hi[used]))
    assert torch.equal(bounds[0][0], bounds[1][0]) and torch.equal(bounds[0][1], bounds[1][1])      # K + 1 gives the same bounds


def test_hmc_sample_with_tails_returns_the_buffers_and_the_slot_map():
    import torch
    eng, x, slot, k_slots = _case(0)
    K = 3
    ref = _run(eng, x, slot, k_slots, IR.BURN, IR.KEEP, IR.LEAP, 77, K=K)
    out = eng.hmc_sample(x, IR.KEEP, IR.BURN, step_size=0.1, n_leapfrog=IR.LEAP, seed=77, row_adapt=0.75, impute=True, tails=K)
    assert out["draws"] is None and out["k_slots"] == k_slots and torch.equal(out["slot"].cpu(), torch.from_numpy(slot))
    used = torch.from_numpy(_used(x, k_slots)).to(eng.device)
    assert tuple(out["tails"].shape) == (2, K, x.shape[0], k_slots)
    assert torch.equal(out["tails"][:, :, used], ref["tails"][:, :, used]) and bool((out["tails"][:, :, ~used] == 0).all())
    assert torch.equal(_bits(out["moments"]), _bits(ref["moments"])) and torch.equal(out["state"], ref["state"])
    plain = eng.hmc_sample(x, IR.KEEP, IR.BURN, step_size=0.1, n_leapfrog=IR.LEAP, seed=77, row_adapt=0.75, impute=True)
    assert "tails" not in plain and "slot" not in plain
    for bad in (0, IR.KEEP + 1, 2.5, True):
        with pytest.raises(ValueError, match="tails must be an integer K"):
            eng.hmc_sample(x, IR.KEEP, IR.BURN, row_adapt=0.75, impute=True, tails=bad)
    with pytest.raises(ValueError, match="tails belongs to impute"):
        eng.hmc_sample(x, IR.KEEP, IR.BURN, row_adapt=0.75, tails=K)


# ---- 6. the class
@pytest.mark.parametrize("shared", [True, False], ids=["shared-pattern", "ragged"])
@pytest.mark.parametrize("p", [20, 61])
def test_class_interval_tails_is_the_default_routes_interval(tmp_path, p, shared):
    """The same seed through BGM.predict(row_adapt=True) (stored draws, sorted cells), fused_predict=True alone and interval='tails' in
    one block and in 32-row blocks: the bounds are the default route's, mean and sd are fused_predict's, bit for bit."""
    from bayesgm_amd.models import BGM
    from bayesgm_amd.models.bgm import impute_tails_block_rows
    n, burn, keep, L, seed, alpha = 70, 20, 40, 4, 5, 0.1
    m = _model(41, 10, p)
    if shared:
        x = np.random.RandomState(42).randn(n, p).astype(np.float32)
        x[:, [3, 17, p - 1]] = np.nan
    else:
        x = _data(n, p, 42, miss=IR.MISS)
    miss = np.isnan(x)
    k_slots = int(miss.sum(axis=1).max())
    K = HM.tail_size(alpha, keep)
    assert 1 < K < keep
    model = BGM(_bgm_params(tmp_path, p), random_seed=0)
    model.set_weights(m["g"])
    a = dict(alpha=alpha, n_mcmc=keep, burn_in=burn, step_size=0.05, num_leapfrog_steps=L, seed=seed, row_adapt=True)
    imp_d, int_d = model.predict(x, **a)
    steps_d = model.hmc_row_step_
    imp_f, _ = model.predict(x, fused_predict=True, **a)
    sd_f, steps_f = model.impute_sd_, model.hmc_row_step_
    assert model.impute_tail_blocks_ is None
    budget = 32 * 8 * K * k_slots
    assert impute_tails_block_rows(K, k_slots, budget) == 32
    for kw, blocks in ((dict(), 1), (dict(max_draw_bytes=budget), 3)):
        imp, interval = model.predict(x, fused_predict=True, interval="tails", **kw, **a)
        assert model.impute_tail_blocks_ == blocks
        assert np.array_equal(imp, imp_f) and np.array_equal(model.impute_sd_, sd_f, equal_nan=True)
        assert np.array_equal(model.hmc_row_step_, steps_f) and np.array_equal(steps_f, steps_d)
        assert np.array_equal(imp[~miss], x[~miss]) and not np.isnan(imp).any()
        if shared:
            assert isinstance(interval, np.ndarray) and interval.shape == (n, 3, 2) and interval.dtype == int_d.dtype
            assert np.array_equal(interval, int_d)
        else:
            assert isinstance(interval, list) and len(interval) == n
            for row in range(n):
                assert interval[row].shape == (int(miss[row].sum()), 2) and interval[row].dtype == int_d[row].dtype
                assert np.array_equal(interval[row], int_d[row]), row
    assert imp_d.shape == imp.shape and model.last_acceptance_rate > 0.0


def test_class_panel_without_nan_and_the_refusals(tmp_path):
    from bayesgm_amd.models import BGM
    p, n = 20, 40
    model = BGM(_bgm_params(tmp_path, p), random_seed=0)
    model.set_weights(_model(41, 10, p)["g"])
    x = np.random.RandomState(3).randn(n, p).astype(np.float32)
    a = dict(n_mcmc=8, burn_in=8, step_size=0.05, num_leapfrog_steps=2, seed=5, row_adapt=True)
    imp_d, int_d = model.predict(x, **a)
    imp, interval = model.predict(x, fused_predict=True, interval="tails", **a)
    assert isinstance(interval, np.ndarray) and interval.shape == int_d.shape == (n, 0, 2) and interval.dtype == int_d.dtype
    assert np.array_equal(imp, x) and np.array_equal(imp_d, x)
    x[::3, 5] = np.nan
    for kw, word in ((dict(interval="tails"), "needs fused_predict"), (dict(interval="normal"), "needs fused_predict"),
                     (dict(interval="quantile", fused_predict=True), "default route"), (dict(interval="hpd"), "'normal', 'quantile' or 'tails'"),
                     (dict(interval="tails", fused_predict=True, max_draw_bytes=0), "max_draw_bytes")):
        with pytest.raises(ValueError, match=word):
            model.predict(x, **dict(a, **kw))
    _, int_q = model.predict(x, interval="quantile", **a)
    _, int_t = model.predict(x, interval="tails", fused_predict=True, **a)
    _, int_n = model.predict(x, interval="normal", fused_predict=True, **a)
    _, int_f = model.predict(x, fused_predict=True, **a)
    assert all(np.array_equal(u, v) for u, v in zip(int_q, int_t)) and all(np.array_equal(u, v) for u, v in zip(int_n, int_f))


# ---- 7. refusals
def _buffers(eng, n, p, k_slots, K):
    import torch
    dev = eng.device
    state, grad = (torch.empty((n, eng.q), device=dev) for _ in range(2))
    return (state, torch.empty(n, device=dev), grad, torch.full((n,), 0.05, device=dev), torch.full((3, n, p), float("nan"), device=dev),
            torch.full((2, K, n, k_slots), float("nan"), device=dev))


def test_invalid_arguments_are_named():
    import ctypes as C
    import torch
    eng = _engine(_model(11, 10, 20))
    dev = eng.device
    n, p, K = 20, 20, 2
    xn = _data(n, p, 12)
    x = torch.from_numpy(xn).to(dev)
    slot_np, k_slots = IR.slots_of(np.isnan(xn))
    slot = torch.from_numpy(slot_np).to(dev)
    state, logp, grad, step, mom, tails = _buffers(eng, n, p, k_slots, K)

    def call(L=2, n_iters=4, **kw):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, n_iters, 2, L, 1, init=True, **kw)

    ok = dict(moments=mom, slot=slot, k_slots=k_slots, tails=tails, k_tail=K)
    # the library's refusals: those of bgm_bgm_hmc_run_rows_impute first, then k_tail
    big = torch.full((2, 3, n, k_slots), float("nan"), device=dev)
    for kw, word in ((dict(n_keep=1), "n_keep"), (dict(max_trajectory=-0.5), "max_trajectory"), (dict(jitter=2), "jitter"), (dict(L=0), "n_leapfrog"),
                     (dict(s_min=0.0), "s_min"), (dict(tails=big, k_tail=3), r"k_tail must be in \[1, n_keep = 2\]; got 3")):
        with pytest.raises(RuntimeError, match=r"hmc_run_rows_impute_tails failed \(-1\).*" + word):
            call(**dict(ok, **kw))
    # at the C entry: NULL tails_dev, NULL slot_dev, k_slots < 1, k_tail < 1, and NULL moments_dev before them
    a = eng._hmc_args(x, state, logp, grad, step, 0, 4, 2, 2, 1, True, 0, None, None, None)
    fn = eng.lib.bgm_bgm_hmc_run_rows_impute_tails
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for args, word in (((P(mom), None, P(slot), k_slots, 2, 1, None, K), b"tails_dev"), ((P(mom), None, None, k_slots, 2, 1, P(tails), K), b"slot_dev"),
                       ((P(mom), None, P(slot), 0, 2, 1, P(tails), K), b"k_slots"), ((P(mom), None, P(slot), k_slots, 2, 1, P(tails), 0), b"k_tail"),
                       ((None, None, P(slot), k_slots, 2, 1, None, 0), b"moments_dev")):
        rc = fn(eng.h, C.byref(a), None, None, 0, 1e-4, 1e2, 0.0, 0, None, *args, None)
        assert rc == -1 and word in eng.lib.bgm_last_error() and b"bgm_bgm_hmc_run_rows_impute_tails" in eng.lib.bgm_last_error(), word
    # what the engine itself refuses: shapes and a slot map that would let the kernel write out of bounds
    bad_slot = slot.clone()
    bad_slot[3, int(np.where(np.isnan(xn[3]))[0][0])] = k_slots
    for kw, word in ((dict(moments=None), "tails needs moments"), (dict(slot=None), "tails needs moments, slot"), (dict(k_slots=0), "k_slots >= 1"),
                     (dict(tails=tails[:, :, :-1]), "tails must be a contiguous"), (dict(tails=tails.double()), "tails must be a contiguous"),
                     (dict(k_tail=K + 1), "tails must be a contiguous"), (dict(tails=None), "k_tail belongs to tails"),
                     (dict(tails=tails[:, :0], k_tail=0), "k_tail >= 1"), (dict(slot=bad_slot), "slot holds an entry >= k_slots")):
        with pytest.raises(ValueError, match=word):
            call(**dict(ok, **kw))
    assert bool(torch.isnan(mom).all()) and bool(torch.isnan(tails).all())
    call(**ok)      # and the engine still samples
    torch.cuda.synchronize()
    miss = torch.isnan(x)
    assert bool(torch.isfinite(state).all()) and bool(torch.isfinite(mom[:, miss]).all())
    used = torch.from_numpy(_used(xn, k_slots)).to(dev)
    assert bool(torch.isfinite(tails[:, :, used]).all()) and bool(torch.isnan(tails[:, :, ~used]).all())


def test_general_width_and_split_precision_are_refused_by_name_and_the_handle_stays_usable():
    import torch
    from bayesgm_amd.engine import BgmEngine
    m = OB.init_model(3, 4, 20, g_units=(32, 32))
    eng = BgmEngine(20, 4, g_units=[32, 32])
    eng.set_weights(m["g"])
    xn = _data(33, 20, 12)
    slot_np, k_slots = IR.slots_of(np.isnan(xn))
    x, slot = torch.from_numpy(xn).to(eng.device), torch.from_numpy(slot_np).to(eng.device)
    state, logp, grad, step, mom, tails = _buffers(eng, 33, 20, k_slots, 2)
    kw = dict(moments=mom, slot=slot, k_slots=k_slots, tails=tails, k_tail=2)
    with pytest.raises(RuntimeError, match=r"hmc_run_rows_impute_tails failed \(-4\).*fused imputation.*general-width"):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True, **kw)
    assert bool(torch.isnan(mom).all()) and bool(torch.isnan(tails).all())
    out = eng.hmc_sample(x, 4, 4, step_size=0.02, n_leapfrog=2, seed=1)
    assert bool(torch.isfinite(out["draws"]).all())
    # split precision
    eng = _engine(_model(11, 10, 61))
    eng.set_precision("f16x3")
    xn = _data(33, 61, 12)
    slot_np, k_slots = IR.slots_of(np.isnan(xn))
    x, slot = torch.from_numpy(xn).to(eng.device), torch.from_numpy(slot_np).to(eng.device)
    state, logp, grad, step, mom, tails = _buffers(eng, 33, 61, k_slots, 2)
    kw = dict(moments=mom, slot=slot, k_slots=k_slots, tails=tails, k_tail=2)
    with pytest.raises(RuntimeError, match=r"hmc_run_rows_impute_tails failed \(-4\).*fused imputation.*split precision"):
        eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True, **kw)
    assert bool(torch.isnan(mom).all()) and bool(torch.isnan(tails).all())
    eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state).all())
    eng.set_precision("fp32")
    eng.hmc_run_rows(x, state, logp, grad, step, 0, 4, 2, 2, 1, init=True, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mom[:, torch.isnan(x)]).all()) and bool(torch.isfinite(tails[:, :, 0, :int(np.isnan(xn[0]).sum())]).all())
