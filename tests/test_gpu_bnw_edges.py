"""The any-width Bayesian sampling kernels (csrc/bnw_kernels.h bnw_rows_kernel / bnw_effects_kernel / bnw_stats_kernel and their layer
product bnw_gemm2 / bnw_gemm2_narrow, host side csrc/bnw_api.hip) at the edges of their run-time branches, against oracle/bnn.py in
float64 with the same Philox streams.  A: the layer product -- widths that are no multiple of 4 (element-wise fetch, misaligned weight
offsets), hidden layers of at most 32 columns (the K-split kernel, one and two column tiles), 129 / 257 / 301 columns (a second and third
pass), one chunk of K, odd and even chunk counts, seven hidden layers, 300 inputs, 80 latents; each with inference-mode normalisation and
with batch statistics.  B: more items than workgroups, blocks of one to three rows, whole-block ranges of a call run alone, two and three
statistics workgroups per block, the per-block proposal scale.  C: the limits (64 latent columns under batch statistics, split precision,
eight hidden layers), each with the session usable afterwards.  Cases and references: _bnw_edges_ref.py; what each case reaches and the
conditions on its inputs: test_bnw_edges_host.py.

Bars (the project's own, none fitted to these kernels): log posterior 2e-5 max|ref| + 2e-3 (test_gpu_bnf.py: the default-shape kernels
compute the same function); Metropolis-Hastings states 1e-5 on the rows whose accept decisions are not within 1e-3 of their uniform in the
oracle, accepted counts within the number of such rows; ADRF 2e-4, ITE 1e-3; evaluate as test_gpu_bnn.py (z 2e-3 max(1, |z|), sums 1e-3 /
2e-3 relative, dose grid 5e-4, ITE 2e-3).  No case has a bar of its own.  Every check prints a BNW-EDGE line (pytest -s)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import bnn as OB
import _bnw_edges_ref as W
from _bnw_edges_ref import f64
from test_gpu_bnn import _engine

pytestmark = pytest.mark.gpu

ids = lambda cases: [c["name"] for c in cases]


@contextlib.contextmanager
def _session(c, units=None):
    eng = _engine(W.setup(c)[0], norm_mode=1 if c["fixed"] else 0, **(units or c["units"]))
    try:
        assert eng.sampling_family() == "bnw"
        yield eng
    finally:
        eng.close()


def _T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the shared panels are read-only)


def _note(part, name, what, err, bar, fragile=None):
    """One line per measured figure (pytest -s): the error, its bar and their ratio."""
    print("BNW-EDGE part=%s case=%s %s err=%.3e bar=%.3e ratio=%.3f%s" % (part, name, what, err, bar, err / bar,
                                                                          "" if fragile is None else " fragile=%d" % fragile))


def _lp_bar(ref):
    return 2e-5 * np.abs(ref).max() + 2e-3


def _panel_on(eng, c):
    _, _, (z, x, y, v) = W.setup(c)
    dev = eng.device
    return _T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev), _T(z, dev)


def _logpost(eng, c, args, lo=0, hi=None):
    """The log posterior of rows [lo, hi) of the case (whole blocks), as a call of their own."""
    a = [t[lo:hi].contiguous() for t in args]
    return eng.logpost(*a, c["bs"], W.LP_SEED, W.LP_STREAM, block0=W.LP_BLOCK0 + lo // c["bs"])


def _check_logpost(part, c, eng):
    ref = W.ref_logpost(c)
    got = _logpost(eng, c, _panel_on(eng, c)).cpu().numpy()
    e = np.abs(got - ref).max()
    _note(part, c["name"], "logpost", e, _lp_bar(ref))
    assert e < _lp_bar(ref), (e, int(np.abs(got - ref).argmax()))


def _run_mh(eng, c, args, lo=0, hi=None):
    """The case's iterations on rows [lo, hi) (whole blocks) -> (state, accepted count, accepted per (iteration, block))."""
    dev = eng.device
    x, y, v, z = [t[lo:hi].contiguous() for t in args]
    b0, n_blocks = lo // c["bs"], (len(z) + c["bs"] - 1) // c["bs"]
    state = z.clone()
    acc = torch.zeros(1, dtype=torch.int32, device=dev)
    accb = torch.zeros((c["n_iters"], n_blocks), dtype=torch.int32, device=dev)
    sdb = None if c["q_sd_blocks"] is None else _T(np.asarray(c["q_sd_blocks"][b0:b0 + n_blocks], np.float32), dev)
    eng.mh_run(x, y, v, state, c["bs"], it_begin=c["it_begin"], n_iters=c["n_iters"], burn_in=0, q_sd=c["q_sd"], seed=c["seed"], init=c["init"],
               row_base=c["row_base"] + lo, block0=c["block0"] + b0, acc_count=acc, acc_blocks=accb, q_sd_blocks=sdb)
    return state, int(acc[0]), accb.cpu().numpy()


def _check_mh(part, c, eng):
    r = W.ref_mh(c)
    n, bs = c["n"], c["bs"]
    state, n_acc, accb = _run_mh(eng, c, _panel_on(eng, c))
    got = state.cpu().numpy()
    ok = ~r.fragile
    assert ok.sum() >= 0.98 * n
    e = np.abs(got[ok] - r.z[ok]).max()
    _note(part, c["name"], "mh", e, 1e-5, int(r.fragile.sum()))
    assert e < 1e-5, e
    assert abs(n_acc - int(r.acc.sum())) <= int(r.fragile.sum())
    assert int(accb.sum()) == n_acc
    for b in range(accb.shape[1]):          # per block: the oracle's count up to the block's own fragile rows
        lo, hi = b * bs, min(n, (b + 1) * bs)
        assert abs(int(accb[:, b].sum()) - int(r.acc[:, lo:hi].sum())) <= int(r.fragile[lo:hi].sum()), b


def _effects(eng, c, draws, lo=0, hi=None):
    """Stand-alone effects with outcome noise of the draws' rows [lo, hi) (whole blocks): ITE [n_keep, rows] | ADRF [n_doses, n_keep]."""
    d = draws[:, lo:hi].contiguous()
    return eng.effects(d, c["bs"], W.EFF_SEED, it0=W.EFF_IT0, x_values=None if c["binary"] else W.EFF_DOSES, sample_y=True,
                       row_base=W.EFF_ROW_BASE + lo, block0=W.EFF_BLOCK0 + lo // c["bs"])


def _check_effects(part, c, eng):
    _, _, (z, _, _, _) = W.setup(c)
    got = _effects(eng, c, _T(W.effect_draws(z), eng.device)).cpu().numpy()
    ref = W.ref_effects(c)
    assert got.shape == ref.shape
    e, bar = np.abs(got - ref).max(), 1e-3 if c["binary"] else 2e-4
    _note(part, c["name"], "ite" if c["binary"] else "adrf", e, bar)
    assert e < bar, e


def _check_evaluate(part, c, eng):
    _, _, (_, x, y, v) = W.setup(c)
    n, p, dev = c["n"], c["p"], eng.device
    r = W.ref_evaluate(c)
    zt, sums, causal = eng.evaluate(_T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev), None, x_values=W.EVAL_DOSES, seed=W.EVAL_SEED, stream_id=W.EVAL_STREAM)
    s = sums.cpu().numpy()
    figures = [("evaluate z", np.abs(zt.cpu().numpy() - r.z).max(), 2e-3 * max(1.0, np.abs(r.z).max())),
               ("evaluate mse_v", abs(s[0] / (n * p) - r.mse_v), 1e-3 * r.mse_v),
               ("evaluate mse_x", abs(s[1] / n - r.mse_x), 2e-3 * r.mse_x),
               ("evaluate mse_y", abs(s[2] / n - r.mse_y), 2e-3 * r.mse_y),
               ("evaluate ite", np.abs(causal.cpu().numpy() - r.causal).max(), 2e-3) if c["binary"] else
               ("evaluate doses", np.abs(causal.cpu().numpy() / n - r.causal).max(), 5e-4)]
    for what, e, bar in figures:
        _note(part, c["name"], what, e, bar)
    for what, e, bar in figures:
        assert e < bar, (what, e, bar)


# ---- A: the layer product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.A_CASES, ids=ids(W.A_CASES))
def test_layer_product_edges_logpost_and_mh(c):
    with _session(c) as eng:
        _check_logpost("A", c, eng)
        _check_mh("A", c, eng)


@pytest.mark.parametrize("c", W.A_CASES, ids=ids(W.A_CASES))
def test_layer_product_edges_effects_and_evaluate(c):
    with _session(c) as eng:
        _check_effects("A", c, eng)
        _check_evaluate("A", c, eng)


# ---- B: rows, blocks and the item loop --------------------------------------------------------------------------------------------
def test_more_items_than_workgroups():
    """4 n_cus + 40 blocks of 2 rows, one item each, on a grid of 4 n_cus workgroups (bnw_plan): every workgroup of the row kernel and of
    the effects kernel comes back for a second item.  Log posterior of all rows, one Metropolis-Hastings iteration and the ITE of two
    draws on the first, a middle and the last block against the oracle."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = W.register(W.many_case(n_cus))
    n, bs = c["n"], c["bs"]
    n_blocks = n // bs
    assert (bs + W.RT - 1) // W.RT == 1 and n_blocks > 4 * n_cus          # n_items > the grid
    _, m64, (z, x, y, v) = W.setup(c)
    blocks = W.many_blocks(c)
    rows = np.concatenate([np.arange(b * bs, (b + 1) * bs) for b in blocks])
    r = W.run_mh(c, m64, x, y, v, z, blocks=blocks)
    assert not r.fragile[rows].any()
    draws = W.effect_draws(z)
    with _session(c) as eng:
        _check_logpost("B", c, eng)
        state, n_acc, accb = _run_mh(eng, c, _panel_on(eng, c))
        assert torch.isfinite(state).all()
        assert int(accb.sum()) == n_acc and 0 < n_acc < n
        e = np.abs(state.cpu().numpy()[rows] - r.z[rows]).max()
        _note("B", c["name"], "mh", e, 1e-5, 0)
        assert e < 1e-5, e
        for b in blocks:
            assert int(accb[:, b].sum()) == int(r.acc[:, b * bs:(b + 1) * bs].sum())
        ite = _effects(eng, c, _T(draws, eng.device)).cpu().numpy()
        assert np.isfinite(ite).all()
        worst = max(np.abs(ite[d, b * bs:(b + 1) * bs] - W.effects_of(c, m64, draws, d, b * bs, (b + 1) * bs)).max() for d in range(2) for b in blocks)
        _note("B", c["name"], "ite", worst, 1e-3)
        assert worst < 1e-3, worst


@pytest.mark.parametrize("c", W.B_TINY, ids=ids(W.B_TINY))
def test_blocks_smaller_than_a_tile(c):
    """Blocks of 3 rows and of 2 (the API's minimum) on 7 rows: the last block is one row."""
    with _session(c) as eng:
        _check_logpost("B", c, eng)
        _check_mh("B", c, eng)
        _check_effects("B", c, eng)
        args = _panel_on(eng, c)
        with pytest.raises(RuntimeError, match="bad argument"):          # a block is a batch of a network call: at least two rows
            eng.logpost(*args, 1, W.LP_SEED, W.LP_STREAM)
        _check_logpost("B", c, eng)


def test_whole_block_ranges_run_alone_reproduce_the_full_call():
    """Inference-mode normalisation: rows share only their block's perturbation, so the ranges [0, 70), [70, 210), [210, 230) of a call on
    blocks of 70 rows, run alone with block0 and row_base moved along, give the full call's bits: log posterior, the states after three
    iterations from chains the kernel initialises (init, it_begin = 0) with their accepted counts, and the ITE with outcome noise."""
    c = W.B_SHARE
    with _session(c) as eng:
        args = _panel_on(eng, c)
        lp = _logpost(eng, c, args)
        state, n_acc, accb = _run_mh(eng, c, args)
        draws = torch.stack([state, args[3]])
        ite = _effects(eng, c, draws)
        assert 0 < n_acc < c["n_iters"] * c["n"] and float((state - args[3]).abs().max()) > 0.0 and float(ite.abs().max()) > 0.0
        total = 0
        for lo, hi in W.B_SHARE_RANGES:
            assert torch.equal(_logpost(eng, c, args, lo, hi), lp[lo:hi]), (lo, hi)
            sub, sub_acc, sub_accb = _run_mh(eng, c, args, lo, hi)
            assert torch.equal(sub, state[lo:hi]), (lo, hi)
            assert np.array_equal(sub_accb, accb[:, lo // c["bs"]:lo // c["bs"] + sub_accb.shape[1]])
            total += sub_acc
            assert torch.equal(_effects(eng, c, draws, lo, hi), ite[:, lo:hi]), (lo, hi)
        assert total == n_acc


@pytest.mark.parametrize("c", W.B_STATS, ids=ids(W.B_STATS))
def test_several_statistics_workgroups_per_block(c):
    """Batch statistics of blocks of 257 and 600 rows: two and three workgroups of bnw_stats_kernel add to one block's fp64 sums."""
    with _session(c) as eng:
        _check_logpost("B", c, eng)
        _check_mh("B", c, eng)


@pytest.mark.parametrize("c", W.B_SCALE, ids=ids(W.B_SCALE))
def test_per_block_proposal_scale(c):
    """q_sd_blocks = [0.1, 0.5, 1.0] over three blocks; the scalar q_sd = 7 must not be read -- by the row kernel, nor by the statistics
    kernel that forms the same proposals under batch statistics."""
    with _session(c) as eng:
        _check_mh("B", c, eng)


# ---- C: limits ----------------------------------------------------------------------------------------------------------------------
def test_batch_statistics_hold_64_latent_columns():
    with _session(W.Q64) as eng:
        _check_logpost("C", W.Q64, eng)
        _check_mh("C", W.Q64, eng)
        _check_effects("C", W.Q64, eng)
        _check_evaluate("C", W.Q64, eng)


def test_a_65th_latent_column_is_refused_under_batch_statistics_only():
    fixed, batch = W.Q65
    with _session(batch) as eng:
        x, y, v, z = _panel_on(eng, batch)
        theta = eng.read(0)
        calls = [lambda: eng.logpost(x, y, v, z, batch["bs"], W.LP_SEED, W.LP_STREAM),
                 lambda: eng.mh_run(x, y, v, z, batch["bs"], 0, 1, 0, 0.3, batch["seed"]),
                 lambda: _effects(eng, batch, z[None]),
                 lambda: eng.evaluate(x, y, v, None, x_values=W.EVAL_DOSES, seed=W.EVAL_SEED, stream_id=W.EVAL_STREAM)]
        for call in calls + calls[:1]:
            with pytest.raises(RuntimeError, match="hold at most 64 latent columns"):
                call()
            assert eng.sampling_family() == "bnw"
        assert torch.equal(z, _panel_on(eng, batch)[3]) and np.array_equal(eng.read(0), theta)          # nothing was written
    with _session(fixed) as eng:          # the same nets with inference-mode normalisation
        _check_logpost("C", fixed, eng)
        _check_mh("C", fixed, eng)


def test_split_precision_is_refused_by_name():
    c = W.PRECISION
    with _session(c) as eng:
        args = _panel_on(eng, c)
        before = _logpost(eng, c, args)
        with pytest.raises(RuntimeError, match="split precision exists on the default-shape"):
            eng.set_precision("f16x3")
        assert eng.sampling_family() == "bnw" and getattr(eng, "_precision", "fp32") == "fp32"
        assert torch.equal(_logpost(eng, c, args), before)
        _check_logpost("C", c, eng)


def test_eight_hidden_layers_are_refused():
    """A net holds seven hidden layers (BNN_MAX_LAYERS = 8 Flipout layers): the driver refuses an eighth by name, the library refuses the
    configuration in bgm_bnn_begin -- which closes the session; the next begin with the seven-layer configuration serves it again."""
    from bayesgm_amd.bnn_engine import BnnEngine
    c = W.BY_NAME["W-deep/fixed"]
    m = W.setup(c)[0]
    with pytest.raises(ValueError, match="at most 7 hidden layers"):
        BnnEngine(c["p"], c["z_dims"], False, norm_mode=1, **W.DEEP8)
    with _session(c) as eng:
        args = _panel_on(eng, c)
        before = _logpost(eng, c, args)
        eng.cfg.n_hidden[0], eng.cfg.units[0][7] = 8, 72
        with pytest.raises(RuntimeError, match="bad configuration"):
            eng.begin(m)
        with pytest.raises(RuntimeError, match="no session"):
            eng.sampling_family()
        eng.cfg.n_hidden[0], eng.cfg.units[0][7] = 7, 0
        eng.begin(m)
        assert eng.sampling_family() == "bnw"
        assert torch.equal(_logpost(eng, c, args), before)
