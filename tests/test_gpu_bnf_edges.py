"""The default-shape Bayesian sampling kernels (csrc/bnf_kernels.h bnf_mh_kernel / bnf_effects_kernel, their split-precision form of
csrc/bnx_kernels.h, the host side csrc/bnf_api.hip / bnf_build.h) at the edges of their shape table, against oracle/bnn.py in float64
with the same Philox streams: every compiled first-layer instance and padded k-step, the first and last output tile counts, the
largest LDS footprint, the dispatch boundaries, the per-block proposal scale, fixed sigmas, a share of one block, and item queues that
are shorter than the XCD count or longer than the waves that serve them.  Cases and references: _bnf_edges_ref.py; their conditions
(few fragile rows, a moving sampler): test_bnf_edges_host.py.  Every case runs in fp32 and after set_precision("f16x3").

Bars (the family's own, test_gpu_bnf.py / test_gpu_bnx.py): log posterior 2e-5 max|ref| + 2e-3; Metropolis-Hastings states 1e-5 on the
rows whose accept decisions are not within 1e-3 of their uniform in the oracle, accepted counts within the number of such rows; ADRF
2e-4, ITE 1e-3, fused against stand-alone effects 1e-5."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import bnn as OB
import _bnf_edges_ref as E
from _bnf_edges_ref import f64
from test_gpu_bnf import _engine

pytestmark = pytest.mark.gpu

MODES = ("fp32", "f16x3")
ids = lambda cases: [c["name"] for c in cases]


@contextlib.contextmanager
def _session(m, mode="fp32", **kw):
    eng = _engine(m, **kw)
    try:
        if mode != "fp32":
            eng.set_precision(mode)
        yield eng
    finally:
        eng.close()


def _case_session(c, mode):
    return _session(E.setup(c)[0], mode, **(c["sigmas"] or {}))


def _T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the shared panels are read-only)


def _note(part, mode, what, err, bar, fragile=None):
    """One line per measured figure (pytest -s): the error, its bar and their ratio."""
    print("BNF-EDGE part=%s mode=%s %s err=%.3e bar=%.3e ratio=%.3f%s" % (part, mode, what, err, bar, err / bar,
                                                                          "" if fragile is None else " fragile=%d" % fragile))


def _lp_bar(ref):
    return 2e-5 * np.abs(ref).max() + 2e-3


def _check_logpost_values(part, mode, name, run, ref, eng):
    """run() -> log posterior under the engine's current precision; in split precision also the two checks of test_gpu_bnx.py."""
    got = run()
    e = np.abs(got - ref).max()
    _note(part, mode, "%s logpost" % name, e, _lp_bar(ref))
    assert e < _lp_bar(ref), e
    if mode != "fp32":
        eng.set_precision("fp32")
        got32 = run()
        eng.set_precision(mode)
        e32 = np.abs(got32 - ref).max()
        assert e < 4.0 * e32 + 1e-4 * (1.0 + np.abs(ref).max() * 1e-3), (e, e32)
        assert np.abs(got - got32).max() > 0.0          # the split kernels did run
    return got


def _check_logpost(part, c, mode):
    _, _, (z, x, y, v) = E.setup(c)
    with _case_session(c, mode) as eng:
        dev = eng.device
        args = (_T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev), _T(z, dev))
        run = lambda: eng.logpost(*args, c["bs"], E.LP_SEED, E.LP_STREAM, block0=E.LP_BLOCK0).cpu().numpy()
        _check_logpost_values(part, mode, c["name"], run, E.ref_logpost(c), eng)


def _run_mh(eng, c, x, y, v, z):
    """The case's iterations on the device -> (state, accepted count, accepted per (iteration, block))."""
    dev = eng.device
    n_blocks = (len(z) + c["bs"] - 1) // c["bs"]
    state = _T(z, dev)
    acc = torch.zeros(1, dtype=torch.int32, device=dev)
    accb = torch.zeros((c["n_iters"], n_blocks), dtype=torch.int32, device=dev)
    sdb = None if c["q_sd_blocks"] is None else _T(np.asarray(c["q_sd_blocks"], np.float32), dev)
    eng.mh_run(_T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev), state, c["bs"], it_begin=c["it_begin"], n_iters=c["n_iters"], burn_in=0,
               q_sd=c["q_sd"], seed=c["seed"], init=c["init"], row_base=c["row_base"], block0=c["block0"], acc_count=acc, acc_blocks=accb,
               q_sd_blocks=sdb)
    return state, int(acc[0]), accb.cpu().numpy()


def _check_mh(part, c, mode):
    _, _, (z, x, y, v) = E.setup(c)
    r = E.ref_mh(c)
    n, bs = c["n"], c["bs"]
    with _case_session(c, mode) as eng:
        state, n_acc, accb = _run_mh(eng, c, x, y, v, z)
    got = state.cpu().numpy()
    ok = ~r.fragile
    assert ok.sum() >= 0.98 * n
    e = np.abs(got[ok] - r.z[ok]).max()
    _note(part, mode, "%s mh" % c["name"], e, 1e-5, int(r.fragile.sum()))
    assert e < 1e-5, e
    assert abs(n_acc - int(r.acc.sum())) <= int(r.fragile.sum())
    assert int(accb.sum()) == n_acc
    for b in range(accb.shape[1]):          # per block: the oracle's count up to the block's own fragile rows
        lo, hi = b * bs, min(n, (b + 1) * bs)
        assert abs(int(accb[:, b].sum()) - int(r.acc[:, lo:hi].sum())) <= int(r.fragile[lo:hi].sum()), b


def _check_effects(part, c, mode):
    """test_gpu_bnf.test_mh_effects_match_oracle at the case's shape: kept draws and fused effects of the sampler, the stand-alone
    effects of the same draws, and the oracle evaluated on the kernel's own draws, with and without outcome noise."""
    _, m64, (z, x, y, v) = E.setup(c)
    binary, n, bs, burn, keep = c["binary"], c["n"], c["bs"], 2, 3
    seed = (2 << 32) | 555
    q = z.shape[1]
    xs = np.linspace(0.0, 3.0, 21).astype(np.float32)
    xv = [1.0, 0.0] if binary else f64(xs)
    with _case_session(c, mode) as eng:
        dev = eng.device
        state = torch.zeros(n, q, device=dev)
        draws = torch.zeros(keep, n, q, device=dev)
        adrf = torch.zeros(len(xs), keep, device=dev, dtype=torch.float64)
        ite = torch.zeros(n, keep, device=dev)
        eng.mh_run(_T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev), state, bs, 0, burn + keep, burn, 0.4, seed, init=True, row_base=40, block0=1,
                   draws=draws, n_keep=keep, effect=2 if binary else 1, sample_y=True, x_values=None if binary else _T(xs, dev),
                   adrf_sum=None if binary else adrf, ite=ite if binary else None)
        kw = dict(it0=burn, x_values=None if binary else xs, row_base=40, block0=1)
        alone = eng.effects(draws, bs, seed, sample_y=True, **kw).cpu().numpy()
        alone0 = eng.effects(draws, bs, seed, sample_y=False, **kw).cpu().numpy()
        dr, st = draws.cpu().numpy(), state.cpu().numpy()
        fused = ite.t().cpu().numpy() if binary else (adrf / n).float().cpu().numpy()
    e = np.abs(alone - fused).max()
    _note(part, mode, "%s fused-vs-alone" % c["name"], e, 1e-5)
    assert e < 1e-5
    init = OB.R.normals(np.arange(40, 40 + n), 0, q, OB.R.TAG_INIT, seed)
    assert np.abs(dr[-1] - st).max() == 0.0
    assert np.abs(dr[0] - init).max() < 10.0 and np.abs(dr[0] - dr[-1]).max() > 0.0
    bar = 1e-3 if binary else 2e-4
    worst = 0.0
    for d in range(keep):
        ref = OB.effects_draw(m64, f64(dr[d]), xv, d, burn + d, True, seed, bs, block0=1, row_base=40)
        worst = max(worst, np.abs(fused[d] - (ref[0] - ref[1])).max() if binary else np.abs(fused[:, d] - ref.mean(axis=1)).max())
    ref0 = OB.effects_draw(m64, f64(dr[1]), xv, 1, burn + 1, False, seed, bs, block0=1, row_base=40)
    worst0 = np.abs(alone0[1] - (ref0[0] - ref0[1])).max() if binary else np.abs(alone0[:, 1] - ref0.mean(axis=1)).max()
    _note(part, mode, "%s %s" % (c["name"], "ite" if binary else "adrf"), max(worst, worst0), bar)
    assert worst < bar and worst0 < bar, (worst, worst0)


# ---- A: every compiled first-layer instance of the sampler, every instance and padded step of the effects kernel -----------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", E.A_CASES, ids=ids(E.A_CASES))
def test_first_layer_instances_logpost(c, mode):
    _check_logpost("A", c, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", E.A_CASES, ids=ids(E.A_CASES))
def test_first_layer_instances_mh(c, mode):
    _check_mh("A", c, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", E.A_CASES + E.EFFECT_CASES, ids=ids(E.A_CASES + E.EFFECT_CASES))
def test_first_layer_instances_mh_with_effects(c, mode):
    _check_effects("A", c, mode)


# ---- B: output tiles of g, the largest LDS footprint -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", E.B_CASES, ids=ids(E.B_CASES))
def test_output_tile_and_lds_edges_logpost(c, mode):
    _check_logpost("B", c, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", E.B_CASES, ids=ids(E.B_CASES))
def test_output_tile_and_lds_edges_mh(c, mode):
    _check_mh("B", c, mode)


# ---- C: dispatch boundaries ---------------------------------------------------------------------------------------------------------
def _shape_case(z_dims, p, binary=False):
    return E.case("C-%s-p%d" % ("-".join(str(d) for d in z_dims), p), z_dims, p, 64, 24, binary=binary)


@pytest.mark.parametrize("z_dims,p", E.SERVED_SHAPES)
def test_shapes_inside_the_table_are_served(z_dims, p):
    assert E.plan(sum(z_dims), p, z_dims[0], z_dims[1]).served
    with _case_session(_shape_case(z_dims, p), "fp32") as eng:
        assert eng.serves_block_shares()
        assert eng.sampling_family() == "bnf"


def _check_refusals_outside_the_family(eng, c, args, z):
    """Split precision and a share of one block exist on the default-shape kernels only; a refusal leaves the session and the states as
    they were."""
    family = eng.sampling_family()
    assert family != "bnf" and not eng.serves_block_shares()
    with pytest.raises(RuntimeError, match="split precision exists on the default-shape"):
        eng.set_precision("f16x3")
    assert not eng.serves_block_shares()          # (a refused mode is not remembered)
    assert eng.sampling_family() == family
    state = _T(z[:10], eng.device)
    with pytest.raises(RuntimeError, match="share of one block"):
        eng.mh_run(args[0][:10].contiguous(), args[1][:10].contiguous(), args[2][:10].contiguous(), state, c["bs"], 0, 1, 0, 0.3, c["seed"],
                   block_row0=5)
    assert torch.equal(state, _T(z[:10], eng.device))


@pytest.mark.parametrize("z_dims,p", E.UNSERVED_SHAPES)
def test_shapes_outside_the_table_fall_back(z_dims, p):
    """p = 3, p = 208, q = 32 and the wide plan (q = 16, p = 176) leave the family.  Each of them passes bns_plan (bnn_sample_api.hip:
    hidden widths 64, inputs <= 208, at most 28 of the 32 sign words per row), so the batch-statistics kernels serve it in their
    inference-mode form: the log posterior meets the oracle at that family's bar (test_gpu_bnn.py); a share of one block and split
    precision exist on the default-shape kernels only."""
    c = _shape_case(z_dims, p)
    assert not E.plan(sum(z_dims), p, z_dims[0], z_dims[1]).served
    _, m64, (z, x, y, v) = E.setup(c)
    with _case_session(c, "fp32") as eng:
        dev = eng.device
        assert eng.sampling_family() == "bns"
        args = (_T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev))
        _check_refusals_outside_the_family(eng, c, args, z)
        assert eng.sampling_family() == "bns"
        got = eng.logpost(*args, _T(z, dev), c["bs"], E.LP_SEED, E.LP_STREAM, block0=E.LP_BLOCK0).cpu().numpy()
        ref = OB.log_posterior_blocks(m64, f64(x), f64(y), f64(v), f64(z), c["bs"], E.LP_SEED, E.LP_STREAM, block0=E.LP_BLOCK0)
        e = np.abs(got - ref).max()
        _note("C", "fp32", "%s fallback logpost" % c["name"], e, 2e-3 * np.abs(ref).max())
        assert e < 2e-3 * np.abs(ref).max(), e


def test_widths_outside_the_fragment_kernels_go_to_the_any_width_family():
    """g_units = [128, 96]: no LDS-fragment family holds a hidden width above 64, so the session samples on the any-width kernels
    (csrc/bnw_kernels.h) -- with the same two refusals as every session outside the default-shape family."""
    from test_gpu_bnf import _model, _panel
    units = dict(g_units=[128, 96])
    c = E.case("C-bnw", (1, 1, 1, 7), 20, 40, 24)
    m = _model(False, z_dims=c["z_dims"], p=c["p"], **units)
    z, x, y, v = _panel(m, c["n"])
    with _session(m, **units) as eng:
        assert eng.sampling_family() == "bnw"
        assert not eng.serves_block_shares()
        args = (_T(x[:, 0], eng.device), _T(y[:, 0], eng.device), _T(v, eng.device))
        _check_refusals_outside_the_family(eng, c, args, z)
        assert eng.sampling_family() == "bnw"


def test_sampling_family_needs_a_session():
    from bayesgm_amd.bnn_engine import BnnEngine
    eng = BnnEngine(50, (1, 1, 1, 7), False, kl_weight=1e-4, max_batch=32, norm_mode=1)
    try:
        with pytest.raises(RuntimeError, match="no session"):
            eng.sampling_family()
        assert not eng.serves_block_shares()
    finally:
        eng.close()


def test_the_capability_query_leaves_the_precision_alone():
    """serves_block_shares() asks the library for the session's family; it does not pass through the precision switch, so the
    remembered precision and the next log posterior are the ones from before the query."""
    c = _shape_case((1, 1, 1, 7), 50)
    _, _, (z, x, y, v) = E.setup(c)
    for mode in MODES:
        with _case_session(c, mode) as eng:
            dev = eng.device
            args = (_T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev), _T(z, dev))
            run = lambda: eng.logpost(*args, c["bs"], E.LP_SEED, E.LP_STREAM, block0=E.LP_BLOCK0)
            before, prec = run(), getattr(eng, "_precision", "fp32")
            assert prec == mode
            assert eng.serves_block_shares()
            assert getattr(eng, "_precision", "fp32") == prec
            assert torch.equal(run(), before)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_doses", E.DOSE_COUNTS)
def test_dose_counts(n_doses, mode):
    """Stand-alone effects of one draw with outcome noise: 1 dose, the 16-dose rounds of the lane-group-distributed noise and one past
    them, BNF_MAX_DOSES = 256; 257 doses leave the family (the batch-statistics effects kernel accumulates doses past its 256 LDS
    slots in global memory)."""
    c = E.case("C-doses", (1, 1, 1, 7), 50, 40, 24)
    _, m64, (z, _, _, _) = E.setup(c)
    seed = (2 << 32) | 555
    xs = np.linspace(0.0, 3.0, n_doses).astype(np.float32) if n_doses > 1 else np.array([1.5], np.float32)
    with _case_session(c, mode) as eng:
        got = eng.effects(_T(z[None], eng.device), c["bs"], seed, it0=3, x_values=xs, sample_y=True, row_base=40, block0=1).cpu().numpy()
        assert eng.sampling_family() == "bnf"          # (the one call that went elsewhere does not move the session)
    ref = OB.effects_draw(m64, f64(z), f64(xs), 0, 3, True, seed, c["bs"], block0=1, row_base=40).mean(axis=1)
    assert got.shape == (n_doses, 1)
    e = np.abs(got[:, 0] - ref).max()
    _note("C", mode, "doses=%d adrf" % n_doses, e, 2e-4)
    assert e < 2e-4, e


# ---- D: options -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_per_block_proposal_scale(mode):
    """q_sd_blocks = [0.1, 0.5, 1.0] over three blocks (the adaptive schedule of CausalBGM.predict always passes it); the scalar q_sd = 7
    must not be read."""
    _check_mh("D", E.D_SCALE, mode)


@pytest.mark.parametrize("mode", MODES)
def test_fixed_sigmas_at_the_family_bars(mode):
    """params['sigma_v' | 'sigma_x' | 'sigma_y'] on a binary treatment: log posterior, Metropolis-Hastings and the ITE with outcome
    noise at the default-shape kernels' own bars."""
    c = E.D_SIGMA
    _, m64, (z, x, y, v) = E.setup(c)
    _check_logpost("D", c, mode)
    free = dict(m64)
    for k in c["sigmas"]:
        free.pop(k)
    ref = E.ref_logpost(c)          # (the option is live: the variance heads give another value)
    assert np.abs(OB.log_posterior_blocks(free, f64(x), f64(y), f64(v), f64(z), c["bs"], E.LP_SEED, E.LP_STREAM, block0=E.LP_BLOCK0) - ref).max() > 1.0
    _check_mh("D", c, mode)
    seed, keep = (2 << 32) | 555, 2
    draws = np.stack([z, z[::-1].copy()])
    with _case_session(c, mode) as eng:
        got = eng.effects(_T(draws, eng.device), c["bs"], seed, it0=4, sample_y=True, row_base=40, block0=1).cpu().numpy()
    worst = 0.0
    for d in range(keep):
        r = OB.effects_draw(m64, f64(draws[d]), [1.0, 0.0], d, 4 + d, True, seed, c["bs"], block0=1, row_base=40)
        worst = max(worst, np.abs(got[d] - (r[0] - r[1])).max())
        rf = OB.effects_draw(free, f64(draws[d]), [1.0, 0.0], d, 4 + d, True, seed, c["bs"], block0=1, row_base=40)
        assert np.abs((rf[0] - rf[1]) - (r[0] - r[1])).max() > 0.05
    _note("D", mode, "%s ite" % c["name"], worst, 1e-3)
    assert worst < 1e-3, worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", E.D_SHARE, ids=ids(E.D_SHARE))
def test_a_share_of_one_block_equals_the_whole_block(c, mode):
    """One block of 100 rows (block 3, rows 500 ...), chains initialised by the kernel, 3 + 2 iterations with kept draws and fused
    effects: once whole, once as the shares [0, 37) and [37, 100) with block_row0 / row_base moved along.  bnf_api.hip: the result does
    not depend on how the block's rows are split -- states, draws and ITE bit for bit, the dose sums (added over the shares) at 1e-5."""
    _, _, (z, x, y, v) = E.setup(c)
    binary, n, bs, burn, keep = c["binary"], c["n"], c["bs"], 3, 2
    q = z.shape[1]
    xs = np.linspace(0.0, 3.0, 21).astype(np.float32)
    with _case_session(c, mode) as eng:
        dev = eng.device

        def run(lo, hi):
            m_ = hi - lo
            state = torch.zeros(m_, q, device=dev)
            draws = torch.zeros(keep, m_, q, device=dev)
            adrf = torch.zeros(len(xs), keep, device=dev, dtype=torch.float64)
            ite = torch.zeros(m_, keep, device=dev)
            acc = torch.zeros(1, dtype=torch.int32, device=dev)
            eng.mh_run(_T(x[lo:hi, 0], dev), _T(y[lo:hi, 0], dev), _T(v[lo:hi], dev), state, bs, 0, burn + keep, burn, c["q_sd"], c["seed"], init=True,
                       row_base=c["row_base"] + lo, block0=c["block0"], block_row0=lo, acc_count=acc, draws=draws, n_keep=keep,
                       effect=2 if binary else 1, sample_y=True, x_values=None if binary else _T(xs, dev), adrf_sum=None if binary else adrf,
                       ite=ite if binary else None)
            return state, draws, ite, adrf, int(acc[0])
        whole = run(0, n)
        a, b = run(0, 37), run(37, n)
    assert n // 4 <= whole[4] // (burn + keep) < n          # the chains moved
    assert torch.equal(torch.cat([a[0], b[0]]), whole[0])
    assert torch.equal(torch.cat([a[1], b[1]], dim=1), whole[1])
    assert a[4] + b[4] == whole[4]
    assert float((whole[1][0] - whole[1][-1]).abs().max()) > 0.0
    if binary:
        assert torch.equal(torch.cat([a[2], b[2]]), whole[2]) and float(whole[2].abs().max()) > 0.0
    else:
        e = float(((a[3] + b[3]) / n - whole[3] / n).abs().max())
        _note("D", mode, "%s adrf of shares" % c["name"], e, 1e-5)
        assert e < 1e-5 and float(whole[3].abs().max()) > 0.0


# ---- E: item queues ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [E.E_TINY, E.E_ONE], ids=ids([E.E_TINY, E.E_ONE]))
def test_short_item_queues(c, mode):
    """61 blocks of 2 rows (the API's minimum) with a last block of 1 row, and a single item: XCD queues with a handful of items, and
    with none."""
    _check_logpost("E", c, mode)
    _check_mh("E", c, mode)


@pytest.mark.parametrize("mode", MODES)
def test_more_items_than_waves(mode):
    """8 n_cus + 40 blocks of 2 rows, one item each: every XCD's queue is longer than the waves that serve it, so waves come back for
    a second item.  First, middle and last block against the oracle; the same blocks run alone, with their block id and row offset,
    give the same bits (rows are independent), as in test_full_size_panel_blocks_are_independent_sampler_runs."""
    x3 = mode != "fp32"
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = max(8, (n_cus // 8) * 8)          # grid_for (bnf_api.hip)
    c = E.many_case(n_cus, x3)
    n, bs = c["n"], c["bs"]
    n_blocks = n // bs
    P = E.plan(sum(c["z_dims"]), c["p"], c["z_dims"][0], c["z_dims"][1])
    n_items = n_blocks * E.groups_per_block(bs)
    assert n_items * (2 if x3 else 1) > 8 * grid          # (split precision: an item is two units)
    assert n_blocks * 2 * P.set_floats * 4 < 0.5e9
    _, m64, (z, x, y, v) = E.setup(c)
    blocks = E.many_blocks(c)
    rows = np.concatenate([np.arange(b * bs, (b + 1) * bs) for b in blocks])
    r = E.run_mh(c, m64, x, y, v, z, blocks=blocks)
    assert not r.fragile[rows].any()
    with _case_session(c, mode) as eng:
        dev = eng.device
        xd, yd, vd, zd = _T(x[:, 0], dev), _T(y[:, 0], dev), _T(v, dev), _T(z, dev)
        lp_dev = []          # the first run is the one in the session's own precision

        def run():
            lp_dev.append(eng.logpost(xd, yd, vd, zd, bs, E.LP_SEED, E.LP_STREAM, block0=E.LP_BLOCK0))
            return lp_dev[-1].cpu().numpy()[rows]
        ref = np.concatenate([OB.log_posterior_blocks(m64, f64(x[lo:lo + bs]), f64(y[lo:lo + bs]), f64(v[lo:lo + bs]), f64(z[lo:lo + bs]), bs,
                                                      E.LP_SEED, E.LP_STREAM, block0=E.LP_BLOCK0 + b) for b, lo in ((b, b * bs) for b in blocks)])
        _check_logpost_values("E", mode, c["name"], run, ref, eng)
        lp = lp_dev[0]
        state, n_acc, accb = _run_mh(eng, c, x, y, v, z)
        assert torch.isfinite(state).all() and torch.isfinite(lp).all()
        assert int(accb.sum()) == n_acc and n // 4 <= n_acc < n
        got = state.cpu().numpy()
        e = np.abs(got[rows] - r.z[rows]).max()
        _note("E", mode, "%s mh" % c["name"], e, 1e-5, 0)
        assert e < 1e-5, e
        for b in blocks:
            lo, hi = b * bs, (b + 1) * bs
            assert int(accb[:, b].sum()) == int(r.acc[:, lo:hi].sum())
            sub = zd[lo:hi].clone()
            eng.mh_run(xd[lo:hi].contiguous(), yd[lo:hi].contiguous(), vd[lo:hi].contiguous(), sub, bs, c["it_begin"], c["n_iters"], 0, c["q_sd"],
                       c["seed"], row_base=c["row_base"] + lo, block0=c["block0"] + b)
            assert torch.equal(sub, state[lo:hi])
            lp_b = eng.logpost(xd[lo:hi].contiguous(), yd[lo:hi].contiguous(), vd[lo:hi].contiguous(), zd[lo:hi].contiguous(), bs, E.LP_SEED,
                               E.LP_STREAM, block0=E.LP_BLOCK0 + b)
            assert torch.equal(lp_b, lp[lo:hi])
