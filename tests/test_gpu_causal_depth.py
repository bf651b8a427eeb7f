"""The LDS-resident CausalBGM kernels at every depth of g the host accepts (g_units = [64] * k, k = 1 .. 8), not only at the five layers
of the shipped configurations.  CausalMeta::n_gh = k - 1 is a run-time trip count in every family: k = 5 takes the scheduled asm block of
causal_kernels.h, every other k the generic loop; k = 1 enters no loop at all.  Five stays in the existing tests; here k is 1, 2, 4, 6, 8.

Shapes: the two smallest that select different code, both with a ragged last tile
    A  z_dims [1,1,1,7], p = 20, continuous, n = 40     KT1 = 1, NTL = 2, direct form of g's likelihood in MH
    B  z_dims [3,3,6,6], p = 50, binary,     n = 50     KT1 = 2, NTL = 7, Gram form in MH

What fits (the take() arithmetic of causal_pack_forward / hmc_prepare restated in _blob_bytes / _hmc_bytes below; the limit is 163 840 B):
    forward blob   A: 44 672 + 16 640 (k - 1) B, fits at every k (161 152 B at k = 8);  B: 77 760 + 16 640 (k - 1) B, fits up to k = 6
                   (160 960 B), refused at k = 7, 8.  The split-precision blob has the same size to the byte, the transposed fit blob and
                   the encoder blob of A and B are smaller, so on these shapes no family has a refusal of its own below the forward
                   blob's (at p = 200 the encoder's own check refuses e_units = [64] * 8: 174 144 B).
    HMC blob       A: 56 208 + 17 664 (k - 1) B, fits up to k = 7 (162 192 B, 1 648 B under the limit: the gradient and HMC tests run
                   it too), refused at k = 8;  B: 69 264 + 17 664 (k - 1) B, fits up
                   to k = 6 (157 584 B).
So every family has k < 5 and k > 5 on both shapes, and test_oversized_models_are_refused_by_name pins the refusals (B at k = 8 on every
sampling entry point, with and without a conditional prior; z_dims [1,1,1,7] with p = 200 at k = 6 and 8; HMC on A at k = 8; the encoder
at p = 200 with eight layers).  fit_begin does not refuse a model whose forward blob is too large and is not made to: by design
(bgm_causal_fit_begin, "chain_only") it is fitted by the row-tile chains or, with nine dense layers in g, by the general-width engine
(csrc/gx_fit_kernels.h); test_fit_of_a_model_without_a_resident_blob_matches_oracle runs both.  Split precision is covered for the
log-posterior kernel only.

Every bar is the one the five-layer test of the family uses (named at each test).  The chain tests compare with a float32 restatement
and count the rows that agree; that count is a condition on the CASE, checked on the CPU first: float32 against float64 restatement,
same seeds, rows of the last draw within 1e-4 (python tests/test_gpu_causal_depth.py prints the table; >= 98.5 % keeps a case):
    k   shape   MH 25+35   row-adaptive MH 25+35   conditional prior 30+10   HMC 8+8, L = 2
    1   A       100.0 %    100.0 %                 100.0 %                   100.0 %
    2   A       100.0 %    100.0 %                 100.0 %                   100.0 %
    4   A       100.0 %    100.0 %                 100.0 %                   100.0 %
    6   A       100.0 %    100.0 %                 100.0 %                   100.0 %
    7   A       -          -                       -                         100.0 %   (gradient / HMC only)
    8   A       100.0 %    100.0 %                 100.0 %                   -  (refused)
    1   B       100.0 %    100.0 %                 100.0 %                   100.0 %
    2   B       100.0 %    100.0 %                 100.0 %                   100.0 %
    4   B       100.0 %    100.0 %                 100.0 %                   100.0 %
    6   B       100.0 %    100.0 %                 100.0 %                   100.0 %
(n = 40 / 50: one row is 2.5 % / 2 %, so 98.5 % means every row.)

Asm block against generic loop (test_transparent_sixth_layer_equals_five_layers): a six-layer g whose last hidden layer is the
identity with zero bias behind positive activations (layer 4 with small weights and bias 0.5: every pre-activation of the panel is
positive in float64) computes the five-layer g exactly in exact arithmetic.  In the kernels the extra layer multiplies by 0.6f (1 + BGM_LRS) =
1 + 5e-8 and rounds twice, a relative 2e-7 on the activations, so the two log posteriors agree within the log-posterior bar
(2e-6 |ref| + 2e-4), not bit for bit; the test states that bar and nothing wider."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _causal_hmc_ref import hmc_sampler, log_posterior_and_grad  # noqa: E402
from _row_adapt_ref import row_adapt_sampler  # noqa: E402
from oracle import causal as OC  # noqa: E402
from oracle import fit as OF  # noqa: E402
from oracle import identifiable as OI  # noqa: E402
from oracle.nets import mlp_forward  # noqa: E402
from tests.test_gpu_causal import _data, _engine, _model  # noqa: E402

pytestmark = pytest.mark.gpu

DEPTHS = (1, 2, 4, 6, 8)
SHAPE_A = dict(name="A", z_dims=[1, 1, 1, 7], p=20, binary=False, n=40)
SHAPE_B = dict(name="B", z_dims=[3, 3, 6, 6], p=50, binary=True, n=50)
LDS_LIMIT = 160 * 1024


def _shape_tiles(s):
    """(KT1, NTL) of bgm_causal_shape (csrc/bgm_host.h)"""
    q1, need = sum(s["z_dims"]) + 1, (s["p"] + 1 + 15) // 16
    kt1 = 1 if q1 <= 12 else 2
    return kt1, (2 if need <= 2 else 7 if need <= 7 else 13 if kt1 == 1 else 10)


def _blob_bytes(k, s):
    """m.total * 4 of causal_pack_forward (csrc/causal_api.hip)"""
    kt1, ntl = _shape_tiles(s)
    return 4 * (3 * 16 * kt1 * 64 + 3 * 64 + (k - 1) * (4096 + 64) + 64 * 16 * ntl + 16 * ntl + 2 * (64 * 32 + 32 + 32 * 16 + 16 + 16 * 16 + 16) + 64)


def _hmc_bytes(k, s):
    """m.total * 4 of hmc_prepare (csrc/causal_hmc_api.hip): every weight block [out tile][in row][17]"""
    kt1, _ = _shape_tiles(s)
    tail = 2 * 64 * 17 + 32 + 32 * 17 + 16 + 16 * 17 + 16
    return 4 * (3 * 4 * 16 * kt1 * 17 + 3 * 64 + (k - 1) * (4 * 64 * 17 + 64) + 4 * 64 * 17 + 132 + 2 * tail)


def _fits(k, s):
    return _blob_bytes(k, s) <= LDS_LIMIT


def _hmc_fits(k, s):
    return _fits(k, s) and _hmc_bytes(k, s) <= LDS_LIMIT


GRID = [(k, s) for s in (SHAPE_A, SHAPE_B) for k in DEPTHS if _fits(k, s)]
# the gradient / HMC kernels also at k = 7 on A: the deepest model their blob holds (162 192 B of the 163 840), and the last of the
# CHMC_MAX_GH guarded trips of causal_hmc_kernels.h
HMC_EDGE = (7, SHAPE_A)
HMC_GRID = sorted([(k, s) for k, s in GRID if _hmc_fits(k, s)] + [HMC_EDGE], key=lambda c: (c[1]["name"], c[0]))
GRAD_GRID = GRID + [HMC_EDGE]
_ids = lambda grid: ["k%d-%s" % (k, s["name"]) for k, s in grid]  # noqa: E731


def test_the_grid_is_the_one_the_docstring_states():
    assert [(k, s["name"]) for k, s in GRID] == [(k, "A") for k in DEPTHS] + [(k, "B") for k in (1, 2, 4, 6)]
    assert [(k, s["name"]) for k, s in HMC_GRID] == [(k, "A") for k in (1, 2, 4, 6, 7)] + [(k, "B") for k in (1, 2, 4, 6)]
    assert _hmc_fits(*HMC_EDGE) and not _hmc_fits(8, SHAPE_A) and LDS_LIMIT - _hmc_bytes(*HMC_EDGE) == 1648
    assert (_blob_bytes(8, SHAPE_A), _blob_bytes(6, SHAPE_B), _hmc_bytes(7, SHAPE_A), _hmc_bytes(8, SHAPE_A)) == (161152, 160960, 162192, 179856)
    for fam in (GRID, HMC_GRID):
        for s in (SHAPE_A, SHAPE_B):
            assert any(k < 5 for k, t in fam if t is s) and any(k > 5 for k, t in fam if t is s)


def _deep(seed, k, s, **kw):
    return _model(seed, s["z_dims"], s["p"], s["binary"], g_units=(64,) * k, **kw)


def _eng(m, k, **kw):
    return _engine(m, g_units=[64] * k, **kw)


def _table(burn, target):
    from bayesgm_amd.row_adapt import row_adapt_factors
    return row_adapt_factors(burn, target)


def _f64(m, *arrs):
    return (OC.cast_model(m, np.float64),) + tuple(a.astype(np.float64) for a in arrs)


# the chain cases: one place for the GPU tests and for the CPU agreement table of the docstring
MH = dict(burn=25, keep=35, q_sd=0.3, seed=1234567890123)
PRIOR = dict(burn=30, keep=10, q_sd=0.4, seed=77, k=7)
HMC = dict(burn=8, keep=8, L=2, step0=0.1, seed=1234567890123, target=0.75)


def _chain_case(k, s):
    return _deep(21, k, s), _data(s["n"], s["p"], 22, s["binary"])


def _prior_case(k, s):
    rs = np.random.RandomState(3)
    m = _deep(5, k, s)
    q = sum(s["z_dims"])
    data = _data(s["n"], s["p"], 6, s["binary"])
    z = rs.randn(s["n"], q).astype(np.float32)
    seg = rs.randint(0, PRIOR["k"], s["n"])
    pn = [(W, (0.3 * rs.randn(*b.shape)).astype(np.float32)) for W, b in OI.init_prior_net(rs, PRIOR["k"], q)]
    mu, s2, _ = OI.prior_params([(W.astype(np.float64), b.astype(np.float64)) for W, b in pn], seg)
    return m, data, z, seg, OI.prior_table(pn, q), mu, s2


# ---------------------------------------------------------------------------------------------------------------------
# log posterior and its gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", GRAD_GRID, ids=_ids(GRAD_GRID))
def test_logpost_and_gradient_match_float64(k, s):
    """bars: tests/test_gpu_causal.py::test_logpost_matches_oracle; tests/test_gpu_causal_hmc.py::test_logpost_grad_matches_float64"""
    m = _deep(1, k, s)
    x, y, v = _data(s["n"], s["p"], 2, s["binary"])
    z = np.random.RandomState(3).randn(s["n"], sum(s["z_dims"])).astype(np.float32)
    eng = _eng(m, k)
    m64, x64, y64, v64, z64 = _f64(m, x, y, v, z)
    ref = OC.log_posterior(m64, x64, y64, v64, z64)
    got = eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()
    err = np.abs(got - ref)
    print("k = %d, %s: logpost worst err / bar %.3f" % (k, s["name"], (err / (2e-6 * np.abs(ref) + 2e-4)).max()))
    assert np.all(err <= 2e-6 * np.abs(ref) + 2e-4), (err.max(), np.abs(ref).max())
    if not _hmc_fits(k, s):
        return
    lp, gr = eng.logpost_grad(x.ravel(), y.ravel(), v, z)
    lp, gr = lp.cpu().numpy(), gr.cpu().numpy()
    ref_lp, ref_gr = log_posterior_and_grad(m64, x64, y64, v64, z64)
    assert np.abs(ref_lp - ref).max() <= 1e-9 * np.abs(ref).max()
    err, gmax, gerr = np.abs(lp - ref_lp), np.abs(ref_gr).max(axis=1), np.abs(gr - ref_gr).max(axis=1)
    print("k = %d, %s: logpost_grad worst value err / bar %.3f, worst gradient err / (5e-5 max|grad|) %.3f"
          % (k, s["name"], (err / (2e-6 * np.abs(ref_lp) + 2e-4)).max(), (gerr / (5e-5 * gmax)).max()))
    assert np.all(err <= 2e-6 * np.abs(ref_lp) + 2e-4), (err.max(), np.abs(ref_lp).max())
    assert np.all(gerr <= 5e-5 * gmax), (gerr / gmax).max()


def _positive_layer4(m5, z):
    """layer 4 with pre-activations in about [0.1, 0.9] on these rows: its weights scaled down until |W h| <= 0.4, its bias set to 0.5.
    (Raising the bias of the random layer instead needs a lift of about 5, which puts log sigma_v^2 into the regime where the log
    posterior amplifies the fp32 error of EVERY kernel, the five-layer one included, to the bar itself.)"""
    m64 = OC.cast_model(m5, np.float64)
    h = z.astype(np.float64)
    for W, b in m64["g"][:4]:
        h = h @ W + b
        h = np.where(h > 0, h, 0.2 * h)
    W4 = (m5["g"][4][0] * np.float32(0.4 / np.abs(h @ m64["g"][4][0]).max())).astype(np.float32)
    m5["g"][4] = (W4, np.full(64, 0.5, np.float32))
    pre = h @ W4.astype(np.float64) + 0.5
    assert pre.min() >= 0.05
    return m5


@pytest.mark.parametrize("s", [SHAPE_A, SHAPE_B], ids=["A", "B"])
def test_transparent_sixth_layer_equals_five_layers(s):
    """n_gh = 4 runs dense_hidden4_asm, n_gh = 5 the generic loop; same function, see the module docstring.  Bar: the log-posterior bar."""
    x, y, v = _data(s["n"], s["p"], 12, s["binary"])
    z = np.random.RandomState(13).randn(s["n"], sum(s["z_dims"])).astype(np.float32)
    m5 = _positive_layer4(_deep(11, 5, s), z)
    m6 = dict(m5)
    m6["g"] = m5["g"][:5] + [(np.eye(64, dtype=np.float32), np.zeros(64, np.float32))] + m5["g"][5:]
    m64, x64, y64, v64, z64 = _f64(m5, x, y, v, z)
    ref = OC.log_posterior(m64, x64, y64, v64, z64)
    assert np.array_equal(ref, OC.log_posterior(OC.cast_model(m6, np.float64), x64, y64, v64, z64))      # exact in float64
    lp5 = _eng(m5, 5).logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()
    lp6 = _eng(m6, 6).logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()
    bar = 2e-6 * np.abs(ref) + 2e-4
    print("%s: |lp6 - lp5| / bar %.3f, |lp5 - f64| / bar %.3f, |lp6 - f64| / bar %.3f; |ref| median %.3g"
          % (s["name"], (np.abs(lp6 - lp5) / bar).max(), (np.abs(lp5 - ref) / bar).max(), (np.abs(lp6 - ref) / bar).max(), np.median(np.abs(ref))))
    assert np.all(np.abs(lp5 - ref) <= bar) and np.all(np.abs(lp6 - ref) <= bar)
    assert np.all(np.abs(lp6 - lp5) <= bar)


# ---------------------------------------------------------------------------------------------------------------------
# MH chains: default, per-chain scale, conditional prior
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", GRID, ids=_ids(GRID))
def test_mh_chain_matches_oracle_chain(k, s):
    """bars: tests/test_gpu_causal.py::test_mh_chain_matches_oracle_chain"""
    import torch
    m, (x, y, v) = _chain_case(k, s)
    eng = _eng(m, k)
    out = eng.mh_sample(x, y, v, MH["burn"], MH["keep"], MH["q_sd"], MH["seed"], want_draws=True, chunk=17)
    draws, acc = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy()
    ref, ref_acc, _ = OC.mh_sampler(m, (x, y, v), MH["burn"], MH["keep"], MH["q_sd"], MH["seed"], return_acc=True)
    assert draws.shape == ref.shape == (MH["keep"], s["n"], sum(s["z_dims"]))
    row_ok = np.all(np.abs(draws[-1] - ref[-1]) <= 1e-4, axis=1)
    print("k = %d, %s: rows equal to the oracle chain %.4f" % (k, s["name"], row_ok.mean()))
    assert row_ok.mean() >= 0.99, row_ok.mean()
    assert np.abs(acc.astype(np.int64) - ref_acc).max() <= max(2, s["n"] // 50)
    assert 0.02 < acc.sum() / (acc.size * s["n"]) < 0.98
    lp = eng.logpost(x.ravel(), y.ravel(), v, out["state"]).cpu().numpy()
    assert np.abs(lp - out["logp"].cpu().numpy()).max() <= 1e-3
    assert np.array_equal(out["state"].cpu().numpy(), draws[-1])
    out2 = eng.mh_sample(x, y, v, MH["burn"], MH["keep"], MH["q_sd"], MH["seed"], want_draws=True)
    assert torch.equal(out2["draws"], out["draws"])


@pytest.mark.parametrize("k,s", GRID, ids=_ids(GRID))
def test_row_adaptive_chain_and_scale_match_restatement(k, s):
    """bars: tests/test_gpu_row_adapt.py::test_chain_and_scale_match_restatement"""
    m, (x, y, v) = _chain_case(k, s)
    eng = _eng(m, k)
    out = eng.mh_sample(x, y, v, MH["burn"], MH["keep"], MH["q_sd"], MH["seed"], want_draws=True, chunk=17, row_adapt=0.25)
    draws, acc, scale = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy(), out["row_scale"].cpu().numpy()
    up, dn = _table(MH["burn"], 0.25)
    ref = row_adapt_sampler(m, (x, y, v), MH["burn"], MH["keep"], MH["q_sd"], MH["seed"], up, dn)
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    print("k = %d, %s: rows equal to the restatement %.4f" % (k, s["name"], row_ok.mean()))
    assert row_ok.mean() >= 0.99, row_ok.mean()
    assert scale.dtype == np.float32 and np.array_equal(scale[row_ok], ref["scale"][row_ok])
    assert np.ptp(scale) > 0
    assert np.abs(acc.astype(np.int64) - ref["acc"].sum(axis=1)).max() <= max(2, s["n"] // 50)
    assert np.array_equal(out["state"].cpu().numpy(), draws[-1])


@pytest.mark.parametrize("k,s", GRID, ids=_ids(GRID))
def test_conditional_prior_log_posterior_and_chain(k, s):
    """bars: tests/test_gpu_identifiable.py::test_conditional_prior_log_posterior_and_chains"""
    import torch
    m, (x, y, v), z, seg, tab, mu, s2 = _prior_case(k, s)
    eng = _eng(m, k)
    eng.set_prior(torch.from_numpy(seg.astype(np.int32)).cuda(), torch.from_numpy(tab).cuda())
    lp = eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()
    m64, x64, y64, v64, z64 = _f64(m, x, y, v, z)
    ref = OC.log_posterior(m64, x64, y64, v64, z64, prior=(mu, s2))
    assert np.all(np.abs(lp - ref) <= 2e-6 * np.abs(ref) + 5e-4), np.abs(lp - ref).max()
    assert np.abs(ref - OC.log_posterior(m64, x64, y64, v64, z64)).max() > 0.1
    out = eng.mh_sample(x, y, v, PRIOR["burn"], PRIOR["keep"], PRIOR["q_sd"], PRIOR["seed"], want_draws=True)
    ref_draws = OC.mh_sampler(m, (x, y, v), PRIOR["burn"], PRIOR["keep"], PRIOR["q_sd"], PRIOR["seed"],
                              prior=(mu.astype(np.float32), s2.astype(np.float32)))
    same = np.all(np.abs(out["draws"].cpu().numpy()[-1] - ref_draws[-1]) <= 1e-4, axis=1).mean()
    print("k = %d, %s: rows equal to the oracle chain %.4f" % (k, s["name"], same))
    assert same >= 0.97, same
    eng.set_prior(None, None)


# ---------------------------------------------------------------------------------------------------------------------
# effects, the event form of the retained phase
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", GRID, ids=_ids(GRID))
def test_effects_match_oracle_on_same_draws(k, s):
    """bars: tests/test_gpu_causal.py::test_standalone_effects_from_draws_match_oracle_and_the_fused_pass"""
    from bayesgm_amd import _lib
    burn, keep, seed = 6, 5, 21
    m = _deep(41, k, s)
    x, y, v = _data(s["n"], s["p"], 42, s["binary"])
    doses = None if s["binary"] else np.linspace(0, 3, 7).astype(np.float32)
    eng = _eng(m, k)
    fused = eng.mh_sample(x, y, v, burn, keep, 1.0, seed, want_draws=True, effect=_lib.EFFECT_ITE if s["binary"] else _lib.EFFECT_ADRF,
                          x_values=doses, sample_y=True)
    alone = eng.effects(x, fused["draws"], burn, seed, x_values=doses, sample_y=True).cpu().numpy()
    ref = OC.infer_from_latent_posterior(OC.cast_model(m, np.float64), fused["draws"].cpu().numpy().astype(np.float64), x_values=doses,
                                         sample_y=True, seed=seed, burn_in=burn)
    assert alone.shape == ref.shape and np.abs(alone - ref).max() <= 2e-4, np.abs(alone - ref).max()
    fused_out = fused["ite"].t().cpu().numpy() if s["binary"] else fused["adrf"].cpu().numpy()
    assert np.abs(alone - fused_out).max() <= 1e-5


@pytest.mark.parametrize("k,s", GRID, ids=_ids(GRID))
def test_event_form_of_the_retained_phase_is_bit_identical(k, s):
    """identities: tests/test_gpu_causal.py::test_event_form_of_the_retained_phase_is_bit_identical / ..._for_binary_treatment_..."""
    from bayesgm_amd import _lib
    m = _deep(21, k, s)
    x, y, v = _data(s["n"], s["p"], 22, s["binary"])
    xs = np.linspace(0, 3, 5)
    kw = dict(effect=_lib.EFFECT_ITE, want_draws=True) if s["binary"] else dict(effect=_lib.EFFECT_ADRF, x_values=xs, want_draws=True)
    eng = _eng(m, k)
    eng.set_outcome_cache(False)
    ref = eng.mh_sample(x, y, v, 25, 70, 1.0, 5, **kw)
    eng.set_outcome_cache(True)
    eng.outcome_cache_stats(reset=True)
    got = eng.mh_sample(x, y, v, 25, 70, 1.0, 5, **kw)
    served, total = eng.outcome_cache_stats()
    assert total == s["n"] * 70                                            # chain-iterations: the event form ran
    assert total - served == int(got["acc_count"].cpu().numpy()[26:].sum()) + s["n"]
    # several segments (a budget that holds about 9 retained iterations of this panel), and the retained phase over three calls
    n_slots, tiles, q = eng.mh_slots(s["n"]), (s["n"] + 15) // 16, sum(s["z_dims"])
    per_iter = n_slots * ((tiles + n_slots - 1) // n_slots) * 16 * (4 * q + 4 + 32 * (1 if s["binary"] else (len(xs) + 3) // 4))
    fixed = 2 * tiles * 64 * 2 * 4 + tiles * 8 + n_slots * 4 if s["binary"] else 0
    eng.set_event_budget(fixed + 9 * per_iter + 100)
    seg = eng.mh_sample(x, y, v, 25, 70, 1.0, 5, **kw)
    chunked = eng.mh_sample(x, y, v, 25, 70, 1.0, 5, chunk=30, **kw)
    eng.set_event_budget(0)
    keys = ("ite", "draws", "acc_count", "state", "logp") if s["binary"] else ("adrf_partial", "adrf", "draws", "acc_count", "state", "logp")
    for key in keys:
        assert np.array_equal(got[key].cpu().numpy(), ref[key].cpu().numpy()), key
        if key != "logp":
            assert np.array_equal(seg[key].cpu().numpy(), ref[key].cpu().numpy()), key
            assert np.array_equal(chunked[key].cpu().numpy(), ref[key].cpu().numpy()), key
    oref = OC.infer_from_latent_posterior(OC.cast_model(m, np.float64), got["draws"].cpu().numpy().astype(np.float64),
                                          None if s["binary"] else xs, True, 5, burn_in=25)
    if s["binary"]:
        assert np.abs(got["ite"].cpu().numpy() - np.asarray(oref).T).max() <= 5e-4
    else:
        assert np.abs(got["adrf"].cpu().numpy() - oref).max() <= 2e-4


# ---------------------------------------------------------------------------------------------------------------------
# split precision, fit, HMC, the encoder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("k,s", GRID, ids=_ids(GRID))
def test_split_precision_log_posterior_matches_float64(k, s, mode):
    """bars: tests/test_gpu_bx3.py::test_bx3_log_posterior_matches_oracle.  The log-posterior kernel only: the split-precision MH kernel
    has a depth loop of its own (causal_mh_bx3_kernel), whose only test is statistical at n = 2048 and stays at five layers."""
    m = _deep(3, k, s)
    x, y, v = _data(s["n"], s["p"], 4, s["binary"])
    z = np.random.RandomState(5).randn(s["n"], sum(s["z_dims"])).astype(np.float32)
    eng = _eng(m, k)
    m64, x64, y64, v64, z64 = _f64(m, x, y, v, z)
    ref = OC.log_posterior(m64, x64, y64, v64, z64)
    eng.set_precision(mode)
    lpbx = eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()
    eng.set_precision("fp32")
    rel, ab = (2e-5, 2e-3) if mode == "bf16x3" else (2e-6, 2e-4)
    err = np.abs(lpbx - ref)
    print("k = %d, %s, %s: worst err / bar %.3f" % (k, s["name"], mode, (err / (rel * np.abs(ref) + ab)).max()))
    assert np.all(err <= rel * np.abs(ref) + ab), err.max()


def _flat(grads):
    return np.concatenate([np.concatenate([dW.ravel(), db.ravel()]) for dW, db in grads])


def _check_fit_gradients(k, s, B):
    """the checks of tests/test_gpu_fit.py::test_theta_gradients_and_z_gradient_match_oracle, with its bars"""
    import torch
    n = s["n"]
    m = _deep(7, k, s)
    x, y, v = _data(n, s["p"], 8, s["binary"])
    z = np.random.RandomState(9).randn(n, sum(s["z_dims"])).astype(np.float32)
    eng = _eng(m, k)
    dev = eng.device
    xd, yd, vd, zd = (torch.from_numpy(a).to(dev) for a in (x.ravel(), y.ravel(), v, z))
    idx_np = np.random.RandomState(3).choice(n, B, replace=False).astype(np.int32)
    idx = torch.from_numpy(idx_np).to(dev)
    npar = eng.fit_begin(n, B)
    grad = torch.empty(npar, device=dev)
    loss = torch.zeros(8, device=dev, dtype=torch.float64)
    eng.fit_theta_grad(xd, yd, vd, zd, idx, B, grad, loss)
    m64 = OC.cast_model(m, np.float64)
    bz, bx, by, bv = (a[idx_np].astype(np.float64) for a in (z, x, y, v))
    lv, mse_v, gg, _ = OF.g_loss_and_grads(m64, bz, bv)
    lx, _, gh, _ = OF.h_loss_and_grads(m64, bz, bx)
    ly, mse_y, gf, _ = OF.f_loss_and_grads(m64, bz, bx, by)
    got = grad.cpu().numpy()
    assert got.size == sum(_flat(g_).size for g_ in (gg, gf, gh))
    o = 0
    for part in (_flat(gg), _flat(gf), _flat(gh)):
        g_ = got[o:o + part.size]
        assert np.abs(g_ - part).max() <= 2e-5 * np.abs(part).max() + 1e-7, (np.abs(g_ - part).max(), np.abs(part).max())
        o += part.size
    l_ = loss.cpu().numpy()
    assert np.allclose([l_[0] / B, l_[2] / B, l_[4] / B], [lv, lx, ly], rtol=2e-5)
    assert np.isclose(l_[1] / (B * s["p"]), mse_v, rtol=2e-5) and np.isclose(l_[5] / B, mse_y, rtol=2e-5)
    zm, zv = torch.zeros_like(zd), torch.zeros_like(zd)
    z_before = zd.clone()
    loss.zero_()
    eng.fit_z_step(xd, yd, vd, zd, zm, zv, idx, B, 1e-3, lazy=True, loss=loss)
    lz_ref, dz_ref = OF.z_loss_and_grad(m64, bz, bx, by, bv)
    assert np.isclose(loss.cpu().numpy()[6] / B, lz_ref, rtol=2e-5)
    assert np.abs(zm.cpu().numpy()[idx_np] / 0.1 - dz_ref).max() <= 2e-5 * np.abs(dz_ref).max() + 1e-8
    untouched = np.setdiff1d(np.arange(n), idx_np)
    assert torch.equal(zd[untouched], z_before[untouched])
    eng.fit_end()
    return eng


@pytest.mark.parametrize("B", [16, 33])
@pytest.mark.parametrize("k,s", GRID, ids=_ids(GRID))
def test_fit_gradients_match_oracle(k, s, B):
    """bars: tests/test_gpu_fit.py::test_theta_gradients_and_z_gradient_match_oracle.  B = 16 is a minibatch of the row-tile chains
    (fit_chain.h) where they take the model; B = 33 is beyond them on every model, so the depth loops of fit_kernels.h run."""
    _check_fit_gradients(k, s, B)


P200 = dict(name="p200", z_dims=[1, 1, 1, 7], p=200, binary=False, n=40)


@pytest.mark.parametrize("k,s", [(8, SHAPE_B), (6, P200)], ids=["k8-B", "k6-p200"])
def test_fit_of_a_model_without_a_resident_blob_matches_oracle(k, s):
    """The forward blob of these two does not fit the LDS (the sampling calls refuse them, below); bgm_causal_fit_begin fits them all
    the same: p = 200 at six layers by the row-tile chains, [3,3,6,6] at eight layers (nine dense layers, more than the chains take) by
    the general-width engine.  Same checks and bars as above, B = 16; the sampling calls of the same handle still refuse afterwards."""
    assert not _fits(k, s)
    eng = _check_fit_gradients(k, s, 16)
    x, y, v = _data(s["n"], s["p"], 8, s["binary"])
    with pytest.raises(RuntimeError, match=r"\(-4\).*does not fit the 160 KiB LDS-resident layout"):
        eng.logpost(x.ravel(), y.ravel(), v, np.zeros((s["n"], sum(s["z_dims"])), np.float32))


@pytest.mark.parametrize("k,s", HMC_GRID, ids=_ids(HMC_GRID))
def test_hmc_chain_and_step_match_restatement(k, s):
    """bars: tests/test_gpu_causal_hmc.py::test_chain_and_step_match_restatement"""
    m, (x, y, v) = _chain_case(k, s)
    burn, keep = HMC["burn"], HMC["keep"]
    out = _eng(m, k).hmc_sample(x, y, v, burn, keep, HMC["step0"], HMC["L"], HMC["seed"], want_draws=True, chunk=5, adapt=HMC["target"])
    draws, acc, step = out["draws"].cpu().numpy(), out["acc_count"].cpu().numpy().astype(np.int64), out["row_step"].cpu().numpy()
    up, dn = _table(burn, HMC["target"])
    ref = hmc_sampler(m, (x, y, v), burn, keep, HMC["step0"], HMC["L"], HMC["seed"], up, dn)
    assert draws.shape == ref["draws"].shape == (keep, s["n"], sum(s["z_dims"]))
    row_ok = np.all(np.abs(draws[-1] - ref["draws"][-1]) <= 1e-4, axis=1)
    print("k = %d, %s: rows equal to the restatement %.4f; acceptance %.3f" % (k, s["name"], row_ok.mean(), acc.sum() / float(acc.size * s["n"])))
    assert row_ok.mean() >= 0.97, row_ok.mean()
    assert step.dtype == np.float32 and np.array_equal(step[row_ok], ref["step"][row_ok])
    assert np.ptp(step) > 0
    assert np.abs(acc - ref["acc"].sum(axis=1)).max() <= int((~row_ok).sum())
    assert np.array_equal(out["state"].cpu().numpy(), draws[-1])


@pytest.mark.parametrize("k,s", [(k, s) for s in (SHAPE_A, SHAPE_B) for k in DEPTHS], ids=_ids([(k, s) for s in (SHAPE_A, SHAPE_B) for k in DEPTHS]))
def test_encoder_matches_oracle(k, s):
    """bar: tests/test_gpu_causal.py::test_encoder_matches_oracle.  e is [64] x k; g stays at five layers."""
    m = _model(11, s["z_dims"], s["p"], s["binary"], e_units=(64,) * k)
    _, _, v = _data(s["n"], s["p"], 12)
    got = _engine(m, e_units=[64] * k).encode(v).cpu().numpy()
    ref = mlp_forward(OC.cast_model(m, np.float64)["e"], v.astype(np.float64))
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------------
# what does not fit is refused by name on the host, and the handle stays usable
# ---------------------------------------------------------------------------------------------------------------------
def test_oversized_models_are_refused_by_name():
    """pattern: tests/test_gpu_causal_hmc.py::test_unsupported_paths_refuse.  The sizes come from _blob_bytes / _hmc_bytes, not from a
    probe: every configuration here exceeds 163 840 B by the host's own arithmetic, and the host checks it before any launch."""
    import torch
    from bayesgm_amd import _lib
    big = P200
    assert _blob_bytes(5, big) <= LDS_LIMIT < _blob_bytes(6, big) and LDS_LIMIT < _blob_bytes(8, SHAPE_B)
    assert _blob_bytes(8, SHAPE_A) <= LDS_LIMIT < _hmc_bytes(8, SHAPE_A)
    layout = r"\(-4\).*model does not fit the 160 KiB LDS-resident layout \(%d B\)"
    for k, s in ((6, big), (8, big), (8, SHAPE_B)):
        m = _deep(51, k, s)
        x, y, v = _data(s["n"], s["p"], 52, s["binary"])
        q = sum(s["z_dims"])
        z = np.zeros((s["n"], q), np.float32)
        draws = np.zeros((2, s["n"], q), np.float32)
        xs = np.linspace(0, 1, 3)
        eng = _eng(m, k)
        eff = dict(effect=_lib.EFFECT_ITE) if s["binary"] else dict(effect=_lib.EFFECT_ADRF, x_values=xs)
        calls = [lambda: eng.logpost(x.ravel(), y.ravel(), v, z), lambda: eng.mh_sample(x, y, v, 3, 3, 0.5, 7),
                 lambda: eng.mh_sample(x, y, v, 3, 3, 0.5, 7, **eff), lambda: eng.mh_sample(x, y, v, 3, 3, 0.5, 7, row_adapt=0.25),
                 lambda: eng.effects(x, draws, 0, 7, x_values=None if s["binary"] else xs),
                 lambda: eng.logpost_grad(x.ravel(), y.ravel(), v, z), lambda: eng.hmc_sample(x, y, v, 2, 2, 0.1, 2, 7)]
        for call in calls:
            with pytest.raises(RuntimeError, match=layout % _blob_bytes(k, s)):
                call()
        for mode in ("bf16x3", "f16x3"):
            eng.set_precision(mode)
            with pytest.raises(RuntimeError, match=layout % _blob_bytes(k, s)):
                calls[0]()
        eng.set_precision("fp32")
        rs = np.random.RandomState(33)                                     # a conditional prior does not change the route
        eng.set_prior(torch.from_numpy(rs.randint(0, 5, s["n"]).astype(np.int32)).cuda(),
                      torch.from_numpy(OI.prior_table(OI.init_prior_net(rs, 5, q), q)).cuda())
        for call in calls[:2]:
            with pytest.raises(RuntimeError, match=layout % _blob_bytes(k, s)):
                call()
        eng.set_prior(None, None)
        # the handle is still usable: the same engine, reconfigured by nothing, encodes (the encoder has its own blob)
        assert eng.encode(v).shape == (s["n"], q)
        # and a five-layer model on the same data runs
        assert _eng(_deep(51, 5, s), 5).logpost(x.ravel(), y.ravel(), v, z).shape == (s["n"],)
    # the encoder is [64] x k with a blob of its own: 16 * 13 * 64 + 64 + 7 * 4160 + 1024 + 16 floats at p = 200, k = 8
    s = P200
    assert 4 * (16 * 13 * 64 + 64 + 7 * (4096 + 64) + 64 * 16 + 16) == 174144 > LDS_LIMIT
    m = _model(56, s["z_dims"], s["p"], e_units=(64,) * 8)
    x, y, v = _data(s["n"], s["p"], 57)
    eng = _engine(m, e_units=[64] * 8)
    for _ in range(2):
        with pytest.raises(RuntimeError, match=r"\(-4\).*encoder does not fit the LDS-resident layout"):
            eng.encode(v)
    z = np.random.RandomState(58).randn(s["n"], 10).astype(np.float32)
    got = eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()            # g, f, h of the same engine fit and run
    m64, x64, y64, v64, z64 = _f64(m, x, y, v, z)
    ref = OC.log_posterior(m64, x64, y64, v64, z64)
    assert np.all(np.abs(got - ref) <= 2e-6 * np.abs(ref) + 2e-4)
    # HMC on shape A at k = 8: the forward blob fits, the dual-access copy of the gradient kernels does not
    s = SHAPE_A
    m = _deep(53, 8, s)
    x, y, v = _data(s["n"], s["p"], 54)
    z = np.random.RandomState(55).randn(s["n"], 10).astype(np.float32)
    eng = _eng(m, 8)
    hmc = r"\(-4\).*bgm_causal_hmc: the weights do not fit the 160 KiB LDS \(%d B\)" % _hmc_bytes(8, s)
    for _ in range(2):                                                     # refused again, not cached as valid
        with pytest.raises(RuntimeError, match=hmc):
            eng.logpost_grad(x.ravel(), y.ravel(), v, z)
        with pytest.raises(RuntimeError, match=hmc):
            eng.hmc_sample(x, y, v, 2, 2, 0.1, 2, 7)
    got = eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()            # the refusals left the handle usable
    m64, x64, y64, v64, z64 = _f64(m, x, y, v, z)
    ref = OC.log_posterior(m64, x64, y64, v64, z64)
    assert np.all(np.abs(got - ref) <= 2e-6 * np.abs(ref) + 2e-4)
    assert eng.mh_sample(x, y, v, 3, 3, 0.5, 7)["state"].shape == (s["n"], 10)
    assert bool(torch.isfinite(eng.mh_sample(x, y, v, 3, 3, 0.5, 7, row_adapt=0.25)["row_scale"]).all())


# ---------------------------------------------------------------------------------------------------------------------
# the CPU agreement table of the module docstring
# ---------------------------------------------------------------------------------------------------------------------
def cpu_agreement(k, s):
    """float32 against float64 restatement, rows of the last draw within 1e-4: (MH, row-adaptive MH, conditional prior, HMC or None)"""
    def rows(a, b):
        return float(np.all(np.abs(a[-1] - b[-1]) <= 1e-4, axis=1).mean())
    m, (x, y, v) = _chain_case(k, s)
    m64, x64, y64, v64 = _f64(m, x, y, v)
    args = (MH["burn"], MH["keep"], MH["q_sd"], MH["seed"])
    mh = rows(OC.mh_sampler(m, (x, y, v), *args), OC.mh_sampler(m64, (x64, y64, v64), *args))
    up, dn = _table(MH["burn"], 0.25)
    ra = rows(row_adapt_sampler(m, (x, y, v), *args, up, dn)["draws"], row_adapt_sampler(m64, (x64, y64, v64), *args, up, dn)["draws"])
    hm = None
    if _hmc_fits(k, s):
        up, dn = _table(HMC["burn"], HMC["target"])
        hargs = (HMC["burn"], HMC["keep"], HMC["step0"], HMC["L"], HMC["seed"], up, dn)
        hm = rows(hmc_sampler(m, (x, y, v), *hargs)["draws"], hmc_sampler(m64, (x64, y64, v64), *hargs)["draws"])
    mp, (x, y, v), _, _, _, mu, s2 = _prior_case(k, s)
    mp64, x64, y64, v64 = _f64(mp, x, y, v)
    pargs = (PRIOR["burn"], PRIOR["keep"], PRIOR["q_sd"], PRIOR["seed"])
    pr = rows(OC.mh_sampler(mp, (x, y, v), *pargs, prior=(mu.astype(np.float32), s2.astype(np.float32))),
              OC.mh_sampler(mp64, (x64, y64, v64), *pargs, prior=(mu, s2)))
    return mh, ra, pr, hm


if __name__ == "__main__":
    for k_, s_ in sorted(GRID + [HMC_EDGE], key=lambda c: (c[1]["name"], c[0])):
        print("    %d   %s       " % (k_, s_["name"]) + "   ".join("%-8s" % ("-" if a is None else "%.1f %%" % (100 * a)) for a in cpu_agreement(k_, s_)))
