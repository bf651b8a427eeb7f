"""Keep phase of the fused MH sampler: the 32 -> 8 -> 2 tail of the outcome net f in the dose passes runs on the vector ALU, one pass
behind the layer-2 MFMAs of the next pass (csrc/causal_kernels.h causal_dose_passes_valu).  BGM_MH_MFMA_TAILS=1 at handle creation
selects the instances that keep the tail on the matrix pipe, as before.

The dose passes do not feed back into the chains, so state, cached log posterior, acceptance counts and draws are expected bit for
bit (np.array_equal) between the two engines; only the ADRF moves, by the fp32 rounding of a 32-term and an 8-term dot product summed
in another order.  Checked per case:
  * the chains of the two engines are equal to the last bit;
  * on the new engine the ADRF with the per-wave outcome cache equals the ADRF without it to the last bit (the cached replay,
    causal_effects_cached, repeats the uncached finish);
  * the ADRF of both engines against the float64 oracle on the retained draws (same weights, same Philox words) within 2e-4 abs, the
    tolerance of tests/test_gpu_causal.py::test_adrf_effects_match_oracle_on_same_draws.  The worst error of each engine is printed
    (MI355X, over all cases: 1.38e-7 with the vector-ALU tails, 1.38e-7 with the matrix-pipe tails, 1.2e-7 between the two).

Dose counts cover the pass plan: 1 and 3 (one partial shared-call pass: the new path's prologue and drain only), 4, 16 (four owned
calls, no remainder), 17 and 20 (owned calls plus a remainder pass).  p = 20 runs the direct form of g's likelihood, p = 50 the Gram
form; n = 40 has a ragged last tile, n = 16 is exactly one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import causal as OC            # noqa: E402
from oracle import identifiable as OI      # noqa: E402
from tests.test_gpu_causal import _model, _data, _engine  # noqa: E402

MFMA = "BGM_MH_MFMA_TAILS"
Z_DIMS = [1, 1, 1, 7]
BURN, KEEP, CHUNK, SEED, Q_SD = 10, 7, 6, 20260131, 0.5      # chunks of 6: the retained phase is split at iterations 12 and 16
TOL = 2e-4
_cache = {}


def _pair(p):
    """(model, new engine, matrix-pipe-tails engine) for v_dim = p, built once"""
    if p not in _cache:
        assert MFMA not in os.environ
        m = _model(81 + p, Z_DIMS, p)
        new = _engine(m)
        os.environ[MFMA] = "1"
        try:
            old = _engine(m)
        finally:
            del os.environ[MFMA]
        _cache[p] = (m, new, old)
    return _cache[p]


def _sample(eng, x, y, v, xs, sample_y, cache, **kw):
    from bayesgm_amd import _lib
    eng.set_outcome_cache("wave" if cache else False)
    try:
        return eng.mh_sample(x, y, v, BURN, KEEP, Q_SD, SEED, want_draws=True, chunk=CHUNK, effect=_lib.EFFECT_ADRF, x_values=xs,
                             sample_y=sample_y, **kw)
    finally:
        eng.set_outcome_cache(True)


def _check(m, new, old, x, y, v, n_doses, keys=("state", "logp", "acc_count", "draws"), xs=None, expect=None, **kw):
    """The checks of the module docstring on one panel.  xs: the doses (default: linspace(0, 3, n_doses)).  expect: what the instance
    table says about this engine pair (tests/test_gpu_valu_tails_instances.py): 'mfma' = both ran the same matrix-pipe instance, so the
    ADRFs are equal to the last bit; 'valu' = the new engine ran the vector-ALU instance, so they are not.  Returns the worst
    |ADRF - oracle64| of the new engine, of the old engine, and the worst difference between the two."""
    xs = np.linspace(0.0, 3.0, n_doses) if xs is None else xs
    assert len(xs) == n_doses
    m64 = OC.cast_model(m, np.float64)
    worst = np.zeros(3)
    for sample_y in (True, False):
        out_n = _sample(new, x, y, v, xs, sample_y, False, **kw)
        out_o = _sample(old, x, y, v, xs, sample_y, False, **kw)
        for k in keys:
            a, b = out_n[k].cpu().numpy(), out_o[k].cpu().numpy()
            assert np.isfinite(a).all(), k
            assert np.array_equal(a, b), (k, sample_y)
        assert out_n["acc_count"].sum().item() > 0          # chains moved
        cached = _sample(new, x, y, v, xs, sample_y, True, **kw)["adrf"].cpu().numpy()
        a_n, a_o = out_n["adrf"].cpu().numpy(), out_o["adrf"].cpu().numpy()
        assert a_n.shape == (n_doses, KEEP)
        assert np.array_equal(cached, a_n), (sample_y, np.abs(cached - a_n).max())
        ref = OC.infer_from_latent_posterior(m64, out_n["draws"].cpu().numpy().astype(np.float64), xs, sample_y, SEED, burn_in=BURN)
        e_n, e_o = np.abs(a_n - ref).max(), np.abs(a_o - ref).max()
        print("sample_y=%d: worst |adrf - oracle64| vector-ALU tails %.3e, matrix-pipe tails %.3e, between the two %.3e"
              % (sample_y, e_n, e_o, np.abs(a_n - a_o).max()))
        assert e_n <= TOL and e_o <= TOL, (sample_y, e_n, e_o)
        if expect is not None:
            assert np.array_equal(a_n, a_o) == (expect == "mfma"), (expect, sample_y)
        worst = np.maximum(worst, [e_n, e_o, np.abs(a_n - a_o).max()])
    return tuple(worst)


@pytest.mark.parametrize("n_doses", [1, 3, 4, 16, 17, 20])
@pytest.mark.parametrize("n", [40, 16])
@pytest.mark.parametrize("p", [20, 50], ids=["direct", "gram"])
def test_valu_tails_keep_the_chains_and_match_the_oracle(p, n, n_doses):
    m, new, old = _pair(p)
    x, y, v = _data(n, p, 82)
    _check(m, new, old, x, y, v, n_doses)


def test_valu_tails_with_the_conditional_prior():
    import torch
    p, n = 50, 40
    m = _model(91, Z_DIMS, p)
    x, y, v = _data(n, p, 92)
    rs = np.random.RandomState(93)
    pn = OI.init_prior_net(rs, 5, sum(Z_DIMS))
    pn = [(W, (0.3 * rs.randn(*b.shape)).astype(np.float32)) for W, b in pn]
    seg, tab = rs.randint(0, 5, n).astype(np.int32), OI.prior_table(pn, sum(Z_DIMS))
    new = _engine(m)
    os.environ[MFMA] = "1"
    try:
        old = _engine(m)
    finally:
        del os.environ[MFMA]
    for eng in (new, old):
        eng.set_prior(torch.from_numpy(seg).cuda(), torch.from_numpy(tab).cuda())
    _check(m, new, old, x, y, v, 20)


def test_valu_tails_with_a_proposal_scale_per_chain():
    p, n = 50, 40
    m, new, old = _pair(p)
    x, y, v = _data(n, p, 94)
    _check(m, new, old, x, y, v, 20, keys=("state", "logp", "acc_count", "draws", "row_scale"), row_adapt=0.25)
