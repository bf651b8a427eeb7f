"""First layers of f and h in the LDS-resident CausalBGM kernels: the K-steps whose packed weights are zero by construction (the
latents a net does not take) are not issued (csrc/bgm_device.h dense_masked / dense_pair_masked, masks from z_dims in
causal_pack_forward).  BGM_MH_ALL_KSTEPS=1 at handle creation issues every K-step, as before.

A skipped step adds 0 * b to its accumulators and the remaining steps keep their order, so every output is expected bit for bit:
the masked engine against the all-K-steps engine on the same model, data and seed, with np.array_equal."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import identifiable as OI      # noqa: E402
from tests.test_gpu_causal import _model, _data, _engine  # noqa: E402

ALL = "BGM_MH_ALL_KSTEPS"


def _pair(m):
    """(masked engine, all-K-steps engine) on the same model"""
    assert ALL not in os.environ
    masked = _engine(m)
    os.environ[ALL] = "1"
    try:
        every = _engine(m)
    finally:
        del os.environ[ALL]
    return masked, every


def _skipped_steps(z_dims):
    """(f, h): first-layer K-steps that hold none of the net's input features; feature f of (z, x) sits in K-step f // 4, and the
    compiled first layers have 3 K-steps for q + 1 <= 12 features and 5 for q + 1 <= 20 (csrc/bgm_host.h, bgm_causal_shape)"""
    z0, z1, z2, _ = z_dims
    q = sum(z_dims)
    ks1 = 3 if q + 1 <= 12 else 5
    f_feat = list(range(z0 + z1)) + [q]                                    # (z0, z1, x)
    h_feat = list(range(z0)) + list(range(z0 + z1, z0 + z1 + z2))          # (z0, z2)
    return tuple(ks1 - len({f // 4 for f in feat}) for feat in (f_feat, h_feat))


CASES = [dict(z_dims=[1, 1, 1, 7], p=50, n=100, binary=False, skipped=(1, 2)),                 # f {0, 2}, h {0}
         dict(z_dims=[2, 2, 2, 6], p=120, n=90, binary=False, skipped=(3, 3)),                 # x opens K-step 3
         dict(z_dims=[3, 3, 6, 6], p=100, n=130, binary=True, skipped=(2, 2)),                 # KT1 = 2, ragged last tile
         dict(z_dims=[3, 5, 1, 1], p=50, n=70, binary=False, skipped=(0, 1)),                  # f skips nothing, h the middle step
         dict(z_dims=[1, 1, 1, 7], p=50, n=100, binary=False, skipped=(1, 2), prior=True),     # conditional prior
         dict(z_dims=[1, 1, 1, 7], p=50, n=100, binary=False, skipped=(1, 2), row_adapt=0.25),  # adaptive_sd='row'
         dict(z_dims=[1, 1, 1, 7], p=50, n=100, binary=False, skipped=(1, 2), cache=True),     # event form of the retained phase
         dict(z_dims=[1, 1, 1, 7], p=20, n=40, binary=False, skipped=(1, 2)),                  # 2 output tiles: the direct form of g's term
         dict(z_dims=[1, 1, 1, 7], p=200, n=40, binary=False, skipped=(1, 2))]                 # 13 output tiles: the bench's kernels


def _run(eng, case, x, y, v, prior):
    import torch
    from bayesgm_amd import _lib
    if prior is not None:
        eng.set_prior(torch.from_numpy(prior[0].astype(np.int32)).cuda(), torch.from_numpy(prior[1]).cuda())
    eng.set_outcome_cache(case.get("cache", False))
    kw = dict(effect=_lib.EFFECT_ITE) if case["binary"] else dict(effect=_lib.EFFECT_ADRF, x_values=np.linspace(0.0, 2.0, 6))
    if "row_adapt" in case:
        kw["row_adapt"] = case["row_adapt"]
    eng.outcome_cache_stats(reset=True)
    out = eng.mh_sample(x, y, v, 30, 30, 0.3, 987654321, want_draws=True, chunk=23, **kw)
    if case.get("cache"):
        assert eng.outcome_cache_stats()[1] == v.shape[0] * 30        # retained chain-iterations: the event form ran
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c["z_dims"])) + "-p%d" % c["p"] + "".join("+" + k for k in ("prior", "row_adapt", "cache") if k in c))
def test_masked_and_all_ksteps_engines_are_bit_identical(case):
    z_dims, p, n = case["z_dims"], case["p"], case["n"]
    assert _skipped_steps(z_dims) == case["skipped"]
    m = _model(51, z_dims, p, case["binary"])
    x, y, v = _data(n, p, 52, case["binary"])
    prior = None
    if case.get("prior"):
        rs = np.random.RandomState(53)
        pn = OI.init_prior_net(rs, 5, sum(z_dims))
        pn = [(W, (0.3 * rs.randn(*b.shape)).astype(np.float32)) for W, b in pn]
        prior = (rs.randint(0, 5, n), OI.prior_table(pn, sum(z_dims)))
    masked, every = _pair(m)
    diff = every.mh_info(n).mfma_per_transition_per_wave - masked.mh_info(n).mfma_per_transition_per_wave
    assert diff == 4 * sum(_skipped_steps(z_dims)), diff
    out_m = _run(masked, case, x, y, v, prior)
    out_e = _run(every, case, x, y, v, prior)
    keys = ["state", "logp", "acc_count", "draws", "ite" if case["binary"] else "adrf"] + (["row_scale"] if "row_adapt" in case else [])
    for k in keys:
        a, b = out_m[k].cpu().numpy(), out_e[k].cpu().numpy()
        assert np.isfinite(a).all(), k
        assert np.array_equal(a, b), (k, np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    assert out_m["acc_count"].sum().item() > 0          # chains moved: the comparison is not one of two frozen samplers


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=["1-1-1-7", "3-3-6-6"])
def test_log_posterior_and_effects_calls_are_bit_identical(case):
    z_dims, p, n = case["z_dims"], case["p"], case["n"]
    m = _model(61, z_dims, p, case["binary"])
    x, y, v = _data(n, p, 62, case["binary"])
    rs = np.random.RandomState(63)
    z = rs.randn(n, sum(z_dims)).astype(np.float32)
    draws = rs.randn(5, n, sum(z_dims)).astype(np.float32)
    xs = None if case["binary"] else np.linspace(0.0, 2.0, 6)
    outs = []
    for eng in _pair(m):
        lp = eng.logpost(x.ravel(), y.ravel(), v, z).cpu().numpy()
        eff = eng.effects(x, draws, 30, 7, x_values=xs).cpu().numpy()
        outs.append((lp, eff))
    for a, b in zip(*outs):
        assert np.isfinite(a).all()
        assert np.array_equal(a, b), np.abs(a.astype(np.float64) - b.astype(np.float64)).max()


def test_conditional_prior_with_two_tile_first_layer_keeps_every_kstep():
    """PRIOR = 1 with KT1 = 2: these MH kernels keep the unmasked first layers (csrc/causal_kernels.h causal_l1_masked: the masked ones
    made them spill), so with the prior set mh_info counts every K-step in both engines, and the results are still bit for bit equal."""
    import torch
    from bayesgm_amd import _lib
    z_dims, p, n = [3, 3, 6, 6], 100, 50
    m = _model(71, z_dims, p, False)
    x, y, v = _data(n, p, 72)
    rs = np.random.RandomState(73)
    pn = OI.init_prior_net(rs, 5, sum(z_dims))
    seg, tab = rs.randint(0, 5, n).astype(np.int32), OI.prior_table(pn, sum(z_dims))
    outs, infos = [], []
    for eng in _pair(m):
        free = eng.mh_info(n).mfma_per_transition_per_wave
        eng.set_prior(torch.from_numpy(seg).cuda(), torch.from_numpy(tab).cuda())
        infos.append((free, eng.mh_info(n).mfma_per_transition_per_wave))
        eng.set_outcome_cache(False)
        outs.append(eng.mh_sample(x, y, v, 30, 30, 0.3, 987654321, want_draws=True, chunk=23, effect=_lib.EFFECT_ADRF,
                                  x_values=np.linspace(0.0, 2.0, 6)))
    (m_free, m_prior), (e_free, e_prior) = infos
    assert e_free - m_free == 4 * sum(_skipped_steps(z_dims)) and m_prior == e_prior == e_free, infos
    for k in ("state", "logp", "acc_count", "draws", "adrf"):
        assert np.array_equal(outs[0][k].cpu().numpy(), outs[1][k].cpu().numpy()), k
