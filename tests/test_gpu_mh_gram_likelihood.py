"""Gram form of g's Gaussian likelihood in the fp32 MH kernels (csrc/causal_kernels.h, g_last_gram) against the direct form
(BGM_MH_DIRECT_LIKELIHOOD=1 at handle creation) and the float64 oracle.

The two forms differ by fp32 rounding in the log posterior only: final chain states agree on >= 99 % of the rows, acceptance counts
within the bound of test_gpu_causal, and the log posterior the sampler caches for its final state is within 2e-6 |ref| + 2e-4 of
the float64 oracle (5e-4 with the conditional prior, as in test_gpu_identifiable)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import causal as OC            # noqa: E402
from oracle import identifiable as OI      # noqa: E402
from tests.test_gpu_causal import _model, _data, _engine  # noqa: E402

DIRECT = "BGM_MH_DIRECT_LIKELIHOOD"


def _pair(m):
    """(Gram-form engine, direct-form engine) on the same model"""
    assert DIRECT not in os.environ
    gram = _engine(m)
    os.environ[DIRECT] = "1"
    try:
        direct = _engine(m)
    finally:
        del os.environ[DIRECT]
    return gram, direct


def _run(eng, x, y, v, binary, prior):
    import torch
    from bayesgm_amd import _lib
    if prior is not None:
        eng.set_prior(torch.from_numpy(prior[0].astype(np.int32)).cuda(), torch.from_numpy(prior[1]).cuda())
    kw = dict(effect=_lib.EFFECT_ITE) if binary else dict(effect=_lib.EFFECT_ADRF, x_values=np.linspace(0.0, 2.0, 6))
    return eng.mh_sample(x, y, v, 30, 30, 0.3, 987654321, want_draws=True, chunk=23, **kw)


def _ref_logp(m, x, y, v, z, prior=None):
    return OC.log_posterior(OC.cast_model(m, np.float64), x.astype(np.float64), y.astype(np.float64), v.astype(np.float64),
                            z.astype(np.float64), prior=prior)


CASES = [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=300, ntl=13),     # 13 output tiles
         dict(z_dims=[1, 1, 1, 7], p=200, binary=True, n=200, ntl=13),
         dict(z_dims=[2, 2, 2, 6], p=150, binary=True, n=130, ntl=10),      # 10 output tiles, two-K-tile first layer
         dict(z_dims=[2, 2, 2, 6], p=120, binary=False, n=90, ntl=10),      # 8 tiles -> the 10-tile shape
         dict(z_dims=[1, 1, 1, 7], p=50, binary=False, n=100, ntl=7),      # 4 tiles -> the 7-tile shape
         dict(z_dims=[1, 1, 1, 7], p=207, binary=False, n=70, ntl=13)]      # the largest v_dim


@pytest.mark.parametrize("cond_prior", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_gram_and_direct_forms_agree(case, cond_prior):
    m = _model(31, case["z_dims"], case["p"], case["binary"])
    x, y, v = _data(case["n"], case["p"], 32, case["binary"])
    q, n = sum(case["z_dims"]), case["n"]
    prior = prior64 = None
    if cond_prior:
        rs = np.random.RandomState(33)
        pn = OI.init_prior_net(rs, 5, q)
        pn = [(W, (0.3 * rs.randn(*b.shape)).astype(np.float32)) for W, b in pn]
        seg = rs.randint(0, 5, n)
        prior = (seg, OI.prior_table(pn, q))
        mu, s2, _ = OI.prior_params([(W.astype(np.float64), b.astype(np.float64)) for W, b in pn], seg)
        prior64 = (mu, s2)
    gram, direct = _pair(m)
    info_g, info_d = gram.mh_info(n), direct.mh_info(n)
    assert info_d.mfma_per_transition_per_wave - info_g.mfma_per_transition_per_wave == 16 * case["ntl"] - 64
    out_g = _run(gram, x, y, v, case["binary"], prior)
    out_d = _run(direct, x, y, v, case["binary"], prior)
    sg, sd = out_g["state"].cpu().numpy(), out_d["state"].cpu().numpy()
    same = np.all(np.abs(sg - sd) <= 1e-4, axis=1).mean()
    assert same >= 0.99, same
    acc_g, acc_d = out_g["acc_count"].cpu().numpy().astype(np.int64), out_d["acc_count"].cpu().numpy().astype(np.int64)
    assert np.abs(acc_g - acc_d).max() <= max(2, n // 50)
    tol = 5e-4 if cond_prior else 2e-4
    for out, s in ((out_g, sg), (out_d, sd)):
        ref = _ref_logp(m, x, y, v, s, prior64)
        err = np.abs(out["logp"].cpu().numpy() - ref)
        assert np.all(err <= 2e-6 * np.abs(ref) + tol), (err.max(), np.abs(ref).max())


def test_gram_form_when_v_is_far_from_the_origin_of_the_output_layer():
    """|v| >> |residual|: g's output bias offset by 5, v = g(z*) + N(0, 0.05^2) at known z*, sigma_v = 0.05.  The Gram form's error
    scales with eps |m0 - v|^2 / (2 sigma_v^2); the anchor m0 = g(0) keeps it within the log-posterior tolerance."""
    from oracle.nets import mlp_forward
    z_dims, p, n = [1, 1, 1, 7], 200, 512
    m = _model(41, z_dims, p, False, sigma_v=0.05)
    W, b = m["g"][-1]
    m["g"][-1] = (W, (b + 5.0).astype(np.float32))
    rs = np.random.RandomState(42)
    zs = rs.randn(n, sum(z_dims))
    mean = mlp_forward(OC.cast_model(m, np.float64)["g"], zs)[:, :p]
    v = (mean + 0.05 * rs.randn(n, p)).astype(np.float32)
    x, y, _ = _data(n, p, 43)
    gram, direct = _pair(m)
    errs = {}
    for name, eng in (("gram", gram), ("direct", direct)):
        out = eng.mh_sample(x, y, v, 40, 20, 0.1, 4242, want_draws=False)
        s = out["state"].cpu().numpy()
        ref = _ref_logp(m, x, y, v, s)
        err = np.abs(out["logp"].cpu().numpy() - ref)
        errs[name] = (err.max(), (err / (2e-6 * np.abs(ref) + 2e-4)).max(), np.median(np.abs(ref)))
    print("worst |logp - float64| (abs, fraction of the tolerance, median |ref|): gram %.3g %.3f %.3g, direct %.3g %.3f %.3g"
          % (errs["gram"] + errs["direct"]))
    assert errs["gram"][1] <= 1.0, errs
