"""predict_individual on the CPU: the refusals of the class surface, the subgroup formula, the finalisation of the per-row moments,
the row blocks of interval='quantile' and the declaration of the entry point.  No device is touched."""
import os

import numpy as np
import pytest

from bayesgm_amd import causal_hmc as HM

DATA = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))


def _bare(cls, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def _error(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(DATA, *args, **kw)
    return str(e.value)


def test_predict_individual_refusals():
    from bayesgm_amd.models.causalbgm import CausalBGM
    ok = _bare(CausalBGM)
    assert "x_values" in _error(ok.predict_individual, None)
    assert "interval must be 'normal' or 'quantile'" in _error(ok.predict_individual, [0.0], interval="hpd")
    msg = _error(ok.predict_individual, [0.0], draw_budget_bytes=1 << 20)
    assert "interval='normal'" in msg and "draw_budget_bytes" in msg
    assert "draw_budget_bytes must be positive" in _error(ok.predict_individual, [0.0], interval="quantile", draw_budget_bytes=0)
    msg = _error(_binary(CausalBGM).predict_individual, [0.0])
    assert "binary" in msg and "predict's ITE" in msg
    assert "groups must be integer labels" in _error(ok.predict_individual, [0.0], groups=np.zeros(3, np.int64))
    assert "groups must be integer labels" in _error(ok.predict_individual, [0.0], groups=np.zeros(4, np.float32))
    # every refusal of the HMC sampler, through the same calls as predict(sampler='hmc'): word for word, and before the method's own
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(mass="dense"), "mass must be"),
                     (dict(mass="diag", burn_in=10), "burn_in >= 20")):
        msg = _error(ok.predict_individual, [0.0], **kw)
        assert word in msg and msg == _error(ok.predict, x_values=[0.0], sampler="hmc", **kw)
        assert msg == _error(ok.predict_individual, None, interval="hpd", **kw)
    split = _bare(CausalBGM)
    split._p["mh_precision"] = "f16x3"
    msg = _error(split.predict_individual, [0.0])
    assert "mh_precision" in msg and msg == _error(split.predict, x_values=[0.0], sampler="hmc")


def _binary(cls):
    m = _bare(cls)
    m._p["binary_treatment"] = True
    return m


def test_subclasses_refuse_predict_individual_as_they_refuse_hmc():
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    for cls, params, word in ((IdentifiableCausalBGM, dict(n_segments=3), "IdentifiableCausalBGM"),
                              (IdentifiableCausalBGMBayes, dict(n_segments=3), "IdentifiableCausalBGM"),
                              (CausalBGMBayes, dict(), "not available for CausalBGMBayes")):
        m = _bare(cls, **params)
        want = _error(m.predict, x_values=[0.0], sampler="hmc")
        assert word in want
        assert _error(m.predict_individual, [0.0]) == want
        assert _error(m.predict_individual, None, interval="quantile", groups=[1]) == want
        assert _error(m.predict_individual, [0.0], mass="diag") == _error(m.predict, x_values=[0.0], sampler="hmc", mass="diag")
    m = _bare(CausalBGMBayes)
    m._p["use_bnn"] = True
    assert "use_bnn" in _error(m.predict_individual, [0.0]) and _error(m.predict_individual, [0.0]) == _error(m.predict, x_values=[0.0], sampler="hmc")


def test_group_formula():
    """mean_g = mean_i(mean_ik), sd_g = sqrt(sum_i var_ik) / m_g, restated in float64 NumPy row by row"""
    rs = np.random.RandomState(5)
    n, n_doses = 23, 4
    mean, sd = rs.randn(n, n_doses), rs.uniform(0.1, 2.0, (n, n_doses))
    labels = rs.randint(0, 3, n) * 5 - 5          # -5, 0, 5 scattered over the rows: no label is contiguous
    labels[11] = 77                               # a label with one row
    assert len({tuple(np.flatnonzero(labels == g)) for g in (-5, 0, 5)}) == 3 and np.any(np.diff(np.flatnonzero(labels == 0)) > 1)
    got = HM.group_dose_response(mean.astype(np.float32), sd.astype(np.float32), labels)
    assert sorted(got) == [-5, 0, 5, 77]
    m32, s32 = mean.astype(np.float32).astype(np.float64), sd.astype(np.float32).astype(np.float64)
    for g, (mean_g, sd_g) in got.items():
        rows = [i for i in range(n) if labels[i] == g]
        want_mean = np.array([sum(m32[i, k] for i in rows) / len(rows) for k in range(n_doses)])
        want_sd = np.array([np.sqrt(sum(s32[i, k] ** 2 for i in rows)) / len(rows) for k in range(n_doses)])
        assert mean_g.dtype == sd_g.dtype == np.float64 and mean_g.shape == sd_g.shape == (n_doses,)
        assert np.allclose(mean_g, want_mean, rtol=1e-14, atol=0) and np.allclose(sd_g, want_sd, rtol=1e-14, atol=0)
    assert np.array_equal(got[77][0], m32[11]) and np.array_equal(got[77][1], s32[11])
    one = HM.group_dose_response(mean, sd, np.zeros(n, np.int32))
    assert list(one) == [0] and np.allclose(one[0][0], mean.mean(axis=0), rtol=1e-14)
    for bad in (np.zeros(n - 1, np.int64), np.zeros((n, 1), np.int64), np.zeros(n, np.float64)):
        with pytest.raises(ValueError, match="groups must be integer labels"):
            HM.group_dose_response(mean, sd, bad)


def test_moment_finalisation():
    """(ref, s1, s2) as the kernel accumulates them -> np.mean / np.std(ddof=1) of the series"""
    rs = np.random.RandomState(6)
    for m in (2, 20, 400):
        y = (3.0 + rs.randn(7, 5, m) * rs.uniform(0.01, 2.0, (7, 5, 1))).astype(np.float32).astype(np.float64)
        y[3, 2, :] = 1.25                                          # a constant series
        ref = y[..., 0]
        s1, s2 = (y - ref[..., None]).sum(axis=-1), ((y - ref[..., None]) ** 2).sum(axis=-1)
        mean, sd = HM.row_moments_finalize(ref, s1, s2, m)
        assert mean.dtype == sd.dtype == np.float64
        assert np.allclose(mean, y.mean(axis=-1), rtol=1e-13, atol=0)
        assert np.allclose(sd, y.std(axis=-1, ddof=1), rtol=1e-9, atol=1e-13)
        assert mean[3, 2] == 1.25 and sd[3, 2] == 0.0
    # float32 planes (what the device holds): converted before any arithmetic
    mean, sd = HM.row_moments_finalize(ref.astype(np.float32), s1.astype(np.float32), s2.astype(np.float32), m)
    assert mean.dtype == np.float64 and np.allclose(sd, y.std(axis=-1, ddof=1), rtol=1e-5, atol=1e-7)
    # rounding that leaves s2 a hair below s1^2 / m: clamped, sd 0 and not NaN
    mean, sd = HM.row_moments_finalize(np.array([1.0]), np.array([3.0]), np.array([3.0 * (1 - 1e-16)]), 3)
    assert sd[0] == 0.0 and mean[0] == 2.0
    mean, sd = HM.row_moments_finalize(np.array([1.5]), np.array([0.0]), np.array([0.0]), 1)      # one draw: no spread
    assert mean[0] == 1.5 and sd[0] == 0.0
    import torch
    t = [torch.from_numpy(a.astype(np.float32)) for a in (ref, s1, s2)]
    tm, ts = HM.row_moments_finalize(*t, m)
    assert tm.dtype == torch.float64 and np.array_equal(tm.numpy(), mean_of(ref, s1, m)) and np.allclose(ts.numpy(), y.std(axis=-1, ddof=1), rtol=1e-5, atol=1e-7)


def mean_of(ref, s1, m):
    return ref.astype(np.float32).astype(np.float64) + s1.astype(np.float32).astype(np.float64) / m


def test_individual_row_blocks():
    shard = [(100, 1000)]
    assert HM.individual_blocks(shard, 3000, 20, "normal") == shard                         # nothing of size n_keep is stored
    assert HM.individual_blocks(shard, 3000, 20, "quantile") == shard                       # 2 GiB / (4 * 3000 * 20) = 8947 rows: one block
    assert HM.individual_block_rows(3000, 20) == (2 << 30) // (4 * 3000 * 20) // 16 * 16 == 8944
    cut = HM.individual_blocks(shard, 20, 5, "quantile", 4 * 20 * 5 * 32)                    # 32 rows a block
    assert cut == [(s, min(s + 32, 1000)) for s in range(100, 1000, 32)] and len(cut) == 29 and cut[-1] == (996, 1000)
    assert HM.individual_block_rows(20, 5, 4 * 20 * 5 * 47) == 32                            # whole row tiles
    tiny = HM.individual_blocks(shard, 3000, 20, "quantile", 4 * 3000 * 20 * 3)              # fewer than 16 rows fit: one tile a block
    assert HM.individual_block_rows(3000, 20, 4 * 3000 * 20 * 3) == 16 and tiny[0] == (100, 116) and len(tiny) == 57
    assert HM.individual_blocks([], 20, 5, "quantile") == []
    with pytest.raises(ValueError, match="draw_budget_bytes"):
        HM.individual_blocks(shard, 20, 5, "quantile", 0)


def test_abi_declares_the_entry_point():
    from bayesgm_amd import _lib
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    name = "bgm_causal_hmc_run_row_effects"
    assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
    assert _lib.SYMBOLS[name] == _lib.SYMBOLS["bgm_causal_hmc_run_effects"]      # row_moments / row_draws in place of adrf_partial / ite
    src = open(os.path.join(root, "bayesgm_amd", "csrc", "build.py")).read()
    assert '"causal_hmc_rowfx_api.hip"' in src
    from bayesgm_amd.engine import CausalEngine
    assert callable(CausalEngine.hmc_run_rows_effects)
