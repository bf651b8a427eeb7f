"""predict_average on the CPU: the combiner of the per-draw label sums into ATE / ATT / ATC against NumPy float64, the refusals of the
class surface, the subclasses' refusals and the declaration of the two entry points.  No device is touched."""
import os

import numpy as np
import pytest

from bayesgm_amd import causal_hmc as HM

N = 6
DATA = (np.array([[0], [1], [1], [0], [1], [0]], np.float32), np.zeros((N, 1), np.float32), np.zeros((N, 5), np.float32))


def _bare(cls, binary=True, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=binary, **params)
    obj.params = obj._p
    return obj


def _error(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(DATA, *args, **kw)
    return str(e.value)


def _panel(rs, n, n_groups, n_draws):
    """a panel with unequal groups: per-row ITE draws (float32 values held in float64), group index, arm"""
    ite = rs.randn(n, n_draws).astype(np.float32).astype(np.float64) * 3.0 + 1.0
    group = np.minimum((rs.uniform(size=n) ** 2 * n_groups).astype(np.int64), n_groups - 1)      # group 0 is the largest
    arm = (rs.uniform(size=n) < 0.3).astype(np.int64)
    return ite, group, arm


def _sums(ite, labels, n_groups):
    return np.stack([ite[labels == c].sum(axis=0) for c in range(2 * n_groups)]).reshape(n_groups, 2, -1)


def test_combiner_against_numpy():
    rs = np.random.RandomState(3)
    n, n_groups, n_draws = 301, 4, 7
    ite, group, arm = _panel(rs, n, n_groups, n_draws)
    assert len(set(np.bincount(group, minlength=n_groups))) == n_groups and np.bincount(group).min() > 0      # unequal sizes
    labels = HM.average_labels(group, arm.astype(np.float32).reshape(-1, 1))
    assert labels.dtype == np.int32 and np.array_equal(labels, 2 * group + arm)
    counts = HM.average_counts(labels, n_groups)
    assert counts.shape == (n_groups, 2) and counts.sum() == n
    got = HM.combine_average_effects(_sums(ite, labels, n_groups), counts)
    for g in range(n_groups):
        rows = group == g
        assert counts[g, 1] == (rows & (arm == 1)).sum() and counts[g, 0] == (rows & (arm == 0)).sum()
        for name, sel in (("ate", rows), ("att", rows & (arm == 1)), ("atc", rows & (arm == 0))):
            want = ite[sel].mean(axis=0)
            assert got[name].dtype == np.float64 and got[name].shape == (n_groups, n_draws)
            assert np.allclose(got[name][g], want, rtol=1e-13, atol=1e-13), (name, g)
        # n ATE = n1 ATT + n0 ATC
        assert np.allclose(counts[g].sum() * got["ate"][g], counts[g, 1] * got["att"][g] + counts[g, 0] * got["atc"][g], rtol=1e-13, atol=1e-12)
    effect, bounds = HM.average_summary(got["ate"], 0.1)
    assert np.allclose(effect, got["ate"].mean(axis=1), rtol=1e-15) and bounds.shape == (n_groups, 2)
    assert np.allclose(bounds, np.quantile(got["ate"], [0.05, 0.95], axis=1).T, rtol=1e-15) and np.all(bounds[:, 0] <= bounds[:, 1])
    with pytest.raises(ValueError, match="combine_average_effects"):
        HM.combine_average_effects(np.zeros((2, 3, 4)), np.zeros((2, 2)))


def test_a_group_without_treated_rows():
    rs = np.random.RandomState(4)
    n, n_groups, n_draws = 90, 3, 5
    ite, group, arm = _panel(rs, n, n_groups, n_draws)
    arm[group == 1] = 0                                   # group 1 has control rows only
    labels = HM.average_labels(group, arm)
    counts = HM.average_counts(labels, n_groups)
    assert counts[1, 1] == 0 and counts[1, 0] > 0
    got = HM.combine_average_effects(_sums(ite, labels, n_groups), counts)
    assert np.all(np.isnan(got["att"][1])) and not np.isnan(got["att"][[0, 2]]).any()
    assert not np.isnan(got["ate"]).any() and not np.isnan(got["atc"]).any()
    assert np.allclose(got["ate"][1], got["atc"][1], rtol=1e-15)
    effect, bounds = HM.average_summary(got["att"], 0.05)
    assert np.isnan(effect[1]) and np.all(np.isnan(bounds[1])) and np.all(np.isfinite(effect[[0, 2]])) and np.all(np.isfinite(bounds[[0, 2]]))
    group_labels = np.array([-3, 10, 42])
    with pytest.raises(ValueError, match=r"estimand='att' is undefined for groups \[10\].*treated"):
        HM.check_average_estimand("att", effect, group_labels)
    HM.check_average_estimand("ate", HM.average_summary(got["ate"], 0.05)[0], group_labels)
    with pytest.raises(ValueError, match=r"estimand='atc' is undefined for the panel.*control"):
        HM.check_average_estimand("atc", np.array([np.nan]), None)


def test_two_shards_add_up_to_the_single_process_result():
    rs = np.random.RandomState(5)
    n, n_groups, n_draws = 200, 3, 6
    ite, group, arm = _panel(rs, n, n_groups, n_draws)
    labels = HM.average_labels(group, arm)
    whole = HM.combine_average_effects(_sums(ite, labels, n_groups), HM.average_counts(labels, n_groups))
    cut = 77
    s = _sums(ite[:cut], labels[:cut], n_groups) + _sums(ite[cut:], labels[cut:], n_groups)
    c = HM.average_counts(labels[:cut], n_groups) + HM.average_counts(labels[cut:], n_groups)
    assert np.array_equal(c, HM.average_counts(labels, n_groups))
    both = HM.combine_average_effects(s, c)
    for name in HM.ESTIMANDS:
        assert np.allclose(both[name], whole[name], rtol=1e-13, atol=1e-13)


def test_check_average_and_labels():
    distinct, index = HM.check_average(True, "ate", np.array([7, -2, 7, 100, -2, 7]), N)
    assert list(distinct) == [-2, 7, 100] and list(index) == [1, 0, 1, 2, 0, 1] and index.dtype == np.int64
    none, index = HM.check_average(True, "att", None, N)
    assert none is None and list(index) == [0] * N
    assert HM.check_average(True, "atc", np.arange(32).repeat(2), 64)[0].shape == (32,)
    with pytest.raises(ValueError, match="groups: at most 32 distinct labels; got 33"):
        HM.check_average(True, "ate", np.arange(33), 33)
    assert 2 * HM.MAX_GROUPS == 64


def test_predict_average_refusals():
    from bayesgm_amd.models.causalbgm import CausalBGM
    assert CausalBGM.average_effects_ is None
    ok = _bare(CausalBGM)
    assert ok.average_effects_ is None
    msg = _error(_bare(CausalBGM, binary=False).predict_average)
    assert "continuous" in msg and "ADRF" in msg
    assert "estimand must be 'ate', 'att' or 'atc'" in _error(ok.predict_average, estimand="cate")
    assert "groups must be integer labels" in _error(ok.predict_average, groups=np.zeros(N - 1, np.int64))
    assert "groups must be integer labels" in _error(ok.predict_average, groups=np.zeros((N, 1), np.int64))
    assert "groups must be integer labels" in _error(ok.predict_average, groups=np.zeros(N, np.float32))
    big = (np.zeros((40, 1), np.float32), np.zeros((40, 1), np.float32), np.zeros((40, 5), np.float32))
    with pytest.raises(ValueError, match="groups: at most 32"):
        ok.predict_average(big, groups=np.arange(40))
    assert "sampler must be 'mh' or 'hmc'" in _error(ok.predict_average, sampler="nuts")
    assert "q_sd" in _error(ok.predict_average, sampler="mh", q_sd=0.0)
    # every refusal of the HMC sampler, through the same calls as predict(sampler='hmc'): word for word, and before the method's own
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(mass="dense"), "mass must be"),
                     (dict(mass="diag", burn_in=10), "burn_in >= 20"), (dict(q_sd=0.0), "q_sd")):
        msg = _error(ok.predict_average, **kw)
        assert word in msg and msg == _error(ok.predict, sampler="hmc", **kw)
        assert msg == _error(ok.predict_average, estimand="cate", **kw)
    assert "mass='diag' belongs to sampler='hmc'" in _error(ok.predict_average, sampler="mh", mass="diag")
    split = _bare(CausalBGM)
    split._p["mh_precision"] = "f16x3"
    msg = _error(split.predict_average)
    assert "mh_precision" in msg and msg == _error(split.predict, sampler="hmc")
    assert ok.average_effects_ is None and CausalBGM.average_effects_ is None


def test_subclasses_refuse_predict_average():
    from bayesgm_amd.models.causalbgm import CausalBGM
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    for cls, params in ((IdentifiableCausalBGM, dict(n_segments=3)), (IdentifiableCausalBGMBayes, dict(n_segments=3)), (CausalBGMBayes, dict())):
        assert cls.predict_average is not CausalBGM.predict_average
        m = _bare(cls, **params)
        for kw in (dict(), dict(sampler="mh"), dict(estimand="att", groups=np.zeros(N, np.int64))):
            msg = _error(m.predict_average, **kw)
            assert "predict_average is not available for %s:" % cls.__name__ in msg


def test_abi_declares_the_entry_points():
    from bayesgm_amd import _lib
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    for name in ("bgm_causal_hmc_run_group_effects", "bgm_ite_group_sums"):
        assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
    fx, gfx = _lib.SYMBOLS["bgm_causal_hmc_run_effects"][1], _lib.SYMBOLS["bgm_causal_hmc_run_group_effects"][1]
    assert len(gfx) == len(fx) - 1 and gfx[:25] == fx[:25]      # labels, n_labels, group_partial in place of x_values, n_doses, adrf_partial, ite
    assert _lib.EFFECT_GROUP_ITE not in (_lib.EFFECT_NONE, _lib.EFFECT_ADRF, _lib.EFFECT_ITE) and _lib.MAX_GROUP_LABELS == 64
    src = open(os.path.join(root, "bayesgm_amd", "csrc", "build.py")).read()
    assert '"causal_hmc_gfx_api.hip"' in src
    from bayesgm_amd.engine import CausalEngine
    assert callable(CausalEngine.hmc_run_group_effects) and callable(CausalEngine.ite_group_sums)
