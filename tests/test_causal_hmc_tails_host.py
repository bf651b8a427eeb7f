"""interval='tails' on the CPU: the size of a tail buffer (causal_hmc.tail_size), the set update and the finisher restated in NumPy
(tests/_causal_hmc_tails_ref.py) against the quantile formula on the fully sorted series, the row blocks, the declaration of the two
entry points and the refusals of the class surface.  No device is touched.  Every comparison of values is exact (==)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _causal_hmc_tails_ref as TR  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402

ALPHAS = (0.01, 0.05, 0.1, 0.5, 0.9)
MS = (1, 2, 3, 5, 20, 21, 101, 400, 3000)      # 101: 0.55 * 100 is 55.00000000000001 in double
DATA = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))


def _series(rs, m, kind):
    if kind == "random":
        return (2.0 + rs.randn(m)).astype(np.float32)
    if kind == "ties":                     # a chain that rejects most proposals: about m / 7 distinct values, each held for a run
        return np.repeat(rs.randn(m // 7 + 1), 7)[:m].astype(np.float32)
    return np.full(m, 1.25, np.float32)    # constant


def _integral_only_in_exact_arithmetic(alpha, m):
    """q (m - 1) is an integer in exact arithmetic for one of the two levels, and its double product is not that integer"""
    a = Fraction(str(alpha))
    for q_exact, q in ((a / 2, alpha / 2), (1 - a / 2, 1 - alpha / 2)):
        vi = q_exact * (m - 1)
        if vi.denominator == 1 and q * float(m - 1) != float(vi):
            return True
    return False


def test_the_grid_holds_products_that_are_integral_only_in_exact_arithmetic():
    hits = [(a, m) for a in ALPHAS for m in MS if _integral_only_in_exact_arithmetic(a, m)]
    assert hits == [(0.9, 101)]                                # the one pair of this grid; every other integral product is exact in double
    i0, i1, t = TR.quantile_idx(1 - 0.9 / 2, 101)
    assert (i0, i1) == (55, 56) and 0.0 < t < 1e-13            # the upper bound leans on the order statistic 56 by that hair
    assert TR.needed(0.45, 0.55, 101) == (47, 46) and HM.tail_size(0.9, 101) == 47
    # an integral product that IS exact still reads the order statistic above it (with weight zero): (0.1, 21) keeps 3 a side
    assert 0.95 * 20.0 == 19.0 and TR.needed(0.05, 0.95, 21) == (3, 2) and HM.tail_size(0.1, 21) == 3


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_tail_size_is_enough_and_one_less_is_not(alpha, m):
    q_lo, q_hi = alpha / 2, 1 - alpha / 2
    K = HM.tail_size(alpha, m)
    n_lo, n_hi = TR.needed(q_lo, q_hi, m)
    assert isinstance(K, int) and 1 <= K <= m and K == min(m, max(n_lo, n_hi))
    rs = np.random.RandomState(1000 * m + int(alpha * 100))
    for kind in ("random", "random", "ties", "constant"):
        y = _series(rs, m, kind)
        assert y.shape == (m,) and y.dtype == np.float32
        srt = np.sort(y)
        want = TR.full_quantiles(y, q_lo, q_hi)
        got = TR.tail_quantiles(srt[:K], srt[m - K:], m, q_lo, q_hi)
        assert got == want and got[0].dtype == np.float32, (kind, got, want)
        if kind != "constant":
            ref = np.quantile(y.astype(np.float64), [q_lo, q_hi])              # NumPy's own rule, in float64 on the float32 values
            assert np.allclose(np.array(want, np.float64), ref, rtol=2e-7, atol=0)
        if K < m:                                                              # K - 1 values a side are too few
            with pytest.raises(ValueError, match="the bounds read"):
                TR.tail_quantiles(srt[:K - 1], srt[m - K + 1:], m, q_lo, q_hi)
            assert max(n_lo, n_hi) > K - 1


@pytest.mark.parametrize("m,alpha", [(1, 0.5), (5, 0.9), (20, 0.1), (21, 0.1), (400, 0.05), (400, 0.01), (3000, 0.01)])
def test_the_set_update_keeps_the_k_smallest_and_the_k_largest(m, alpha):
    """the heap update draw by draw, ties at the threshold included: as multisets tail 0 is sort(y)[:K] and tail 1 sort(y)[-K:], and
    the finisher on them gives the bounds of the full series"""
    K = HM.tail_size(alpha, m)
    rs = np.random.RandomState(m + 7)
    for kind in ("random", "ties", "constant"):
        y = _series(rs, m, kind)
        t0, t1 = TR.tails_of(y, K)
        srt = np.sort(y)
        assert np.array_equal(np.sort(t0), srt[:K]) and np.array_equal(np.sort(t1), srt[m - K:]), kind
        assert t0[0] == srt[K - 1] and t1[0] == srt[m - K]                     # the thresholds sit at slot 0
        assert TR.tail_quantiles(t0, t1, m, alpha / 2, 1 - alpha / 2) == TR.full_quantiles(y, alpha / 2, 1 - alpha / 2)
        # a run cut after any draw is the same run: the state is the buffer alone
        cut = min(m, K + 3)
        a0, a1 = TR.tails_of(y, K, stop=cut)
        for d in range(cut, m):
            TR.tail_push(a0, K, d, y[d], True)
            TR.tail_push(a1, K, d, y[d], False)
        assert np.array_equal(a0, t0) and np.array_equal(a1, t1)


def test_tail_size_at_the_sizes_of_the_documents():
    assert HM.tail_size(0.01, 3000) == 16 and HM.tail_size(0.05, 3000) == 76
    assert HM.tail_size(0.0, 50) == 2 and HM.tail_size(1.0, 50) == 26 and HM.tail_size(0.01, 1) == 1 and HM.tail_size(0.01, 2) == 2
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="alpha"):
            HM.tail_size(bad, 10)
    with pytest.raises(ValueError, match="m must be"):
        HM.tail_size(0.05, 0)


def test_tails_row_blocks():
    shard = [(100, 2000000)]
    assert (2 << 30) // (8 * 16 * 20) == 838860 and HM.tails_block_rows(16, 20) == 838860 // 16 * 16 == 838848
    assert HM.tails_block_rows(76, 20) == (2 << 30) // (8 * 76 * 20) // 16 * 16 == 176592
    cut = HM.individual_blocks(shard, 3000, 20, "tails", k_tail=16)
    assert cut == [(100, 838948), (838948, 1677796), (1677796, 2000000)]
    assert HM.individual_blocks(shard, 3000, 20, "normal") == shard and len(HM.individual_blocks(shard, 3000, 20, "quantile")) == 224
    small = HM.individual_blocks([(0, 96)], 20, 5, "tails", 8 * 3 * 5 * 32, k_tail=3)              # 32 rows a block
    assert small == [(0, 32), (32, 64), (64, 96)]
    assert HM.tails_block_rows(3, 5, 8 * 3 * 5 * 47) == 32 and HM.tails_block_rows(3000, 20, 1) == 16      # whole tiles, at least one
    with pytest.raises(ValueError, match="draw_budget_bytes"):
        HM.individual_blocks(shard, 20, 5, "tails", 0, k_tail=3)
    # the unchanged routes take no notice of k_tail
    assert HM.individual_blocks([(0, 96)], 20, 5, "quantile", 4 * 20 * 5 * 32, k_tail=3) == [(0, 32), (32, 64), (64, 96)]


def test_abi_declares_the_two_entry_points():
    from bayesgm_amd import _lib
    import ctypes as C
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    for name in ("bgm_causal_hmc_run_row_tails", "bgm_row_tail_quantiles"):
        assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
    rows, tails = _lib.SYMBOLS["bgm_causal_hmc_run_row_effects"], _lib.SYMBOLS["bgm_causal_hmc_run_row_tails"]
    assert tails[0] is C.c_int and tails[1] == rows[1][:-1] + [C.c_void_p, C.c_int32, C.c_void_p]      # + row_tails_dev, k_tail before the stream
    assert "float *row_draws_dev,\n" in header and "float *row_tails_dev, int32_t k_tail, void *stream);" in header
    assert _lib.SYMBOLS["bgm_row_tail_quantiles"][1] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]
    src = open(os.path.join(root, "bayesgm_amd", "csrc", "build.py")).read()
    assert '"causal_hmc_tails_api.hip"' in src and '"causal_hmc_rowfx_api.hip"' in src
    from bayesgm_amd.engine import CausalEngine
    assert callable(CausalEngine.hmc_run_rows_tails) and callable(CausalEngine.row_tail_quantiles)


def _bare(cls, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def _error(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


def test_refusals_new_and_unchanged():
    from bayesgm_amd.models.causalbgm import CausalBGM
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    ok = _bare(CausalBGM)
    # an unknown interval: the sentence of before, verbatim, and the new mode named after it
    for msg in (_error(ok.predict_individual, DATA, [0.0], interval="hpd"), _error(ok.predict_new, DATA[2], None, [0.0], interval="hpd")):
        assert "interval must be 'normal' or 'quantile'; got 'hpd'" in msg and "'tails'" in msg
    # 'tails' stores something per row: a budget is allowed and must be positive; 'normal' still has nothing to bound
    assert "draw_budget_bytes must be positive" in _error(ok.predict_individual, DATA, [0.0], interval="tails", draw_budget_bytes=0)
    assert "draw_budget_bytes must be positive" in _error(ok.predict_new, DATA[2], None, [0.0], interval="tails", draw_budget_bytes=-1)
    msg = _error(ok.predict_individual, DATA, [0.0], draw_budget_bytes=1 << 20)
    assert "interval='normal'" in msg and "draw_budget_bytes" in msg
    assert "x_values" in _error(ok.predict_individual, DATA, None, interval="tails")
    assert "groups must be integer labels" in _error(ok.predict_individual, DATA, [0.0], interval="tails", groups=np.zeros(3, np.int64))
    binary = _bare(CausalBGM)
    binary._p["binary_treatment"] = True
    msg = _error(binary.predict_individual, DATA, [0.0], interval="tails")
    assert "binary" in msg and "predict's ITE" in msg and msg == _error(binary.predict_individual, DATA, [0.0])
    msg = _error(binary.predict_new, DATA[2], None, interval="tails")
    assert "interval='tails'" in msg and "ITE route" in msg
    # the refusals of the HMC sampler and of the subclasses come first and stay word for word
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(mass="dense"), "mass must be"),
                     (dict(mass="diag", burn_in=10), "burn_in >= 20")):
        msg = _error(ok.predict_individual, DATA, [0.0], interval="tails", **kw)
        assert word in msg and msg == _error(ok.predict, DATA, x_values=[0.0], sampler="hmc", **kw)
    split = _bare(CausalBGM)
    split._p["mh_precision"] = "f16x3"
    msg = _error(split.predict_individual, DATA, [0.0], interval="tails")
    assert "mh_precision" in msg and msg == _error(split.predict, DATA, x_values=[0.0], sampler="hmc")
    for cls, params, word in ((IdentifiableCausalBGM, dict(n_segments=3), "IdentifiableCausalBGM"), (CausalBGMBayes, dict(), "not available for CausalBGMBayes")):
        m = _bare(cls, **params)
        want = _error(m.predict, DATA, x_values=[0.0], sampler="hmc")
        assert word in want and _error(m.predict_individual, DATA, [0.0], interval="tails") == want
    bnn = _bare(CausalBGMBayes)
    bnn._p["use_bnn"] = True
    msg = _error(bnn.predict_individual, DATA, [0.0], interval="tails")
    assert "use_bnn" in msg and msg == _error(bnn.predict, DATA, x_values=[0.0], sampler="hmc")
