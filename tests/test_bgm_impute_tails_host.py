"""BGM.predict(fused_predict=True, interval='tails') / bgm_bgm_hmc_run_rows_impute_tails, host side: the block-row arithmetic at the sizes
the documents quote, the tail sizes, the binding and the keywords, the refusals that come before any device work, and the heap
restatement of tests/_causal_hmc_tails_ref.py pushed in this kernel's order -- per retained draw the head tiles in turn, in a tile
lane (j, g) owns the cells 16 tx + 4 g + r of row j, r = 0 .. 3, and pushes a missing cell's value into the series row * k_slots + slot
of a buffer [2][K][n][k_slots], tail 0 first -- which leaves, per series, sort(x)[:K] and sort(x)[-K:] on series with ties.
"""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bgm_impute_ref as IR  # noqa: E402
import _causal_hmc_tails_ref as TR  # noqa: E402

from bayesgm_amd import causal_hmc as HM  # noqa: E402


def test_tail_sizes_at_the_defaults():
    assert HM.tail_size(0.05, 5000) == 126 and HM.tail_size(0.05, 1000) == 26
    assert HM.tail_size(0.1, 40) == 3 and HM.tail_size(0.05, 6) == 2 and HM.tail_size(0.05, 1) == 1


def test_block_rows_at_the_sizes_the_documents_quote():
    from bayesgm_amd.models.bgm import impute_tails_block_rows as rows
    budget = 64 << 30      # predict's default max_draw_bytes
    # p = 500, 90 % missing: k_slots is near 470 (a row's count is binomial(500, 0.9)); 8 K k_slots bytes per row
    for K, k_slots, want in ((126, 470, (budget // (8 * 126 * 470)) // 16 * 16), (26, 470, (budget // (8 * 26 * 470)) // 16 * 16),
                             (126, 500, 136336), (126, 1, (budget // 1008) // 16 * 16)):
        assert rows(K, k_slots, budget) == want and want % 16 == 0
    assert rows(126, 470, budget) == 145040 and rows(26, 470, budget) == 702928      # against the draws route's 7 469 rows at n_mcmc = 5000
    # whole tiles, at least 16
    assert rows(3, 3, 32 * 8 * 3 * 3) == 32 and rows(3, 3, 32 * 8 * 3 * 3 + 71) == 32 and rows(3, 3, 47 * 72) == 32 and rows(3, 3, 48 * 72) == 48
    assert rows(126, 500, 1) == 16 and rows(126, 500, 8 * 126 * 500 * 31) == 16
    with pytest.raises(ValueError, match="positive"):
        rows(3, 3, 0)
    # bytes per missing-cell slot: 8 K against the draws route's 4 n_mcmc
    assert 8 * HM.tail_size(0.05, 5000) == 1008 and 4 * 5000 == 20000


def test_the_entry_point_is_bound_and_declared_and_the_keywords_exist():
    from bayesgm_amd import _lib
    from bayesgm_amd.csrc import build
    from bayesgm_amd.engine import BgmEngine, CausalEngine
    from bayesgm_amd.models.bgm import BGM
    from bayesgm_amd.models.bgm_bnn import BGMBayes
    res, args = _lib.SYMBOLS["bgm_bgm_hmc_run_rows_impute_tails"]
    impute = _lib.SYMBOLS["bgm_bgm_hmc_run_rows_impute"][1]
    # bgm_bgm_hmc_run_rows_impute's arguments, then tails_dev and k_tail before the stream
    assert res is C.c_int and args[:len(impute) - 1] == impute[:-1] and args[len(impute) - 1:] == [C.c_void_p, C.c_int32, C.c_void_p]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    assert "BGM_API int bgm_bgm_hmc_run_rows_impute_tails(" in header and "BGM_API int bgm_bgm_hmc_run_rows_impute(" in header
    assert "bgm_impute_tails_api.hip" in build.SOURCES and "bgm_impute_api.hip" in build.SOURCES
    # the heap routines live in one header that both kernel families include
    csrc = os.path.join(root, "bayesgm_amd", "csrc")
    for name in ("causal_kernels.h", "bgm_rowstep_kernels.h"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "row_tails.h"' in text and "void row_tail_push(" not in text, name
    assert open(os.path.join(csrc, "row_tails.h")).read().count("void row_tail_push(") == 1
    run = inspect.signature(BgmEngine.hmc_run_rows).parameters
    assert run["tails"].default is None and run["k_tail"].default == 0
    assert inspect.signature(BgmEngine.hmc_sample).parameters["tails"].default is None
    assert list(inspect.signature(BgmEngine.row_tail_quantiles).parameters) == list(inspect.signature(CausalEngine.row_tail_quantiles).parameters)
    for cls in (BGM, BGMBayes):
        assert inspect.signature(cls.predict).parameters["interval"].default is None


def test_the_refusals_of_interval_come_before_any_device_work():
    from bayesgm_amd.engine import BgmEngine
    from bayesgm_amd.models.bgm import BGM
    from bayesgm_amd.models.bgm_bnn import BGMBayes
    x = np.zeros((4, 5), np.float32)
    model = object.__new__(BGM)               # no engine, no device: the refusal comes before either is touched
    model.params = dict(hmc_precision="fp32")
    for kw, word in ((dict(interval="tails"), "interval='tails' needs fused_predict"), (dict(interval="normal"), "interval='normal' needs fused_predict"),
                     (dict(interval="tails", row_adapt=True), "needs fused_predict"),
                     (dict(interval="quantile", row_adapt=True, fused_predict=True), "interval='quantile'.*default route.*fused_predict"),
                     (dict(interval="hpd"), "'normal', 'quantile' or 'tails'"), (dict(interval="hpd", row_adapt=True, fused_predict=True), "'normal', 'quantile' or 'tails'"),
                     (dict(interval=0.95), "'normal', 'quantile' or 'tails'"),
                     (dict(interval="tails", fused_predict=True), "fused_predict needs row_adapt"),
                     (dict(interval="tails", row_adapt=True, fused_predict=True, return_samples=True), "return_samples"),
                     (dict(interval="tails", row_adapt=True, fused_predict=True, max_draw_bytes=0), "max_draw_bytes must be positive")):
        with pytest.raises(ValueError, match=word):
            model.predict(x, **kw)
    model.params = dict(hmc_precision="f16x3")
    with pytest.raises(ValueError, match="fused_predict.*hmc_precision"):
        model.predict(x, row_adapt=True, fused_predict=True, interval="tails")
    bayes = object.__new__(BGMBayes)
    for kw, word in ((dict(interval="tails"), "interval.*use_bnn"), (dict(interval="quantile"), "interval.*use_bnn"),
                     (dict(interval="tails", fused_predict=True), "fused_predict.*use_bnn")):      # (fused_predict is still refused first)
        with pytest.raises(ValueError, match=word):
            bayes.predict(x, **kw)
    eng = object.__new__(BgmEngine)
    with pytest.raises(ValueError, match="tails belongs to impute"):
        eng.hmc_sample(x, 4, 4, row_adapt=0.75, tails=2)
    with pytest.raises(ValueError, match="tails must be an integer K"):
        eng.hmc_sample(x, 4, 4, row_adapt=0.75, impute=True, tails=5)


def _push_in_kernel_order(values, miss, slot, k_slots, K, stop=None):
    """values [m, n, p] float32 -> tails [2, K, n, k_slots] (NaN where nothing was written), pushed as the kernel pushes: per draw the
    row tiles, per tile the head tiles tx, per lane (j, g) the registers r = 0 .. 3, tail 0 then tail 1."""
    m, n, p = values.shape
    tails = np.full((2, K, n * k_slots), np.nan, np.float32)
    for d in range(m if stop is None else stop):
        for tile in range((n + 15) // 16):
            for tx in range((p + 15) // 16):
                for lane in range(64):
                    j, g = lane & 15, lane >> 4
                    row = 16 * tile + j
                    for r in range(4):
                        c = 16 * tx + 4 * g + r
                        if row < n and c < p and miss[row, c] and slot[row, c] >= 0:
                            series = row * k_slots + slot[row, c]
                            TR.tail_push(tails[0, :, series], K, d, values[d, row, c], True)
                            TR.tail_push(tails[1, :, series], K, d, values[d, row, c], False)
    return tails.reshape(2, K, n, k_slots)


@pytest.mark.parametrize("m,K", [(6, 6), (6, 1), (6, 3), (40, 2), (60, 17), (1, 1)])
def test_heap_restatement_in_this_kernels_order_gives_the_sorted_ends(m, K):
    n, p = 19, 37      # a ragged second row tile, a last head tile that ends at column 5
    rs = np.random.RandomState(100 * m + K)
    x = rs.randn(n, p).astype(np.float32)
    x[rs.rand(n, p) < IR.MISS] = np.nan
    x[0, :] = np.nan
    x[1, :] = 0.5
    miss = np.isnan(x)
    slot, k_slots = IR.slots_of(miss)
    assert k_slots == p
    values = np.round(rs.randn(m, n, p) * 2.0).astype(np.float32) / 2.0      # a grid of 0.5: ties in every series of more than a few draws
    values[m // 2:, :, ::3] = values[:m - m // 2, :, ::3]                     # and exact repeats, as rejected transitions make them
    tails = _push_in_kernel_order(values, miss, slot, k_slots, K)
    used = np.arange(k_slots)[None, :] < miss.sum(axis=1)[:, None]
    series = np.stack([values[:, r, c] for r in range(n) for c in range(p) if miss[r, c]])      # row-major: the order of `used`
    srt = np.sort(series, axis=1)
    assert m == 1 or (srt[:, 1:] == srt[:, :-1]).any()
    got = np.sort(tails[:, :, used], axis=1)
    assert np.array_equal(got[0].T, srt[:, :K]) and np.array_equal(got[1].T, srt[:, m - K:])
    assert np.array_equal(tails[0, 0][used], srt[:, K - 1]) and np.array_equal(tails[1, 0][used], srt[:, m - K])
    assert np.isnan(tails[:, :, ~used]).all() and np.isnan(tails[:, :, 1]).all()
    # cut anywhere: the buffer after `stop` draws is a function of those draws alone (no carried state)
    if m >= 6:
        part = _push_in_kernel_order(values, miss, slot, k_slots, K, stop=4)
        srt4 = np.sort(series[:, :4], axis=1)
        k4 = min(K, 4)
        assert np.array_equal(np.sort(part[0][:k4][:, used], axis=0).T, srt4[:, :k4])
    # and the finisher on the two tails gives the quantile pair of the whole series
    if K >= HM.tail_size(0.1, m):
        for s_ in range(0, series.shape[0], 37):
            t0, t1 = tails[0][:, used][:, s_], tails[1][:, used][:, s_]
            assert TR.tail_quantiles(t0, t1, m, 0.05, 0.95) == TR.full_quantiles(series[s_], 0.05, 0.95)
