"""estimate_latent_dims / get_SDR_dim / slice_y without a GPU: slicing, and the float64 host finishing fed with NumPy moments,
against the reference's own results (tests/golden/latent_dims.npz, tests/golden/make_latent_dims_golden.py)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _latent_dims_panels import ESTIMATED, GOLDEN, N_SLICES, RATIOS, SETTINGS, panels  # noqa: E402

from bayesgm_amd import latent_dims as LD  # noqa: E402
from bayesgm_amd.utils import estimate_latent_dims, get_SDR_dim, slice_y  # noqa: E402

MARGIN = 1e-5


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "latent_dims.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def data():
    return panels()


def labels_of(t, n_slices):
    """slice labels of the rows of t in their own order (the host rule of slice_y applied to the sorted values)"""
    t = np.asarray(t).reshape(-1)
    order = np.argsort(t, kind="stable")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ind, cnt = slice_y(t[order], n_slices)
    lab = np.empty_like(ind)
    lab[order] = ind
    return lab, cnt


def numpy_moments(v, labelings):
    """float64 (n, colsum, [slice sums], gram) of v shifted by its first row -- what bgm_sdr_moments returns"""
    w = np.asarray(v, dtype=np.float64)
    w = w - w[0]
    sums = []
    for lab, cnt in labelings:
        s = np.zeros((cnt.shape[0], w.shape[1]))
        np.add.at(s, lab, w)
        sums.append(s)
    return w.shape[0], w.sum(0), sums, w.T @ w


@pytest.mark.parametrize("name", ["hi", "sun", "colangelo", "ties", "binary", "n7", "offset", "f64", "const"])
@pytest.mark.parametrize("ns", N_SLICES)
def test_slice_y_matches_reference(gold, data, name, ns):
    y = np.sort(data[name][1][:, 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ind, cnt = slice_y(y, ns)
    np.testing.assert_array_equal(ind, gold["%s_slice_y_%d_ind" % (name, ns)])
    np.testing.assert_array_equal(cnt, gold["%s_slice_y_%d_cnt" % (name, ns)])
    assert ind.dtype == np.int64
    # tied values share a slice
    same = y[:-1] == y[1:]
    np.testing.assert_array_equal(ind[:-1][same], ind[1:][same])


def test_slice_y_warning_and_error():
    y = np.array([1.0, 1.0, 2.0, 3.0, 3.0, 3.0])
    with pytest.warns(UserWarning, match="n_slices greater than the number of unique y values. Setting n_slices equal to 3."):
        ind, cnt = slice_y(y, 10)
    np.testing.assert_array_equal(ind, [0, 0, 1, 2, 2, 2])
    np.testing.assert_array_equal(cnt, [2, 1, 3])
    with pytest.raises(ValueError, match="only has one unique y value"):
        slice_y(np.ones(5), 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        slice_y(y, 3)                      # n_slices == number of unique values: no warning


def _host_estimate(x, y, v, setting):
    ly, cy = labels_of(y, 10)
    lx, cx = labels_of(x, 10)
    n, colsum, (sy, sx), gram = numpy_moments(v, [(ly, cy), (lx, cx)])
    mom = LD._Moments(n, colsum, gram)
    margins = [LD._sdr_dim(mom, sy, cy, 0.8, True)[1], LD._sdr_dim(mom, sx, cx, 0.8, True)[1],
               float(np.min(np.abs(np.cumsum(mom.pca_ratio()) - setting[0])))]
    return LD._latent_dims_from_moments(mom, sy, cy, sx, cx, *setting), min(margins)


@pytest.mark.parametrize("name", ESTIMATED)
def test_host_finishing_reproduces_estimates(gold, data, name):
    x, y, v = data[name]
    skipped = 0
    for setting, want in zip(SETTINGS, gold[name + "_estimate"]):
        got, margin = _host_estimate(x, y, v, setting)
        if margin < MARGIN:
            skipped += 1
            continue
        assert got == [int(t) for t in want], (setting, got, want)
        assert all(type(t) is int for t in got)
    assert skipped <= 1


def test_host_finishing_reproduces_sdr_sweep(gold, data):
    skipped = total = 0
    for name in ESTIMATED:
        x, y, v = data[name]
        for target, t in (("y", y), ("x", x)):
            want = gold["%s_sdr_%s" % (name, target)]
            for i, ns in enumerate(N_SLICES):
                lab, cnt = labels_of(t, ns)
                n, colsum, (s,), gram = numpy_moments(v, [(lab, cnt)])
                mom = LD._Moments(n, colsum, gram)
                for j, r in enumerate(RATIOS):
                    got, margin = LD._sdr_dim(mom, s, cnt, r, True)
                    total += 1
                    if margin < MARGIN:
                        skipped += 1
                        continue
                    assert got == want[i, j], (name, target, ns, r, got, want[i, j])
    assert skipped <= 0.02 * total, (skipped, total)


@pytest.mark.parametrize("name", ["hi", "sun", "colangelo", "ties", "binary", "n7", "offset", "f64", "const"])
def test_host_pca_ratio_matches_sklearn(gold, data, name):
    v = data[name][2]
    n, colsum, _, gram = numpy_moments(v, [])
    got = LD._Moments(n, colsum, gram).pca_ratio()
    np.testing.assert_allclose(got, gold[name + "_pca_ratio"], rtol=0, atol=1e-5)


def test_threshold_rule():
    assert LD._threshold_count([1.0, 1.0, 2.0], 0.5) == 1
    assert LD._threshold_count([3.0, 1.0], 0.75) == 1
    assert LD._threshold_count([3.0, 1.0], 0.76) == 2
    k, margin = LD._threshold_count([3.0, 1.0], 0.76, return_margin=True)
    assert k == 2 and abs(margin - 0.01) < 1e-12


def test_public_names_are_the_bayesgm_amd_objects():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat"))
    try:
        import bayesgm.utils as U
        import bayesgm.utils.helpers as H
    finally:
        sys.path.pop(0)
    import bayesgm_amd.utils as A
    assert U.estimate_latent_dims is A.estimate_latent_dims is LD.estimate_latent_dims
    assert "estimate_latent_dims" in U.__all__
    assert H.estimate_latent_dims is LD.estimate_latent_dims
    assert H.get_SDR_dim is LD.get_SDR_dim and H.slice_y is LD.slice_y
    assert H.get_ADRF is A.get_ADRF


def test_signatures_follow_the_reference():
    import inspect
    sig = inspect.signature(estimate_latent_dims)
    assert list(sig.parameters) == ["x", "y", "v", "v_ratio", "z0_dim", "max_total_dim", "min_z3_dim"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [0.7, 3, 64, 3]
    sig = inspect.signature(get_SDR_dim)
    assert list(sig.parameters) == ["X", "y", "n_slices", "ratio"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [10, 0.8]
    assert inspect.signature(slice_y).parameters["n_slices"].default == 10
