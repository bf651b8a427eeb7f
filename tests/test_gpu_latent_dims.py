"""bgm_sdr_moments (csrc/sdr_kernels.h) against float64 NumPy, and estimate_latent_dims / get_SDR_dim on the GPU against the
reference's results (tests/golden/latent_dims.npz)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _latent_dims_panels import ESTIMATED, GOLDEN, N_SLICES, RATIOS, SETTINGS, panels  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1e-5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a HIP device")
    return t


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "latent_dims.npz")) as f:
        return {k: f[k] for k in f.files}


def kernel_moments(torch, v, labs, s, shift=None, ldv=None):
    """raw bgm_sdr_moments output (NumPy) for device v [n, ldv] (first p columns used)"""
    import ctypes as C
    from bayesgm_amd import _lib
    from bayesgm_amd.latent_dims import _handle
    lib = _lib.load()
    n, p = v.shape
    h = _handle(torch.cuda.current_device())
    ws_bytes = C.c_int64()
    _lib.check(lib.bgm_sdr_moments_workspace(h, n, p, s[0], s[1], C.byref(ws_bytes)), "ws")
    ws = torch.empty(max(1, ws_bytes.value // 8), dtype=torch.float64, device="cuda")
    out = torch.full(((1 + s[0] + s[1]) * p + p * p,), float("nan"), dtype=torch.float64, device="cuda")
    ptr = [l.data_ptr() if l is not None else None for l in labs]
    rc = lib.bgm_sdr_moments(h, C.c_void_p(v.data_ptr()), int(v.dtype == torch.float64), n, p, v.stride(0),
                             C.c_void_p(shift.data_ptr()) if shift is not None else None, ptr[0], s[0], ptr[1], s[1],
                             C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel() * 8, None)
    _lib.check(rc, "bgm_sdr_moments")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def numpy_reference(v, labs, s, shift):
    """the same rectangle in float64 NumPy, and the entrywise bound sum |a b| of each entry"""
    w = v.astype(np.float64) - (shift if shift is not None else 0.0)
    n, p = w.shape
    a = [np.ones((n, 1))]
    for lab, k in zip(labs, s):
        if k:
            a.append((lab[:, None] == np.arange(k)[None, :]).astype(np.float64))
    a = np.concatenate(a, 1)
    ext, ext_abs = a.T @ w, a.T @ np.abs(w)
    return np.concatenate([ext.ravel(), (w.T @ w).ravel()]), np.concatenate([ext_abs.ravel(), (np.abs(w).T @ np.abs(w)).ravel()])


GRID = [(1, 1, (2, 0)), (3, 15, (10, 2)), (4097, 16, (64, 10)), (4097, 17, (2, 1024)), (100003, 200, (10, 10)),
        (4097, 500, (10, 2)), (3, 200, (1024, 0)), (100003, 17, (0, 0))]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,p,s", GRID)
def test_kernel_moments_match_numpy(torch, dtype, n, p, s):
    rs = np.random.RandomState(n + p)
    sd = np.exp(rs.randn(p))
    v = (rs.randn(n, p) * sd + 1e4 * sd).astype(np.float32 if dtype == "f32" else np.float64)    # columns offset by 1e4 sd
    labs = [rs.randint(0, k, size=n).astype(np.int32) if k else None for k in s]
    shift = v[0].astype(np.float64)
    vd = torch.from_numpy(v).cuda()
    ld = [torch.from_numpy(l).cuda() if l is not None else None for l in labs]
    got = kernel_moments(torch, vd, ld, s, torch.from_numpy(shift).cuda())
    want, bound = numpy_reference(v, labs, s, shift)
    err = np.abs(got - want)
    assert np.all(err <= 1e-10 * bound + 1e-300), (err / np.maximum(bound, 1e-300)).max()


def test_kernel_exact_integers_whole_rectangle(torch):
    """small integers are exact in float64: the whole (extra rows + Gram) rectangle must match bit for bit, so that a C/D-layout
    or mirroring error cannot hide in a symmetric block; non-default leading dimension, no shift"""
    rs = np.random.RandomState(3)
    n, p, ldv = 1001, 37, 45
    full = rs.randint(-4, 5, size=(n, ldv)).astype(np.float32)
    full[:, p:] = 1e30                                     # past column p: must never be read into the result
    vd = torch.from_numpy(full).cuda()[:, :p]
    assert vd.stride(0) == ldv
    labs = [rs.randint(0, 7, size=n).astype(np.int32), rs.randint(0, 19, size=n).astype(np.int32)]
    got = kernel_moments(torch, vd, [torch.from_numpy(l).cuda() for l in labs], (7, 19))
    want, _ = numpy_reference(full[:, :p], labs, (7, 19), None)
    np.testing.assert_array_equal(got, want)
    gram = got[(1 + 7 + 19) * p:].reshape(p, p)
    assert not np.array_equal(gram[:16, 16:32], gram[16:32, :16])      # asymmetric off-diagonal blocks are placed right


def test_kernel_is_deterministic(torch):
    rs = np.random.RandomState(5)
    v = torch.from_numpy(rs.randn(50001, 200).astype(np.float32)).cuda()
    lab = [torch.from_numpy(rs.randint(0, 10, size=50001).astype(np.int32)).cuda() for _ in range(2)]
    a = kernel_moments(torch, v, lab, (10, 10), v[0].double().contiguous())
    b = kernel_moments(torch, v, lab, (10, 10), v[0].double().contiguous())
    assert a.tobytes() == b.tobytes()


def test_kernel_limits(torch):
    import ctypes as C
    from bayesgm_amd import _lib
    from bayesgm_amd.latent_dims import _handle
    lib = _lib.load()
    h = _handle(torch.cuda.current_device())
    b = C.c_int64()
    assert lib.bgm_sdr_moments_workspace(h, 100, 2049, 10, 10, C.byref(b)) == -4
    assert b"2048" in lib.bgm_last_error()
    assert lib.bgm_sdr_moments_workspace(h, 100, 20, 1025, 10, C.byref(b)) == -4
    assert b"1024" in lib.bgm_last_error()
    assert lib.bgm_sdr_moments_workspace(h, 100, 2048, 1024, 1024, C.byref(b)) == 0


@pytest.mark.parametrize("name", ["hi", "ties", "binary", "n7", "f64"])
@pytest.mark.parametrize("ns", [5, 10, 20])
def test_device_labels_equal_host_slice_y(torch, name, ns):
    from bayesgm_amd.latent_dims import _device_slices, slice_y
    y = panels()[name][1][:, 0]
    order = np.argsort(y, kind="stable")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ind, cnt = slice_y(y[order], ns)
        lab, cnt_d = _device_slices(torch.from_numpy(y).cuda(), ns)
    want = np.empty_like(ind)
    want[order] = ind
    np.testing.assert_array_equal(lab.cpu().numpy(), want)
    np.testing.assert_array_equal(cnt_d, cnt)


def _margins(x, y, v, setting):
    """float64 margins of the three thresholds of a setting (the host restatement on NumPy moments)"""
    from test_latent_dims_host import _host_estimate
    return _host_estimate(x, y, v, setting)[1]


@pytest.mark.parametrize("form", ["numpy", "torch_device", "float64"])
def test_estimate_latent_dims_matches_reference(torch, gold, form):
    from bayesgm_amd.utils import estimate_latent_dims
    data = panels()
    skipped = 0
    for name in ESTIMATED:
        x, y, v = data[name]
        if form == "torch_device":
            args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, y, v)]
        elif form == "float64":
            args = [a.astype(np.float64) for a in (x, y, v)]
        else:
            args = [x, y[:, 0], v]                           # (n,) targets are accepted too
        for setting, want in zip(SETTINGS, gold[name + "_estimate"]):
            if _margins(x, y, v, setting) < MARGIN:
                skipped += 1
                continue
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = estimate_latent_dims(*args, *setting)
            assert got == [int(t) for t in want], (name, setting, got, want)
            assert all(type(t) is int for t in got)
    assert skipped <= 3


def test_get_sdr_dim_sweep_matches_reference(torch, gold):
    from bayesgm_amd.utils import get_SDR_dim
    from test_latent_dims_host import labels_of, numpy_moments
    from bayesgm_amd import latent_dims as LD
    data = panels()
    skipped = total = 0
    for name in ["hi", "ties", "binary", "offset", "f64"]:
        x, y, v = data[name]
        vd = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        for target, t in (("y", y), ("x", x)):
            want = gold["%s_sdr_%s" % (name, target)]
            td = torch.from_numpy(np.ascontiguousarray(t)).cuda()
            for i, ns in enumerate(N_SLICES):
                lab, cnt = labels_of(t, ns)
                n, colsum, (s,), gram = numpy_moments(v, [(lab, cnt)])
                mom = LD._Moments(n, colsum, gram)
                for j, r in enumerate(RATIOS):
                    total += 1
                    if LD._sdr_dim(mom, s, cnt, r, True)[1] < MARGIN:
                        skipped += 1
                        continue
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        got = get_SDR_dim(vd, td, ns, r)
                    assert type(got) is int and got == want[i, j], (name, target, ns, r, got, want[i, j])
    assert skipped <= 0.02 * total


def test_error_paths(torch):
    from bayesgm_amd.utils import estimate_latent_dims, get_SDR_dim
    rs = np.random.RandomState(0)
    v = rs.randn(100, 5).astype(np.float32)
    x, y = rs.randn(100, 1), rs.randn(100, 1)
    bad = v.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or inf"):
        estimate_latent_dims(x, y, bad)
    yi = y.copy()
    yi[0] = np.inf
    with pytest.raises(ValueError, match="NaN or inf"):
        get_SDR_dim(v, yi)
    with pytest.raises(ValueError, match="N > p"):
        estimate_latent_dims(x[:5], y[:5], v[:5])
    with pytest.raises(ValueError, match="1024 slices"):
        get_SDR_dim(rs.randn(3000, 4), rs.randn(3000), n_slices=2000)
    with pytest.raises(ValueError, match="2048"):
        get_SDR_dim(np.zeros((2100, 2049), np.float32), rs.randn(2100))


def test_constant_column(torch, gold):
    """rank-deficient V: the GPU result equals the float64 pseudo-inverse restatement, and the PCA part equals sklearn"""
    from bayesgm_amd import latent_dims as LD
    from test_latent_dims_host import labels_of, numpy_moments
    x, y, v = panels()["const"]
    vt = torch.from_numpy(v).cuda()
    ly, cy = LD._device_slices(torch.from_numpy(y[:, 0]).cuda(), 10)
    lx, cx = LD._device_slices(torch.from_numpy(x[:, 0]).cuda(), 10)
    n, colsum, (sy, sx), gram = LD._moments_device(vt, [(ly, cy), (lx, cx)])
    mom = LD._Moments(n, colsum, gram)
    np.testing.assert_allclose(mom.pca_ratio(), gold["const_pca_ratio"], rtol=0, atol=1e-5)
    hy, hcy = labels_of(y, 10)
    hx, hcx = labels_of(x, 10)
    hn, hcol, (hsy, hsx), hgram = numpy_moments(v, [(hy, hcy), (hx, hcx)])
    hmom = LD._Moments(hn, hcol, hgram)
    np.testing.assert_allclose(mom.sir_eigenvalues(sy, cy), hmom.sir_eigenvalues(hsy, hcy), rtol=1e-9, atol=1e-12)
    assert mom.whiten.shape[1] == v.shape[1] - 1
    want = LD._latent_dims_from_moments(hmom, hsy, hcy, hsx, hcx)
    assert LD.estimate_latent_dims(x, y, v) == want
