"""Latent-dimension split of CausalBGM: ``estimate_latent_dims``, ``get_SDR_dim`` and ``slice_y``.

Names, signatures, defaults and return shapes follow the reference's ``bayesgm.utils`` (utils/helpers.py:69-222); the code is
the build's own.  The reference standardises the data, takes two economic QRs of the N x p panel (one per sliced inverse
regression) and a full PCA.  All three need only the first and second moments of V and its per-slice column sums, so here:

  * the slices are labelled on the device (``torch.unique`` / ``searchsorted``: only the <= n_slices + 1 slice boundaries
    reach the host);
  * one HIP pass over V (``bgm_sdr_moments``, csrc/sdr_kernels.h) returns, in float64, the column sums, the slice sums of both
    labelings and the Gram matrix of V shifted by its first row;
  * the host finishes in float64 NumPy: centring, the correlation matrix Corr = D^-1 (G / n) D^-1, ONE ``eigh`` of it, which
    gives PCA's explained-variance ratios (eig(Corr) / trace(Corr)) and the whitening U L^-1/2 of both SIR problems, whose
    matrices M = R^-T B R^-1 (B = sum_k s_k s_k^T / c_k, s_k the centred slice sums, G = R^T R) have the eigenvalues of the
    whitened B.

Deviations from the reference (DESIGN.md section "Latent dimensions"): everything is float64 where the reference runs float32
LAPACK on float32 input; y is sliced on its own values (the reference slices float32-standardised y, which can merge
neighbouring values into ties); whitening uses the pseudo-inverse square root of Corr (eigenvalues below 1e-12 of the largest
are dropped), which equals the QR form at full rank and gives a defined answer for constant or collinear columns.

There is no CPU path: ``estimate_latent_dims`` and ``get_SDR_dim`` run on the current HIP device.
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib

_RANK_TOL = 1e-12            # pseudo-inverse square root: eigenvalues of Corr below this fraction of the largest are dropped
MAX_P = 2048                 # limits of the moment kernel (bgm_sdr_moments)
MAX_SLICES = 1024


# ---------------------------------------------------------------------------------------------------------------------
# slicing (helpers.py:69-137)
# ---------------------------------------------------------------------------------------------------------------------
def _partition(cum, n, n_slices):
    """Slice boundaries (positions in the sorted order) from the cumulative counts `cum` of the sorted unique values: each
    value its own slice when n_slices >= the number of unique values, else the greedy rule -- a slice ends at the first
    unique value whose cumulative count reaches (start + floor(n / n_slices)), until fewer than 3 rows remain."""
    cum = np.asarray(cum, dtype=np.int64)
    if n_slices >= cum.shape[0]:
        return np.concatenate(([0], cum))
    step = n // n_slices
    bounds, seen = [0], 0
    while seen < n - 2:
        k = min(int(np.searchsorted(cum, seen + step, side="left")), cum.shape[0] - 1)
        seen = int(cum[k])
        bounds.append(seen)
    return np.asarray(bounds, dtype=np.int64)


def _check_unique(n_unique, n_slices):
    if n_unique == 1:
        raise ValueError("The target only has one unique y value. It does not make sense to fit SIR or SAVE in this case.")
    if n_slices > n_unique:
        warnings.warn("n_slices greater than the number of unique y values. Setting n_slices equal to {0}.".format(n_unique))


def _indicator_from_bounds(bounds, n):
    """Slice of every sorted position: slice j spans bounds[j] .. bounds[j + 1], the last one runs to the end (a partition
    without a slice leaves every row in slice 1, as the reference does)."""
    ind = np.ones(n, dtype=np.int64)
    m = bounds.shape[0] - 1
    for j in range(m):
        ind[bounds[j]:(bounds[j + 1] if j < m - 1 else n)] = j
    return ind


def slice_y(y, n_slices=10):
    """Non-overlapping slices of the target y: ``(slice_indicator, slice_counts)``.

    ``slice_indicator[i]`` is the slice of the i-th observation in the SORTED order of y (as the reference, which is called on
    sorted data); tied values always share a slice.  When ``n_slices`` exceeds the number of unique values every value gets its
    own slice (with a warning); a single unique value is a ``ValueError``."""
    y = np.asarray(y)
    n = y.shape[0]
    uniq, counts = np.unique(y, return_counts=True)
    _check_unique(uniq.shape[0], n_slices)
    bounds = _partition(np.cumsum(counts), n, n_slices)
    ind = _indicator_from_bounds(bounds, n)
    return ind, np.bincount(ind)


# ---------------------------------------------------------------------------------------------------------------------
# host finishing (float64 NumPy)
# ---------------------------------------------------------------------------------------------------------------------
def _threshold_count(vals, ratio, return_margin=False):
    """argmax(cumsum(vals) >= ratio * sum(vals)) + 1 over `vals` in descending order; with return_margin also the smallest
    distance |cumsum / sum - ratio| (how far the answer is from flipping)."""
    vals = np.sort(np.asarray(vals, dtype=np.float64))[::-1]
    total = vals.sum()
    cum = np.cumsum(vals)
    k = int(np.argmax(cum >= ratio * total)) + 1
    if not return_margin:
        return k
    margin = float(np.min(np.abs(cum / total - ratio))) if total != 0 else 0.0
    return k, margin


class _Moments:
    """Centred float64 moments of V from the (shifted) sums: n, mean, centred Gram, and the eigen-decomposition of Corr."""

    def __init__(self, n, colsum, gram):
        self.n = float(n)
        shifted_mean = np.asarray(colsum, dtype=np.float64) / self.n
        self.shifted_mean = shifted_mean
        g = np.asarray(gram, dtype=np.float64) - self.n * np.outer(shifted_mean, shifted_mean)
        g = 0.5 * (g + g.T)
        var = np.maximum(np.diag(g) / self.n, 0.0)
        sd = np.sqrt(var)
        sd[sd == 0.0] = 1.0                               # StandardScaler: a constant column keeps scale 1
        self.sd = sd
        corr = g / self.n / np.outer(sd, sd)
        w, u = np.linalg.eigh(0.5 * (corr + corr.T))
        self.w, self.u = w, u
        keep = w > _RANK_TOL * max(w.max(), 0.0)
        self.whiten = u[:, keep] / np.sqrt(w[keep])       # (p, rank): W^T Corr W = I

    def pca_ratio(self):
        """PCA's explained_variance_ratio_ of the standardised panel (descending)."""
        w = np.clip(self.w[::-1], 0.0, None)
        return w / w.sum()

    def sir_eigenvalues(self, slice_sums, counts):
        """Eigenvalues (descending) of the SIR matrix of one labeling from its shifted slice sums [S, p] and counts [S]."""
        counts = np.asarray(counts, dtype=np.float64)
        sums = np.asarray(slice_sums, dtype=np.float64)
        nz = counts > 0
        centred = sums[nz] - counts[nz, None] * self.shifted_mean[None, :]
        t = (centred / self.sd[None, :]) @ self.whiten / np.sqrt(self.n * counts[nz])[:, None]     # rows: whitened slice means
        return np.linalg.eigvalsh(t.T @ t)[::-1]


def _sdr_dim(mom, slice_sums, counts, ratio, return_margin=False):
    return _threshold_count(mom.sir_eigenvalues(slice_sums, counts), ratio, return_margin)


def _latent_dims_from_moments(mom, sums_y, counts_y, sums_x, counts_x, v_ratio=0.7, z0_dim=3, max_total_dim=64, min_z3_dim=3):
    """The split [z0, z1, z2, z3] of estimate_latent_dims from float64 moments (the host half of the function)."""
    z1 = _sdr_dim(mom, sums_y, counts_y, 0.8)
    z2 = _sdr_dim(mom, sums_x, counts_x, 0.8)
    total = min(max_total_dim, int(np.argmax(np.cumsum(mom.pca_ratio()) >= v_ratio)) + 1)
    z3 = total - z0_dim - z1 - z2
    if z3 <= min_z3_dim:
        z3 = min_z3_dim
    return [int(z0_dim), int(z1), int(z2), int(z3)]


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
_handles = {}


def _handle(index):
    if index not in _handles:
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.bgm_create(C.byref(h), index), "bgm_create")
        _handles[index] = h
    return _handles[index]


def _as_device(a, device, name):
    """A 2-D float32 / float64 device tensor view of `a` (NumPy or torch); device tensors are used in place."""
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64 if t.dtype in (torch.int64, torch.int32, torch.uint8, torch.int16, torch.int8, torch.bool) else
                 torch.float32)
    if t.device != device:
        t = t.to(device, non_blocking=False)
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2:
        raise ValueError("%s must be 1-D or 2-D, got shape %s" % (name, tuple(t.shape)))
    return t


def _as_target(a, device, n, name):
    t = _as_device(a, device, name)
    if t.shape[1] != 1:
        raise ValueError("The shape of %s should be (n_samples, 1)." % name)
    if t.shape[0] != n:
        raise ValueError("%s has %d rows, the covariates %d" % (name, t.shape[0], n))
    return t[:, 0]


def _finite(t, name):
    import torch
    if not bool(torch.isfinite(t).all()):
        raise ValueError("%s contains NaN or inf" % name)


def _device_slices(y, n_slices):
    """int32 slice labels of every row of the device vector y (in its own order) and the slice counts (host)."""
    import torch
    n = y.shape[0]
    uniq, inverse, counts = torch.unique(y, sorted=True, return_inverse=True, return_counts=True)
    n_unique = int(uniq.shape[0])
    _check_unique(n_unique, n_slices)
    cum = torch.cumsum(counts, 0)
    if n_slices >= n_unique:
        labels = inverse
    else:
        # the greedy rule of _partition on the device: at most ceil(n / step) + 1 steps, no host round trip in between
        step = n // n_slices
        seen = torch.zeros((), dtype=cum.dtype, device=y.device)
        bounds = [seen]
        for _ in range(min(n_unique, -(-n // step) + 1)):
            k = torch.clamp(torch.searchsorted(cum, seen + step, side="left"), max=n_unique - 1)
            seen = torch.where(seen < n - 2, cum[k], seen)
            bounds.append(seen)
        b = torch.unique_consecutive(torch.stack(bounds)).cpu().numpy()       # the only transfer: <= n_slices + 1 boundaries
        if b.shape[0] == 1:                                                     # no slice formed: every row in slice 1
            labels = torch.ones_like(inverse)
        else:
            inner = torch.as_tensor(b[1:-1], device=y.device, dtype=cum.dtype)
            start = cum - counts                                                # first sorted position of every unique value
            labels = torch.searchsorted(inner, start, side="right")[inverse]
    labels = labels.to(torch.int32)
    counts_out = torch.bincount(labels.to(torch.int64)).cpu().numpy()
    return labels.contiguous(), counts_out


def _moments_device(v, labelings):
    """(n, colsum, [slice sums], gram) in float64 NumPy from one bgm_sdr_moments pass over the device matrix v."""
    import torch
    n, p = v.shape
    if v.stride(1) != 1:
        v = v.contiguous()
    dev = v.device
    lib = _lib.load()
    h = _handle(dev.index if dev.index is not None else torch.cuda.current_device())
    shift = v[0].to(torch.float64).contiguous()
    s = [int(c.shape[0]) for _, c in labelings] + [0] * (2 - len(labelings))
    for k in s:
        if k > MAX_SLICES:
            raise ValueError("estimate_latent_dims: %d slices exceed the kernel limit of %d slices per labeling" % (k, MAX_SLICES))
    ws_bytes = C.c_int64()
    _lib.check(lib.bgm_sdr_moments_workspace(h, n, p, s[0], s[1], C.byref(ws_bytes)), "bgm_sdr_moments_workspace")
    ws = torch.empty(max(1, (ws_bytes.value + 7) // 8), dtype=torch.float64, device=dev)
    out = torch.empty((1 + s[0] + s[1]) * p + p * p, dtype=torch.float64, device=dev)
    labs = [lab.data_ptr() for lab, _ in labelings] + [None] * (2 - len(labelings))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.bgm_sdr_moments(h, C.c_void_p(v.data_ptr()), int(v.dtype == torch.float64), n, p, v.stride(0),
                                   C.c_void_p(shift.data_ptr()), labs[0], s[0], labs[1], s[1], C.c_void_p(out.data_ptr()),
                                   C.c_void_p(ws.data_ptr()), ws.numel() * 8, stream), "bgm_sdr_moments")
    o = out.cpu().numpy()
    sums, off = [], p
    for k in s[:len(labelings)]:
        sums.append(o[off:off + k * p].reshape(k, p))
        off += k * p
    gram = o[(1 + s[0] + s[1]) * p:].reshape(p, p)
    return n, o[:p], sums, gram


def _prepare(v, name="v"):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bayesgm_amd: estimate_latent_dims / get_SDR_dim run on a HIP device; none is available "
                           "(there is no CPU path)")
    device = torch.device("cuda", torch.cuda.current_device()) if not (isinstance(v, torch.Tensor) and v.is_cuda) else v.device
    vt = _as_device(v, device, name)
    n, p = vt.shape
    if p > MAX_P:
        raise ValueError("%s has %d columns: the moment kernel's limit is p <= %d" % (name, p, MAX_P))
    if n <= p:
        raise ValueError("%s has %d rows and %d columns: need more rows than columns (N > p)" % (name, n, p))
    _finite(vt, name)
    return vt, device


def get_SDR_dim(X, y, n_slices=10, ratio=0.8):
    """Dimension of the sufficient dimension reduction of X for y by sliced inverse regression: the number of leading
    eigenvalues of the SIR matrix whose cumulative sum reaches `ratio` of the total.  X: (n, p); y: (n,) or (n, 1); NumPy
    arrays or torch tensors (device tensors are used in place).  Runs on the current HIP device."""
    xt, device = _prepare(X, "X")
    yt = _as_target(y, device, xt.shape[0], "y")
    _finite(yt, "y")
    labels, counts = _device_slices(yt, n_slices)
    n, colsum, sums, gram = _moments_device(xt, [(labels, counts)])
    return _sdr_dim(_Moments(n, colsum, gram), sums[0], counts, ratio)


def estimate_latent_dims(x, y, v, v_ratio=0.7, z0_dim=3, max_total_dim=64, min_z3_dim=3):
    """Latent-dimension split ``[z0, z1, z2, z3]`` of CausalBGM for a data set: z1 = SIR dimension of V for y, z2 = SIR
    dimension of V for x (ratio 0.8, 10 slices each), total = number of principal components of standardised V that explain
    `v_ratio` of its variance (at most `max_total_dim`), z3 = total - z0 - z1 - z2, raised to `min_z3_dim` when it is not above
    it.  x, y: (n,) or (n, 1); v: (n, p); NumPy arrays or torch tensors (device tensors are used in place).  One pass of the
    moment kernel over V on the current HIP device."""
    vt, device = _prepare(v, "v")
    n = vt.shape[0]
    yt = _as_target(y, device, n, "y")
    xt = _as_target(x, device, n, "x")
    _finite(yt, "y")
    _finite(xt, "x")
    lab_y, cnt_y = _device_slices(yt, 10)
    lab_x, cnt_x = _device_slices(xt, 10)
    _, colsum, sums, gram = _moments_device(vt, [(lab_y, cnt_y), (lab_x, cnt_x)])
    return _latent_dims_from_moments(_Moments(n, colsum, gram), sums[0], cnt_y, sums[1], cnt_x, v_ratio=v_ratio, z0_dim=z0_dim,
                                     max_total_dim=max_total_dim, min_z3_dim=min_z3_dim)
