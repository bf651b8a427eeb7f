"""Thin Python driver over the C ABI (include/bgm_hip.h).

PyTorch supplies device memory and the HIP stream only; all arithmetic of the
hot path runs in libbgm_hip.so.  There is no CPU fallback: constructing an
engine without a gfx950 GPU or without the built library raises.
"""
import collections
import contextlib
import ctypes as C
import functools
import inspect

import numpy as np
import torch

from . import _lib
from . import causal_hmc as HM
from . import row_adapt as RA

DEFAULT_G_UNITS = [64, 64, 64, 64, 64]
DEFAULT_FH_UNITS = [64, 32, 8]


def flatten_net(net):
    """[(W [in,out], b [out]), ...] -> flat float32 in Keras order."""
    return np.concatenate([np.concatenate([np.asarray(W, np.float32).ravel(), np.asarray(b, np.float32).ravel()])
                           for W, b in net]).astype(np.float32)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32(t, device):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _row_tail_quantiles(eng, tails, m, q_lo, q_hi):
    """The body of CausalEngine.row_tail_quantiles and BgmEngine.row_tail_quantiles (bgm_row_tail_quantiles)."""
    if tails.dim() < 3 or tails.shape[0] != 2 or tails.dtype != torch.float32:
        raise ValueError("row_tail_quantiles: tails must be float32 [2, K, ...]; got %s %r" % (tails.dtype, tuple(tails.shape)))
    tails = tails.contiguous()
    k_tail, shape = int(tails.shape[1]), tuple(tails.shape[2:])
    n_series = int(np.prod(shape))
    lo = torch.empty(shape, device=eng.device, dtype=torch.float32)
    hi = torch.empty_like(lo)
    _lib.check(eng.lib.bgm_row_tail_quantiles(eng.h, _ptr(tails), n_series, k_tail, int(m), float(q_lo), float(q_hi), _ptr(lo), _ptr(hi),
                                              eng._stream()), "bgm_row_tail_quantiles")
    return lo, hi


def _check_buffer(who, name, t, dtype, shape, shown):
    """An output buffer of a segment: None, or a contiguous tensor of `dtype` whose shape is `shape` (None: any size there);
    ValueError naming the buffer, with `shown` for the expected shape, otherwise."""
    if t is not None and (t.dtype != dtype or not t.is_contiguous() or t.dim() != len(shape)
                          or any(want is not None and have != want for have, want in zip(t.shape, shape))):
        raise ValueError("%s: %s must be a contiguous %s tensor %s; got %s %r" %
                         (who, name, str(dtype).replace("torch.", ""), shown, t.dtype, tuple(t.shape)))


def _doses(sample_y, x_values):
    """(sample_y, x_values, n_doses) of an entry point with an effect pass, marshalled for ctypes"""
    return int(bool(sample_y)), _ptr(x_values), 0 if x_values is None else int(x_values.numel())


# The parameters every segment of the HMC sampler takes -- CausalEngine.hmc_run and the per-row family hmc_run_rows_* --, with their
# defaults and in the order of the C ABI's common prefix (CausalEngine._hmc_args), written once.
_P = inspect.Parameter
SEGMENT_PARAMS = ([_P(name, _P.POSITIONAL_OR_KEYWORD) for name in ("x", "y", "v", "state", "logp", "grad", "step", "it_begin", "n_iters",
                                                                   "burn_in", "n_leapfrog", "seed")] +
                  [_P(name, _P.POSITIONAL_OR_KEYWORD, default=default) for name, default in
                   (("init", False), ("row_base", 0), ("up", None), ("dn", None), ("s_min", RA.S_MIN), ("s_max", RA.S_MAX), ("acc_count", None),
                    ("draws", None), ("n_keep", 0))])


def _segment_method(fn):
    """fn(self, seg, <the method's own parameters, with defaults>) -> the public method (self, <SEGMENT_PARAMS>, <its own>,
    partial=False), under fn's name and docstring and with that signature for inspect.  A call is bound against it, so a caller's
    mistake (an unknown keyword, a missing argument) is the TypeError of a written-out parameter list; fn receives the bound
    arguments as the dict `seg` (defaults applied) and its own ones again by keyword."""
    own = list(inspect.signature(fn).parameters.values())[2:]
    sig = inspect.Signature([_P("self", _P.POSITIONAL_OR_KEYWORD)] + SEGMENT_PARAMS + own + [_P("partial", _P.POSITIONAL_OR_KEYWORD, default=False)])

    @functools.wraps(fn)
    def method(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        seg = bound.arguments
        return fn(seg["self"], seg, **{p.name: seg[p.name] for p in own})
    method.__signature__ = sig
    return method


_RowRoute = collections.namedtuple("_RowRoute", "method buffers finish")      # CausalEngine._row_routes


class CausalEngine(object):
    """Device-side state of one CausalBGM model: packed weights + kernels."""

    def __init__(self, v_dim, z_dims, binary_treatment=False, g_units=None, f_units=None, h_units=None,
                 e_units=None, sigma_v=None, sigma_x=None, sigma_y=None, device=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("bayesgm_amd: no HIP device visible; the hot path has no CPU fallback")
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        torch.cuda.init()
        torch.zeros(1, device=self.device)  # make sure the HIP context of this device exists
        self.v_dim = int(v_dim)
        self.z_dims = [int(z) for z in z_dims]
        self.q = sum(self.z_dims)
        self.binary = bool(binary_treatment)
        cfg = _lib.CausalConfig()
        cfg.v_dim = self.v_dim
        for i in range(4):
            cfg.z_dims[i] = self.z_dims[i]
        cfg.binary_treatment = int(self.binary)
        for name, units, default in (("g", g_units, DEFAULT_G_UNITS), ("f", f_units, DEFAULT_FH_UNITS),
                                     ("h", h_units, DEFAULT_FH_UNITS), ("e", e_units, DEFAULT_G_UNITS)):
            units = list(default if units is None else units)
            if len(units) > _lib.BGM_MAX_LAYERS:
                raise ValueError("%s_units: at most %d hidden layers" % (name, _lib.BGM_MAX_LAYERS))
            setattr(cfg, "n_hidden_" + name, len(units))
            arr = getattr(cfg, name + "_units")
            for i, u in enumerate(units):
                arr[i] = int(u)
        cfg.sigma_v = float(sigma_v) if sigma_v is not None else -1.0
        cfg.sigma_x = float(sigma_x) if sigma_x is not None else -1.0
        cfg.sigma_y = float(sigma_y) if sigma_y is not None else -1.0
        self.cfg = cfg
        self.h = C.c_void_p()
        _lib.check(self.lib.bgm_create(C.byref(self.h), self.device.index), "bgm_create")
        _lib.check(self.lib.bgm_causal_configure(self.h, C.byref(cfg)), "bgm_causal_configure")

    def set_precision(self, mode):
        """Arithmetic of logpost / mh_run launched afterwards: "fp32" (default) | "bf16x3" | "f16x3" (bgm_causal_set_precision)."""
        _lib.check(self.lib.bgm_causal_set_precision(self.h, {"fp32": 0, "bf16x3": 1, "f16x3": 2}[mode]), "bgm_causal_set_precision")

    def set_disc_norm(self, mode):
        """BatchNormalization mode of the EGM discriminators opened afterwards: "batch" | "fixed" (bgm_set_disc_norm)."""
        _lib.check(self.lib.bgm_set_disc_norm(self.h, {"batch": 0, "fixed": 1}[mode]), "bgm_set_disc_norm")

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.bgm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- weights ---------------------------------------------------------
    def set_weights(self, net_id, net):
        theta = flatten_net(net) if not isinstance(net, np.ndarray) else np.ascontiguousarray(net, np.float32)
        _lib.check(self.lib.bgm_causal_set_weights(self.h, net_id, theta.ctypes.data_as(C.c_void_p),
                                                   theta.size, self._stream()), "bgm_causal_set_weights")
        if not hasattr(self, "_w_count"):
            self._w_count = {}
        self._w_count[int(net_id)] = int(theta.size)

    def set_model(self, g=None, f=None, h=None, e=None):
        for nid, net in ((_lib.NET_G, g), (_lib.NET_F, f), (_lib.NET_H, h), (_lib.NET_E, e)):
            if net is not None:
                self.set_weights(nid, net)

    # -- kernels ---------------------------------------------------------
    def logpost(self, x, y, v, z):
        """get_log_posterior (causalbgm/base.py:765-817) -> torch [n] on device."""
        x, y, v, z = (_f32(t, self.device) for t in (x, y, v, z))
        n = v.shape[0]
        out = torch.empty(n, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.bgm_causal_logpost(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(z), n, _ptr(out),
                                               self._stream()), "bgm_causal_logpost")
        return out

    @contextlib.contextmanager
    def _partial_rows(self, partial, x, y):
        """partial=True of the gradient / HMC calls: NaN in x / y means "not observed" for the calls made inside (the handle flag
        bgm_causal_hmc_set_partial, cleared on the way out).  A row with y observed and x not is refused first (causal_hmc.py)."""
        if not partial:
            yield
            return
        HM.check_partial_rows(x, y)
        _lib.check(self.lib.bgm_causal_hmc_set_partial(self.h, 1), "bgm_causal_hmc_set_partial")
        try:
            yield
        finally:
            _lib.check(self.lib.bgm_causal_hmc_set_partial(self.h, 0), "bgm_causal_hmc_set_partial")

    def logpost_grad(self, x, y, v, z, partial=False):
        """get_log_posterior and its gradient with respect to z -> (logp [n], grad [n, q]) on the device (bgm_causal_logpost_grad:
        g's Gaussian term in the Gram form on every shape; fp32 LDS-resident shapes with the standard-normal prior).
        partial=True: NaN in y, or in x and y, marks what a row does not observe; its target is p(z | x, v) or p(z | v)."""
        x, y, v, z = (_f32(t, self.device) for t in (x, y, v, z))
        n = v.shape[0]
        out = torch.empty(n, device=self.device, dtype=torch.float32)
        grad = torch.empty((n, self.q), device=self.device, dtype=torch.float32)
        with self._partial_rows(partial, x, y):
            _lib.check(self.lib.bgm_causal_logpost_grad(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(z), n, _ptr(out), _ptr(grad),
                                                        self._stream()), "bgm_causal_logpost_grad")
        return out, grad

    @_segment_method
    def hmc_run(self, seg, effect=_lib.EFFECT_NONE, sample_y=True, x_values=None, adrf_partial=None, ite=None, labels=None, n_labels=0,
                group_partial=None):
        """One segment of the HMC latent sampler for all rows (bgm_causal_hmc_run); state / logp / grad / step are in / out.
        effect = EFFECT_ADRF / EFFECT_ITE: the segment runs the kernels with the effect pass inside (bgm_causal_hmc_run_effects):
        x_values [n_doses] and adrf_partial [n_slots, n_keep, n_doses] (+=), or ite [n, n_keep], receive the effects of the
        iterations >= burn_in of this segment.  effect = EFFECT_GROUP_ITE: hmc_run_group_effects with labels / n_labels /
        group_partial.  partial=True: NaN in y, or in x and y, marks what a row does not observe (logpost_grad); EFFECT_ADRF and
        EFFECT_GROUP_ITE have no kernels for it and raise the library's error."""
        if effect == _lib.EFFECT_NONE:
            self._hmc_segment("bgm_causal_hmc_run", seg)
        elif effect == _lib.EFFECT_GROUP_ITE:
            self._hmc_segment("bgm_causal_hmc_run_group_effects", seg, int(bool(sample_y)), _ptr(labels), int(n_labels), _ptr(group_partial))
        elif effect == (_lib.EFFECT_ITE if self.binary else _lib.EFFECT_ADRF):
            self._hmc_segment("bgm_causal_hmc_run_effects", seg, *_doses(sample_y, x_values), _ptr(adrf_partial), _ptr(ite))
        else:
            raise ValueError("hmc_run: effect must be EFFECT_NONE or the effect of the treatment type (EFFECT_ITE for a binary "
                             "treatment, EFFECT_ADRF otherwise); got %r" % (effect,))

    def _hmc_args(self, x, y, v, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, init, row_base, up, dn, s_min, s_max,
                  acc_count, draws, n_keep):
        """The handle and the 24 arguments that every entry point of an HMC segment takes first (include/bgm_hip.h; the parameters
        of SEGMENT_PARAMS in their order), marshalled for ctypes; the entry point's own arguments and the stream follow them."""
        return (self.h, _ptr(x), _ptr(y), _ptr(v), v.shape[0], int(row_base), _ptr(state), _ptr(logp), _ptr(grad), _ptr(step), _ptr(up),
                _ptr(dn), 0 if up is None else int(up.numel()), float(s_min), float(s_max), int(bool(init)), int(it_begin), int(n_iters),
                int(burn_in), int(n_leapfrog), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(acc_count), _ptr(draws), int(n_keep))

    def _hmc_segment(self, entry, seg, *own):
        """One segment through the C entry point `entry`: inside the observation pattern of seg["partial"], the common arguments of
        seg (a segment method's bound arguments), the entry point's `own`, the stream; the library's error raises."""
        with self._partial_rows(seg["partial"], seg["x"], seg["y"]):
            _lib.check(getattr(self.lib, entry)(*self._hmc_args(*(seg[p.name] for p in SEGMENT_PARAMS)), *own, self._stream()), entry)

    @_segment_method
    def hmc_run_rows_effects(self, seg, sample_y=True, x_values=None, row_moments=None, row_draws=None):
        """hmc_run with the dose-response of every row kept (bgm_causal_hmc_run_row_effects; a continuous treatment): x_values
        [n_doses]; row_moments [3, n_doses, n] float32 (ref = y at retained draw 0, s1 = sum of y - ref, s2 = sum of (y - ref)^2,
        in / out across segments) and, optionally, row_draws [n, n_doses, n_keep] receive y_i(x_k) of the iterations >= burn_in of
        this segment.  partial=True: as in hmc_run."""
        self._hmc_segment("bgm_causal_hmc_run_row_effects", seg, *_doses(sample_y, x_values), _ptr(row_moments), _ptr(row_draws))

    @_segment_method
    def hmc_run_rows_tails(self, seg, sample_y=True, x_values=None, row_moments=None, row_draws=None, row_tails=None):
        """hmc_run_rows_effects with the two tails of every (row, dose) series kept beside its moments
        (bgm_causal_hmc_run_row_tails): row_tails [2, K, n_doses, n] float32, in / out across segments, tail 0 the K smallest and
        tail 1 the K largest of the retained y_i(x_k), each a heap in no sorted order (row_tail_quantiles reads them); 1 <= K <=
        n_keep.  Chain, moments and row_draws are those of hmc_run_rows_effects bit for bit."""
        doses, n = _doses(sample_y, x_values), seg["v"].shape[0]
        _check_buffer("hmc_run_rows_tails", "row_tails", row_tails, torch.float32, (2, None, None, None), "[2, K, n_doses, n]")
        if row_tails is not None and tuple(row_tails.shape[2:]) != (doses[2], n):      # (its own words: the sizes, and the shape alone)
            raise ValueError("hmc_run_rows_tails: row_tails must be [2, K, n_doses, n] = [2, K, %d, %d]; got %r" %
                             (doses[2], n, tuple(row_tails.shape)))
        self._hmc_segment("bgm_causal_hmc_run_row_tails", seg, *doses, _ptr(row_moments), _ptr(row_draws), _ptr(row_tails),
                          0 if row_tails is None else int(row_tails.shape[1]))

    @_segment_method
    def hmc_run_rows_contrasts(self, seg, sample_y=True, x_values=None, row_moments=None, row_cmoments=None, contrast_draws=None,
                               contrast_tails=None):
        """hmc_run_rows_effects with the contrast of every dose against the baseline x_values[0] kept beside the curve
        (bgm_causal_hmc_run_row_contrasts): c_i(k) = y_i(x_k) - y_i(x_0) of every retained draw, one float32 subtraction inside the
        kernel.  row_cmoments [3, n_doses, n] float32 receives its shifted sums (the rule of row_moments, in / out across
        segments); optionally contrast_draws [n, n_doses, n_keep] the differences themselves and contrast_tails [2, K, n_doses, n]
        their K smallest and K largest (hmc_run_rows_tails' layout, 1 <= K <= n_keep).  Chain and row_moments are those of
        hmc_run_rows_effects bit for bit.  The library refuses the call while a trajectory option is set."""
        doses, n = _doses(sample_y, x_values), seg["v"].shape[0]
        _check_buffer("hmc_run_rows_contrasts", "contrast_tails", contrast_tails, torch.float32, (2, None, doses[2], n),
                      "[2, K, n_doses, n] = [2, K, %d, %d]" % (doses[2], n))
        self._hmc_segment("bgm_causal_hmc_run_row_contrasts", seg, *doses, _ptr(row_moments), _ptr(row_cmoments), _ptr(contrast_draws),
                          _ptr(contrast_tails), 0 if contrast_tails is None else int(contrast_tails.shape[1]))

    @_segment_method
    def hmc_run_rows_choice(self, seg, sample_y=True, x_values=None, row_moments=None, row_draws=None, best_count=None, best_moments=None,
                            above_count=None, threshold=0.0, maximize=True):
        """hmc_run_rows_effects with the choice among the doses kept beside the curve (bgm_causal_hmc_run_row_choice): best_count
        [n_doses, n] int32 counts the retained draws at which dose k gave the row its best outcome (the largest y with maximize,
        else the smallest; the lowest dose index on ties), best_moments [2, n] float32 holds ref = the best y of retained draw 0
        and s1 = the sum of best - ref, and, optionally, above_count [n_doses, n] int32 counts the draws with y > threshold (a
        finite number).  All are written by the first retained iteration and in / out across segments.  Chain, row_moments and
        row_draws are those of hmc_run_rows_effects bit for bit.  The library refuses the call while a trajectory option is set."""
        doses, n = _doses(sample_y, x_values), seg["v"].shape[0]
        for name, t, shape, dt in (("best_count", best_count, (doses[2], n), torch.int32), ("best_moments", best_moments, (2, n), torch.float32),
                                   ("above_count", above_count, (doses[2], n), torch.int32)):
            _check_buffer("hmc_run_rows_choice", name, t, dt, shape, repr(shape))
        self._hmc_segment("bgm_causal_hmc_run_row_choice", seg, *doses, _ptr(row_moments), _ptr(row_draws), _ptr(best_count),
                          _ptr(best_moments), _ptr(above_count), float(threshold), int(bool(maximize)))

    def row_tail_quantiles(self, tails, m, q_lo, q_hi):
        """tails [2, K, ...] float32 on the device (hmc_sample's out["tails"]: the K smallest and the K largest of every series' m
        values) -> (lo, hi), each of shape tails.shape[2:]: the quantiles row_mean_quantiles gives on the m values, bit for bit
        (bgm_row_tail_quantiles).  K below what (m, q_lo, q_hi) need (causal_hmc.tail_size) raises the library's error."""
        return _row_tail_quantiles(self, tails, m, q_lo, q_hi)

    def hmc_run_group_effects(self, x, y, v, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, labels=None, n_labels=0,
                              group_partial=None, **kw):
        """hmc_run with the individual treatment effect of a binary treatment summed by row label inside the sampler
        (bgm_causal_hmc_run_group_effects): labels [n] int32 on the device, every label in [0, n_labels) -- the caller's duty, the
        kernel does not report a label outside --, group_partial [n_slots, n_keep, n_labels] float32 (+=, n_slots =
        bgm_causal_evaluate_slots) receives the sums of the iterations >= burn_in of this segment.  The other arguments are
        hmc_run's."""
        self.hmc_run(x, y, v, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, effect=_lib.EFFECT_GROUP_ITE,
                     labels=labels, n_labels=n_labels, group_partial=group_partial, **kw)

    def _group_labels(self, labels, n_labels, n, who):
        """labels [n] (NumPy or tensor, integer) with every label in [0, n_labels), checked on the host -> int32 tensor on the device"""
        n_labels = int(n_labels) if n_labels is not None else 0
        if not 1 <= n_labels <= _lib.MAX_GROUP_LABELS:
            raise ValueError("%s: n_labels must be in [1, %d]; got %r" % (who, _lib.MAX_GROUP_LABELS, n_labels))
        host = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if labels is None or host.shape != (n,) or not np.issubdtype(host.dtype, np.integer):
            raise ValueError("%s: labels must be integers of shape [n] = (%d,); got %s of shape %r" % (who, n, host.dtype, host.shape))
        if n and (int(host.min()) < 0 or int(host.max()) >= n_labels):
            raise ValueError("%s: labels must lie in [0, n_labels) = [0, %d); got %d .. %d" % (who, n_labels, int(host.min()), int(host.max())))
        return torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(self.device), n_labels

    def ite_group_sums(self, ite, labels, n_labels):
        """ite [n, n_keep] float32 on the device, labels [n] in [0, n_labels) -> float64 [n_labels, n_keep]: the sums of ite over the
        rows of every label (bgm_ite_group_sums; rows in ascending order, one owner per element, bit-identical from call to call)."""
        ite = _f32(ite, self.device)
        n, n_keep = ite.shape
        lab, n_labels = self._group_labels(labels, n_labels, n, "ite_group_sums")
        out = torch.zeros((n_labels, n_keep), device=self.device, dtype=torch.float64)
        if n and n_keep:
            _lib.check(self.lib.bgm_ite_group_sums(self.h, _ptr(ite), _ptr(lab), n, n_keep, n_labels, _ptr(out), self._stream()),
                       "bgm_ite_group_sums")
        return out

    def set_hmc_mass(self, scale=None, ref=None, s1=None, s2=None, accumulate=False):
        """Diagonal metric of the hmc_run calls made afterwards (bgm_causal_hmc_set_mass): scale float32 [n x q] (device), the
        per-coordinate factors of every chain's step, aligned with the rows of the call.  accumulate: those calls also add
        z - ref and its square into s1 / s2 [n x q] after every decision (the moments hmc_mass_update turns into scales).
        scale = None: back to identity mass."""
        self._hmc_mass_keep = (scale, ref, s1, s2)          # keep the buffers alive while set
        _lib.check(self.lib.bgm_causal_hmc_set_mass(self.h, _ptr(scale), _ptr(ref), _ptr(s1), _ptr(s2), int(bool(accumulate))),
                   "bgm_causal_hmc_set_mass")

    def set_hmc_trajectory(self, max_trajectory=None, jitter=False, n_steps=None):
        """The number of leapfrog steps per chain and iteration of the hmc_run calls made afterwards (bgm_causal_hmc_set_trajectory;
        causal_hmc.resolve_trajectory): with max_trajectory = T a chain whose step is eps takes row_adapt.leapfrog_cap(eps,
        n_leapfrog, T) steps, with jitter a number uniform on 1 .. that cap drawn per chain and iteration.  n_steps: int32 [n]
        (device), aligned with the rows of the call, += the steps of every iteration >= burn_in.  All three off (the default):
        back to the kernels without the option.  hmc_run_rows_tails and EFFECT_GROUP_ITE raise the library's error while set."""
        T, jit = HM.resolve_trajectory(max_trajectory, jitter)
        _check_buffer("set_hmc_trajectory", "n_steps", n_steps, torch.int32, (None,), "[n]")
        self._hmc_traj_keep = n_steps                       # keep the buffer alive while set
        _lib.check(self.lib.bgm_causal_hmc_set_trajectory(self.h, float(T), int(jit), _ptr(n_steps)), "bgm_causal_hmc_set_trajectory")

    def hmc_mass_update(self, n_draws, state, scale, ref, s1, s2):
        """End of an estimation window of n_draws iterations (bgm_causal_hmc_mass_update): scale from the moments (causal_hmc.py,
        mass_update), then ref = state and s1 = s2 = 0.  n_draws = 0 only resets."""
        _lib.check(self.lib.bgm_causal_hmc_mass_update(self.h, state.shape[0], int(n_draws), _ptr(state), _ptr(scale), _ptr(ref), _ptr(s1),
                                                       _ptr(s2), self._stream()), "bgm_causal_hmc_mass_update")

    def hmc_sample(self, x, y, v, burn_in, n_keep, step_size, n_leapfrog, seed, chunk=None, want_draws=False, row_base=0,
                   adapt=HM.DEFAULT_TARGET, adapt_table=None, mass=None, mass_windows=None, mass_scale=None, effect=_lib.EFFECT_NONE,
                   x_values=None, sample_y=True, row_effects=False, row_draws=False, labels=None, n_labels=None, partial=False,
                   row_tails=None, max_trajectory=None, jitter=False, row_contrasts=False, row_choice=False, maximize=True, threshold=None):
        """HMC over the latent posterior of every row, one chain per row with a step size of its own.

        adapt = target acceptance rate (None: the step stays step_size): after each of the burn_in decisions a chain multiplies its
        step by the factor of row_adapt.row_adapt_factors(burn_in, adapt) for "moved" / "did not" and clamps it; the retained chain
        is plain HMC.  adapt_table = (up, dn) replaces that schedule.  One launch per chunk of iterations (None: one launch).

        mass = 'diag': every chain estimates a scale per coordinate from its own burn-in draws in the windows of
        causal_hmc.mass_windows(burn_in) (mass_windows = (start, ends) replaces them) and keeps it afterwards; the step table is
        causal_hmc.mass_schedule's.  mass_scale = tensor [n x q]: that metric, frozen, no estimation.  Windows are launch
        boundaries; cuts by chunk inside them change nothing.

        effect = EFFECT_ADRF (with x_values) / EFFECT_ITE: infer_from_latent_posterior runs inside the sampler on every retained
        state (hmc_run), no draws are needed; every launch, burn-in included, is the fused kernel, so a model it refuses (LDS) is
        refused before any state is written.  The result is engine.effects on the draws of the same run, bit for bit.

        effect = EFFECT_GROUP_ITE (a binary treatment, with labels [n] in [0, n_labels), n_labels <= 64): the ITE of every retained
        state is summed by row label inside the sampler (hmc_run_group_effects) and no ITE matrix is stored: group_sums
        [n_labels, n_keep] float32, the sum over each label's rows per draw (group_partial [n_slots, n_keep, n_labels], the wave
        slots' sums it is reduced from, is returned too).  A row's value is that of EFFECT_ITE bit for bit; the sums depend on the
        grid through the slots, not on chunk.

        row_effects = True (a continuous treatment, with x_values, instead of an effect): the dose-response of every row,
        y_i(x_k) of every retained state, is summarised inside the sampler (hmc_run_rows_effects) into row_mean / row_sd
        [n, n_doses] (float64, causal_hmc.row_moments_finalize) without stored draws; row_draws = True also returns them,
        row_draws [n, n_doses, n_keep].  The chain is that of the run without effects, and a row's result depends on (seed,
        row_base + row, the row's data) alone.  row_tails = K (with row_effects, 1 <= K <= n_keep): the K smallest and the K
        largest values of every (row, dose) series are kept as well (hmc_run_rows_tails) and returned as tails [2, K, n_doses, n],
        from which row_tail_quantiles gives the exact quantile bounds (K = causal_hmc.tail_size(alpha, n_keep)); chain, moments
        and row_draws are those of the run without it.

        row_contrasts = True (with row_effects): x_values[0] is a baseline dose, and the contrast c_i(k) = y_i(x_k) - y_i(x_0) of
        every retained state is summarised inside the sampler as well (hmc_run_rows_contrasts) into contrast_mean / contrast_sd
        [n, n_doses] (float64; column 0 is exactly 0); row_mean / row_sd and the chain are those of the run without it.  The
        optional buffers then hold the contrasts, not the values: row_draws = True returns contrast_draws [n, n_doses, n_keep] (the
        float32 difference of the columns k and 0 of the row_draws of a run without row_contrasts) and row_tails = K their tails.
        With sample_y the two doses carry independent noise.  Not available for a binary treatment (it has EFFECT_ITE) or with
        max_trajectory / jitter: ValueError before a device is touched.

        row_choice = True (with row_effects): the doses are compared on every retained state inside the sampler
        (hmc_run_rows_choice): best_count [n, n_doses] (int64) is the number of retained draws at which dose k gave the row its best
        outcome -- the largest with maximize, else the smallest, the lowest dose index on ties; rows sum to n_keep --, best_mean [n]
        (float64) the posterior mean of that best outcome, and, with threshold = a finite number, above_count [n, n_doses] (int64)
        the draws with y > threshold.  Chain, row_mean / row_sd and row_draws are those of the run without it.  With sample_y every
        dose carries its own independent noise.  Not available with row_contrasts, row_tails, max_trajectory / jitter or a binary
        treatment, nor with a metric (mass / mass_scale) together with partial at more than 11 latent features (that one kernel is
        not built: causal_hmc.check_choice_kernel): ValueError before a device is touched.

        partial = True: NaN in y, or in x and y, marks what a row does not observe (new units): its chain samples p(z | x, v) or
        p(z | v) (logpost_grad).  A row with y observed and x not is refused.  Works without an effect, with EFFECT_ITE and with
        row_effects; a fully observed panel gives the run of partial = False bit for bit.

        max_trajectory = T / jitter = True (set_hmc_trajectory, for this run): a chain takes as many of the n_leapfrog steps as
        keep step x steps below T (at least one), and with jitter a number uniform on 1 .. that many, drawn per chain and
        iteration; a wave's loop ends at the largest count of its 16 rows.  row_leapfrog [n] (float32) is the mean number of steps
        per retained transition.  With every option off the run is the one without them, bit for bit.  row_tails and
        EFFECT_GROUP_ITE have no such kernels: ValueError before anything is launched.
        Returns dict(draws [n_keep, n, q] | None, state, logp, grad, acc_count [burn_in + n_keep], row_step [n]) and, with a metric,
        mass_scale [n x q]; with an effect, adrf [n_doses, n_keep], ite [n, n_keep] or group_sums [n_labels, n_keep]; with a
        trajectory option, n_steps [n] (int32, the steps of the retained transitions) and row_leapfrog [n] = n_steps / n_keep."""
        HM.check_args(step_size, n_leapfrog, adapt)
        traj_T, traj_jit = HM.resolve_trajectory(max_trajectory, jitter)
        traj = traj_T > 0.0 or traj_jit != 0
        kind = HM.result_kind(effect, row_effects, row_tails, row_contrasts, row_choice)
        HM.check_result(kind, lambda: self.binary, traj, row_draws, row_tails, row_contrasts)
        if row_choice:
            threshold = HM.check_threshold(threshold)
            if kind.hole is not None:
                HM.check_choice_kernel(self.q, mass not in (None, "identity") or mass_scale is not None, partial)
        elif threshold is not None:
            raise ValueError("hmc_sample: threshold belongs to row_choice=True")
        diag = HM.check_mass(mass, True, adapt if adapt_table is None else True) is not None
        if diag and mass_scale is not None:
            raise ValueError("hmc_sample: mass='diag' estimates the metric; mass_scale gives a frozen one")
        start, ends = None, []
        if diag:
            (start, ends), table = HM.mass_schedule(burn_in, float(adapt) if adapt is not None else HM.DEFAULT_TARGET, mass_windows)
            adapt_table = table if adapt_table is None else adapt_table
        dev = self.device
        x, y, v = (_f32(t, dev) for t in (x, y, v))
        x, y = x.reshape(-1), y.reshape(-1)
        n, total = v.shape[0], int(burn_in) + int(n_keep)
        up = dn = None
        if adapt_table is not None or adapt is not None:
            up, dn = adapt_table if adapt_table is not None else RA.row_adapt_factors(burn_in, float(adapt))
            up, dn = (_f32(np.asarray(t, dtype=np.float32).reshape(-1), dev) for t in (up, dn))
            if up.numel() != dn.numel():
                raise ValueError("hmc_sample: adapt_table = (up, dn) of equal length")
            if up.numel() == 0:
                up = dn = None
        state = torch.empty((n, self.q), device=dev, dtype=torch.float32)
        logp = torch.empty(n, device=dev, dtype=torch.float32)
        grad = torch.empty((n, self.q), device=dev, dtype=torch.float32)
        step = torch.full((n,), float(np.float32(step_size)), device=dev, dtype=torch.float32)
        acc = torch.zeros(total, device=dev, dtype=torch.int32)
        draws = torch.empty((n_keep, n, self.q), device=dev, dtype=torch.float32) if want_draws else None
        chunk = total if chunk is None else max(1, int(chunk))
        launch, route_kw, collect = self._hmc_route(kind, n, n_keep, x_values, labels, n_labels, row_draws, row_tails,
                                                    (bool(maximize), threshold) if row_choice else None)
        scale = moments = None
        if diag:
            scale = torch.ones((n, self.q), device=dev, dtype=torch.float32)
            moments = [torch.zeros((n, self.q), device=dev, dtype=torch.float32) for _ in range(3)]      # ref, s1, s2
        elif mass_scale is not None:
            scale = _f32(mass_scale, dev).clone()
            if tuple(scale.shape) != (n, self.q):
                raise ValueError("hmc_sample: mass_scale must be [n x q] = %r; got %r" % ((n, self.q), tuple(scale.shape)))
        marks = [start] + ends if diag else []
        n_steps = torch.zeros(n, device=dev, dtype=torch.int32) if traj else None
        with self._partial_rows(partial, x, y):      # the pattern is checked and the handle's flag set once, not per segment
            try:
                if scale is not None:
                    self.set_hmc_mass(scale)
                if traj:
                    self.set_hmc_trajectory(max_trajectory, jitter, n_steps)
                it = 0
                while it < total:
                    stop = min([it + chunk, total] + [b for b in marks if b > it])
                    launch(x, y, v, state, logp, grad, step, it, stop - it, burn_in, n_leapfrog, seed, init=(it == 0), row_base=row_base,
                           up=up, dn=dn, acc_count=acc, draws=draws, n_keep=n_keep, sample_y=sample_y, **route_kw)
                    if stop in marks:      # a window's edge: the first one only sets the reference point and turns the moments on
                        k = marks.index(stop)
                        self.hmc_mass_update(0 if k == 0 else stop - marks[k - 1], state, scale, *moments)
                        self.set_hmc_mass(scale, *moments, accumulate=(k < len(marks) - 1))
                    it = stop
            finally:
                if scale is not None:
                    self.set_hmc_mass(None)
                if traj:
                    self.set_hmc_trajectory(None)
        out = dict(draws=draws, state=state, logp=logp, grad=grad, acc_count=acc, row_step=step)
        if scale is not None:
            out["mass_scale"] = scale
        if traj:
            out["n_steps"], out["row_leapfrog"] = n_steps, n_steps.float() / float(max(1, int(n_keep)))
        collect(out)
        return out

    # The result routes of hmc_sample, one per kind of result (causal_hmc.RESULT_KINDS; which kind the options ask for and what does
    # not exist with it was decided there, before a device was touched).  Each checks what is its own, allocates its buffers and
    # returns (launch, kw, collect): the engine method that runs a segment, the keyword arguments it takes besides the common ones,
    # and the function that adds the route's keys to the returned dict.
    def _hmc_route(self, kind, n, n_keep, x_values, labels, n_labels, row_draws, row_tails=None, row_choice=None):
        if labels is not None and (kind is None or kind.name != "group_ite"):
            raise ValueError("hmc_sample: labels belong to effect=EFFECT_GROUP_ITE")
        if kind is not None and kind.request.get("row_effects"):
            return self._route_rows(kind, n, n_keep, x_values, row_draws, row_tails, row_choice)
        route = {None: self._route_none, "adrf": self._route_adrf, "ite": self._route_ite, "group_ite": self._route_group_ite}
        return route[kind and kind.name](n, n_keep, x_values, labels, n_labels)

    def _evaluate_slots(self, n):
        ns = C.c_int32()
        _lib.check(self.lib.bgm_causal_evaluate_slots(self.h, n, C.byref(ns)), "bgm_causal_evaluate_slots")
        return ns.value

    def _route_none(self, n, n_keep, x_values, labels, n_labels):
        return self.hmc_run, {}, lambda out: None

    def _route_adrf(self, n, n_keep, x_values, labels, n_labels):
        if x_values is None:
            raise ValueError("hmc_sample: effect=EFFECT_ADRF needs x_values")
        xv = _f32(np.atleast_1d(np.asarray(x_values, dtype=np.float32)), self.device)
        n_slots = self._evaluate_slots(n)
        part = torch.zeros((n_slots, n_keep, xv.numel()), device=self.device, dtype=torch.float32)
        return (self.hmc_run, dict(effect=_lib.EFFECT_ADRF, x_values=xv, adrf_partial=part),
                lambda out: out.update(adrf=self.adrf_reduce(part, n_slots, xv.numel(), n_keep, n)))

    def _route_ite(self, n, n_keep, x_values, labels, n_labels):
        ite = torch.empty((n, n_keep), device=self.device, dtype=torch.float32)
        return self.hmc_run, dict(effect=_lib.EFFECT_ITE, ite=ite), lambda out: out.update(ite=ite)

    def _route_group_ite(self, n, n_keep, x_values, labels, n_labels):
        lab, n_lab = self._group_labels(labels, n_labels, n, "hmc_sample")
        n_slots = self._evaluate_slots(n)
        try:
            part = torch.zeros((n_slots, n_keep, n_lab), device=self.device, dtype=torch.float32)
        except torch.cuda.OutOfMemoryError:
            raise RuntimeError("hmc_sample: cannot allocate group_partial [n_slots x n_keep x n_labels] = [%d x %d x %d] float32 (%d "
                               "bytes)" % (n_slots, n_keep, n_lab, 4 * n_slots * n_keep * n_lab))
        return (self.hmc_run, dict(effect=_lib.EFFECT_GROUP_ITE, labels=lab, n_labels=n_lab, group_partial=part),
                lambda out: out.update(group_partial=part, group_sums=self.adrf_reduce(part, n_slots, n_lab, n_keep, 1.0)))

    def _row_routes(self):
        """The per-row kinds (causal_hmc.RESULT_KINDS): the engine method of a segment, the buffers the kind allocates beside
        row_moments -- (keyword of that method, shape over n_doses d, n, n_keep k and the tail size K, dtype, zeroed, asked for by)
        -- and what it adds to the result beside row_mean / row_sd.  The stored series and the tails are those of the values or,
        for the contrasts, of the contrasts: the same buffers under the kind's own keywords and result key.  A buffer that is not
        zeroed is written whole by the first retained iteration."""
        f32, i32 = torch.float32, torch.int32
        draws, tails = ("row_draws", "ndk", f32, False, "draws"), ("row_tails", "2Kdn", f32, False, "tails")
        return {"rows": _RowRoute(self.hmc_run_rows_effects, (draws,), self._finish_rows),
                "tails": _RowRoute(self.hmc_run_rows_tails, (draws, tails), self._finish_rows),
                "contrasts": _RowRoute(self.hmc_run_rows_contrasts, (("row_cmoments", "3dn", f32, True, None),
                                                                     ("contrast_draws",) + draws[1:], ("contrast_tails",) + tails[1:]),
                                       self._finish_contrasts),
                "choice": _RowRoute(self.hmc_run_rows_choice, (draws, ("best_count", "dn", i32, True, None), ("best_moments", "2n", f32, True, None),
                                                               ("above_count", "dn", i32, True, "threshold")), self._finish_choice)}

    def _route_rows(self, kind, n, n_keep, x_values, row_draws, row_tails=None, row_choice=None):
        if self.binary:
            raise ValueError(kind.wrong_treatment)
        if x_values is None:
            raise ValueError("hmc_sample: row_effects needs x_values")
        if row_tails is not None and (isinstance(row_tails, bool) or int(row_tails) != row_tails or not 1 <= int(row_tails) <= int(n_keep)):
            raise ValueError("hmc_sample: row_tails must be an integer K with 1 <= K <= n_keep = %d; got %r" % (int(n_keep), row_tails))
        xv = _f32(np.atleast_1d(np.asarray(x_values, dtype=np.float32)), self.device)
        size = {"n": n, "d": xv.numel(), "k": n_keep, "K": row_tails and int(row_tails), "2": 2, "3": 3}
        asked = dict(draws=bool(row_draws), tails=row_tails is not None, threshold=row_choice is not None and row_choice[1] is not None)
        route = self._row_routes()[kind.name]
        kw = dict(x_values=xv, row_moments=torch.zeros((3, xv.numel(), n), device=self.device, dtype=torch.float32))      # ref, s1, s2
        for name, shape, dtype, zeroed, when in route.buffers:
            make = torch.zeros if zeroed else torch.empty
            kw[name] = make(tuple(size[c] for c in shape), device=self.device, dtype=dtype) if when is None or asked[when] else None
        if row_choice is not None:
            kw.update(maximize=row_choice[0], threshold=0.0 if row_choice[1] is None else row_choice[1])

        def collect(out):
            out["row_mean"], out["row_sd"] = self._row_moments(kw["row_moments"], n_keep)
            route.finish(out, kw, n_keep)
        return route.method, kw, collect

    @staticmethod
    def _row_moments(mom, n_keep):
        mean, sd = HM.row_moments_finalize(mom[0], mom[1], mom[2], n_keep)
        return mean.t().contiguous(), sd.t().contiguous()

    @staticmethod
    def _finish_rows(out, kw, n_keep, draws="row_draws", tails="row_tails"):
        if kw[draws] is not None:
            out[draws] = kw[draws]
        if kw.get(tails) is not None:
            out["tails"] = kw[tails]

    def _finish_contrasts(self, out, kw, n_keep):
        out["contrast_mean"], out["contrast_sd"] = self._row_moments(kw["row_cmoments"], n_keep)
        self._finish_rows(out, kw, n_keep, "contrast_draws", "contrast_tails")

    def _finish_choice(self, out, kw, n_keep):
        self._finish_rows(out, kw, n_keep)
        bmom = kw["best_moments"]
        out["best_count"] = kw["best_count"].t().contiguous().long()
        out["best_ref"], out["best_s1"] = bmom[0], bmom[1]
        out["best_mean"] = bmom[0].double() + bmom[1].double() / float(max(1, int(n_keep)))
        if kw["above_count"] is not None:
            out["above_count"] = kw["above_count"].t().contiguous().long()

    def encode(self, v):
        v = _f32(v, self.device)
        n = v.shape[0]
        z = torch.empty((n, self.q), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.bgm_causal_encode(self.h, _ptr(v), n, _ptr(z), self._stream()), "bgm_causal_encode")
        return z

    def mh_slots(self, n):
        s = C.c_int32()
        _lib.check(self.lib.bgm_causal_mh_slots(self.h, n, C.byref(s)), "bgm_causal_mh_slots")
        return s.value

    def mh_info(self, n):
        info = _lib.MhInfo()
        _lib.check(self.lib.bgm_causal_mh_info(self.h, n, C.byref(info)), "bgm_causal_mh_info")
        return info

    def mh_run(self, x, y, v, state, logp, it_begin, n_iters, burn_in, q_sd, seed, init=False, row_base=0,
               acc_count=None, draws=None, n_keep=0, effect=_lib.EFFECT_NONE, sample_y=True, x_values=None,
               adrf_partial=None, ite=None, clock=None):
        """One segment of metropolis_hastings_sampler (causalbgm/base.py:860-898) for all rows."""
        a = _lib.MhArgs()
        a.x_dev, a.y_dev, a.v_dev = x.data_ptr(), y.data_ptr(), v.data_ptr()
        a.n = v.shape[0]
        a.row_base = int(row_base)
        a.state_dev, a.logp_dev = state.data_ptr(), logp.data_ptr()
        a.init = int(bool(init))
        a.it_begin, a.n_iters, a.burn_in = int(it_begin), int(n_iters), int(burn_in)
        a.q_sd = float(q_sd)
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        a.acc_count_dev = acc_count.data_ptr() if acc_count is not None else None
        a.draws_dev = draws.data_ptr() if draws is not None else None
        a.n_keep = int(n_keep)
        a.effect = int(effect)
        a.sample_y = int(bool(sample_y))
        a.x_values_dev = x_values.data_ptr() if x_values is not None else None
        a.n_doses = int(x_values.numel()) if x_values is not None else 0
        a.adrf_partial_dev = adrf_partial.data_ptr() if adrf_partial is not None else None
        a.ite_dev = ite.data_ptr() if ite is not None else None
        a.clock_dev = clock.data_ptr() if clock is not None else None
        _lib.check(self.lib.bgm_causal_mh_run(self.h, C.byref(a), self._stream()), "bgm_causal_mh_run")

    def adrf_reduce(self, partial, n_slots, n_doses, n_keep, n_total):
        out = torch.empty((n_doses, n_keep), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.bgm_adrf_reduce(self.h, _ptr(partial), n_slots, n_doses, n_keep, float(n_total),
                                            _ptr(out), self._stream()), "bgm_adrf_reduce")
        return out

    def row_mean_quantiles(self, mat, q_lo, q_hi):
        """mat [n_rows, m] on device -> (mean, lo, hi) each [n_rows]."""
        mat = mat.contiguous()
        n_rows, m = mat.shape
        mean = torch.empty(n_rows, device=self.device, dtype=torch.float32)
        lo = torch.empty_like(mean)
        hi = torch.empty_like(mean)
        _lib.check(self.lib.bgm_row_mean_quantiles(self.h, _ptr(mat), n_rows, m, float(q_lo), float(q_hi),
                                                   _ptr(mean), _ptr(lo), _ptr(hi), self._stream()),
                   "bgm_row_mean_quantiles")
        return mean, lo, hi

    # -- evaluate -----------------------------------------------------------------
    def evaluate(self, x, y, v, z, x_values=None):
        """CausalBGM.evaluate arithmetic (causalbgm/base.py:534-570) on device tensors.
        Returns (sums[3] float64 tensor, causal): causal = ITE [n] (binary) or dose sums [n_doses]."""
        n = v.shape[0]
        sums = torch.zeros(4, device=self.device, dtype=torch.float64)
        if self.binary:
            ite = torch.empty(n, device=self.device, dtype=torch.float32)
            _lib.check(self.lib.bgm_causal_evaluate(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(z), n, None, 0, _ptr(sums),
                                                    None, _ptr(ite), self._stream()), "bgm_causal_evaluate")
            return sums, ite
        xv = _f32(np.atleast_1d(np.asarray(x_values, dtype=np.float32)), self.device)
        n_slots = self._evaluate_slots(n)
        partial = torch.zeros((n_slots, xv.numel()), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.bgm_causal_evaluate(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(z), n, _ptr(xv), xv.numel(),
                                                _ptr(sums), _ptr(partial), None, self._stream()), "bgm_causal_evaluate")
        dose_sums = self.adrf_reduce(partial, n_slots, xv.numel(), 1, 1.0).reshape(-1)
        return sums, dose_sums

    def effects(self, x, draws, burn_in, seed, x_values=None, sample_y=True, row_base=0):
        """infer_from_latent_posterior (causalbgm/base.py:671-763) for draws [n_keep, n, q] on the device:
        binary -> ITE draws [n_keep, n]; continuous -> ADRF draws [n_doses, n_keep] (mean over the n rows)."""
        x = _f32(x, self.device).reshape(-1)
        draws = _f32(draws, self.device)
        n_keep, n, _ = draws.shape
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if self.binary:
            ite = torch.empty((n, n_keep), device=self.device, dtype=torch.float32)
            _lib.check(self.lib.bgm_causal_effects(self.h, _ptr(x), _ptr(draws), n, int(row_base), n_keep, int(burn_in), seed,
                                                   int(bool(sample_y)), None, 0, None, _ptr(ite), self._stream()), "bgm_causal_effects")
            return ite.t().contiguous()
        xv = _f32(np.atleast_1d(np.asarray(x_values, dtype=np.float32)), self.device)
        n_slots = self._evaluate_slots(n)
        partial = torch.zeros((n_slots, n_keep, xv.numel()), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.bgm_causal_effects(self.h, _ptr(x), _ptr(draws), n, int(row_base), n_keep, int(burn_in), seed,
                                               int(bool(sample_y)), _ptr(xv), xv.numel(), _ptr(partial), None, self._stream()),
                   "bgm_causal_effects")
        return self.adrf_reduce(partial, n_slots, xv.numel(), n_keep, n)

    # -- fit step functions ------------------------------------------------------
    def fit_begin(self, n_rows, max_batch):
        _lib.check(self.lib.bgm_causal_fit_begin(self.h, int(n_rows), int(max_batch), self._stream()),
                   "bgm_causal_fit_begin")
        n = C.c_int64()
        _lib.check(self.lib.bgm_causal_fit_n_params(self.h, C.byref(n)), "bgm_causal_fit_n_params")
        self.n_params = n.value
        return n.value

    def fit_theta_grad(self, x, y, v, data_z, idx, batch_global, grad, loss=None, row_lo=0, batch=None):
        b = int(idx.numel()) if idx is not None else int(batch)
        _lib.check(self.lib.bgm_causal_fit_theta_grad(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(data_z), _ptr(idx),
                                                      int(row_lo), b, int(batch_global), _ptr(grad), _ptr(loss),
                                                      self._stream()), "bgm_causal_fit_theta_grad")

    def fit_theta_apply(self, grad, lr_theta):
        _lib.check(self.lib.bgm_causal_fit_theta_apply(self.h, _ptr(grad), float(lr_theta), self._stream()),
                   "bgm_causal_fit_theta_apply")

    def fit_z_step(self, x, y, v, data_z, zm, zv, idx, batch_global, lr_z, lazy=False, loss=None):
        """lazy: False / 0 = dense-decay Adam on the whole table, True / 1 = batch rows only, 2 = replay (fit_z_sync first)."""
        _lib.check(self.lib.bgm_causal_fit_z_step(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(data_z), _ptr(zm), _ptr(zv),
                                                  _ptr(idx), 0, int(idx.numel()), int(batch_global), float(lr_z),
                                                  int(lazy), _ptr(loss), self._stream()),
                   "bgm_causal_fit_z_step")

    def fit_epoch(self, x, y, v, data_z, zm, zv, perm, batch, lr_theta, lr_z, lazy, loss=None, loss_z=None):
        """All minibatches perm[0:batch], perm[batch:2 batch], ... of one epoch with the loop inside the library
        (bgm_causal_fit_epoch; single process)."""
        _lib.check(self.lib.bgm_causal_fit_epoch(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(data_z), _ptr(zm), _ptr(zv), _ptr(perm),
                                                 int(perm.numel()), int(batch), float(lr_theta), float(lr_z), int(lazy), _ptr(loss),
                                                 _ptr(loss_z), self._stream()), "bgm_causal_fit_epoch")

    def fit_epoch_dp(self, comm, x, y, v, data_z, zm, zv, perm, batch, lr_theta, lr_z, lazy, loss=None, loss_z=None):
        """This rank's share of a data-parallel epoch (bgm_causal_fit_epoch_dp): `batch` local rows per minibatch, the fused g|f|h
        gradient summed over the ranks of `comm` (parallel.DeviceComm) by one ncclAllReduce per step enqueued inside the library."""
        _lib.check(self.lib.bgm_causal_fit_epoch_dp(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(data_z), _ptr(zm), _ptr(zv), _ptr(perm),
                                                    int(perm.numel()), int(batch), float(lr_theta), float(lr_z), int(lazy), _ptr(loss),
                                                    _ptr(loss_z), comm.handle, self._stream()), "bgm_causal_fit_epoch_dp")

    def describe(self, batch=32):
        """Kernel paths of this handle (sampling; minibatch steps when a fit session is open) as text."""
        buf = C.create_string_buffer(512)
        _lib.check(self.lib.bgm_causal_describe(self.h, int(batch), buf, 512), "bgm_causal_describe")
        return buf.value.decode()

    def fit_z_sync(self, data_z, zm, zv, idx, lr_z):
        """Replay mode: bring the rows idx (None = every row) of the latent table and its Adam slots up to the current step."""
        _lib.check(self.lib.bgm_causal_fit_z_sync(self.h, _ptr(data_z), _ptr(zm), _ptr(zv), _ptr(idx), 0 if idx is None else int(idx.numel()),
                                                  float(lr_z), self._stream()), "bgm_causal_fit_z_sync")

    def fit_z_grad(self, x, y, v, data_z, idx, batch_global, dz_out, loss=None):
        """d(batch-mean negative log joint, standard-normal prior)/d(batch rows of data_z) -> dz_out [batch x q]; no update."""
        _lib.check(self.lib.bgm_causal_fit_z_grad(self.h, _ptr(x), _ptr(y), _ptr(v), _ptr(data_z), _ptr(idx), 0, int(idx.numel()),
                                                  int(batch_global), _ptr(dz_out), _ptr(loss), self._stream()), "bgm_causal_fit_z_grad")

    def set_prior(self, seg=None, tab=None):
        """Conditional latent prior of the sampling calls made afterwards (bgm_causal_set_prior): seg int32 [n] (device), tab float32
        [n_segments x (q + 2)] = mu, 1 / sigma^2, (q / 2) log sigma^2 per segment (device).  None clears it."""
        self._prior_keep = (seg, tab)          # keep the buffers alive while set
        _lib.check(self.lib.bgm_causal_set_prior(self.h, _ptr(seg), _ptr(tab), 0 if tab is None else int(tab.shape[0])),
                   "bgm_causal_set_prior")

    def set_row_scale(self, scale=None, up=None, dn=None, s_min=RA.S_MIN, s_max=RA.S_MAX):
        """Per-chain proposal scale of the mh_run calls made afterwards (bgm_causal_set_row_scale): scale float32 [n] (device, in / out,
        aligned with the rows of those calls; written from q_sd by a call with init=True), up / dn float32 [n_table] (device): factor
        of iteration it < n_table for a chain that moved / did not.  scale=None switches back to the single q_sd."""
        self._row_scale_keep = (scale, up, dn)          # keep the buffers alive while set
        _lib.check(self.lib.bgm_causal_set_row_scale(self.h, _ptr(scale), _ptr(up), _ptr(dn), 0 if up is None else int(up.numel()),
                                                     float(s_min), float(s_max)), "bgm_causal_set_row_scale")

    def get_weights(self, net_id, dims):
        """Device parameters of one net -> [(W, b), ...] (Keras order)."""
        count = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
        buf = np.empty(count, np.float32)
        _lib.check(self.lib.bgm_causal_get_weights(self.h, int(net_id), buf.ctypes.data_as(C.c_void_p), count,
                                                   self._stream()), "bgm_causal_get_weights")
        out, off = [], 0
        for i in range(len(dims) - 1):
            nw = dims[i] * dims[i + 1]
            out.append((buf[off:off + nw].reshape(dims[i], dims[i + 1]).copy(),
                        buf[off + nw:off + nw + dims[i + 1]].copy()))
            off += nw + dims[i + 1]
        return out

    def fit_state(self, state=None):
        """Optimizer state of the open fit session (bgm_causal_fit_state): read -> dict(m, v, t_theta, t_z); pass such a
        dict to install it."""
        n = self.n_params
        steps = (C.c_int64 * 2)()
        if state is None:
            m, v = np.empty(n, np.float32), np.empty(n, np.float32)
            _lib.check(self.lib.bgm_causal_fit_state(self.h, 0, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), n, steps,
                                                     self._stream()), "bgm_causal_fit_state")
            return dict(m=m, v=v, t_theta=int(steps[0]), t_z=int(steps[1]))
        m = np.ascontiguousarray(state["m"], np.float32)
        v = np.ascontiguousarray(state["v"], np.float32)
        steps[0], steps[1] = int(state["t_theta"]), int(state["t_z"])
        _lib.check(self.lib.bgm_causal_fit_state(self.h, 1, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), n, steps,
                                                 self._stream()), "bgm_causal_fit_state")
        return None

    def fit_end(self):
        _lib.check(self.lib.bgm_causal_fit_end(self.h, self._stream()), "bgm_causal_fit_end")

    # -- EGM warm start (causalbgm/base.py:305-431) -------------------------------
    @staticmethod
    def flatten_disc(dz):
        """{'W','b','gamma','beta'} lists -> flat [W0..WL | b0..bL | gamma.. | beta..] (bgm_hip.h layout)."""
        return np.concatenate([np.asarray(a, np.float32).ravel() for k in ("W", "b", "gamma", "beta") for a in dz[k]])

    def egm_begin(self, batch_size, dz_units, lr, use_z_rec, dz):
        """Start a warm-start session from the installed g, e, f, h and the discriminator `dz`."""
        cfg = _lib.EgmConfig()
        cfg.batch_size = int(batch_size)
        cfg.n_hidden_dz = len(dz_units)
        for i, u in enumerate(dz_units):
            cfg.dz_units[i] = int(u)
        cfg.lr = float(lr)
        cfg.use_z_rec = int(bool(use_z_rec))
        theta = self.flatten_disc(dz) if isinstance(dz, dict) else np.ascontiguousarray(dz, np.float32)
        self._egm_counts = None
        _lib.check(self.lib.bgm_causal_egm_begin(self.h, C.byref(cfg), theta.ctypes.data_as(C.c_void_p), theta.size,
                                                 self._stream()), "bgm_causal_egm_begin")
        self._egm_n_dz = theta.size

    def egm_disc_step(self, z, idx, v, eps, apply=True, out=None):
        _lib.check(self.lib.bgm_causal_egm_disc_step(self.h, _ptr(z), _ptr(idx), _ptr(v), float(eps), int(bool(apply)),
                                                     _ptr(out), self._stream()), "bgm_causal_egm_disc_step")

    def egm_gen_step(self, z, idx, v, x, y, apply=True, out=None):
        _lib.check(self.lib.bgm_causal_egm_gen_step(self.h, _ptr(z), _ptr(idx), _ptr(v), _ptr(x), _ptr(y),
                                                    int(bool(apply)), _ptr(out), self._stream()), "bgm_causal_egm_gen_step")

    def egm_sizes(self):
        """(parameters of g | e | f | h, parameters of the discriminator): the buffer sizes of egm_grad / egm_apply."""
        return sum(self._w_count[k] for k in (_lib.NET_G, _lib.NET_E, _lib.NET_F, _lib.NET_H)), int(self._egm_n_dz)

    def egm_grad(self, which, scale, out):
        """Data-parallel warm start: the gradient of the last step run with apply=False, times `scale`, into the device tensor `out`."""
        _lib.check(self.lib.bgm_causal_egm_grad(self.h, int(which), float(scale), _ptr(out), out.numel(), self._stream()), "bgm_causal_egm_grad")

    def egm_apply(self, which, grad):
        """... and the Adam step of that optimizer from the (all-reduced) gradient."""
        _lib.check(self.lib.bgm_causal_egm_apply(self.h, int(which), _ptr(grad), grad.numel(), self._stream()), "bgm_causal_egm_apply")

    def egm_read(self, what, count):
        """what: 0 generator-side parameters [g|e|f|h], 1 discriminator, 2 / 3 last gen / disc gradients."""
        buf = np.empty(int(count), np.float32)
        _lib.check(self.lib.bgm_causal_egm_read(self.h, int(what), buf.ctypes.data_as(C.c_void_p), buf.size, self._stream()),
                   "bgm_causal_egm_read")
        return buf

    def egm_sync(self):
        _lib.check(self.lib.bgm_causal_egm_sync(self.h, self._stream()), "bgm_causal_egm_sync")

    def egm_end(self):
        _lib.check(self.lib.bgm_causal_egm_end(self.h, self._stream()), "bgm_causal_egm_end")

    OUTCOME_CACHE_NAMES = {"off": 0, "wave": 1, "chain": 2}

    @classmethod
    def outcome_cache_mode(cls, on):
        """bool (False = off, True = per chain), a name ('off' / 'wave' / 'chain') or the C ABI's number (0 / 1 / 2, bgm_hip.h) -> mode.
        (bools are resolved first: True == 1 in Python, but True means 'the default cache' = mode 2, the integer 1 means mode 1.)"""
        if isinstance(on, (bool, np.bool_)):
            return 2 if on else 0
        if isinstance(on, str) and on in cls.OUTCOME_CACHE_NAMES:
            return cls.OUTCOME_CACHE_NAMES[on]
        if isinstance(on, (int, np.integer)) and int(on) in (0, 1, 2):
            return int(on)
        raise ValueError("outcome cache mode must be False / 'off' / 0, 'wave' / 1 or True / 'chain' / 2; got %r" % (on,))

    def set_outcome_cache(self, on=True):
        """Retained phase of the effect samplers: False / 'off' = the outcome net at every retained draw (the reference); 'wave' = reuse
        the (mean, sd) of a 16-chain tile none of whose chains moved; True / 'chain' (default) = per chain, through the event form of the
        retained phase where it exists (csrc/causal_event_kernels.h), else 'wave'.  Bit-identical sums in every mode."""
        _lib.check(self.lib.bgm_causal_set_outcome_cache(self.h, self.outcome_cache_mode(on)), "bgm_causal_set_outcome_cache")

    def set_event_budget(self, n_bytes):
        """Upper bound on the event buffers of one segment of the retained phase in its event form (0: BGM_EVENT_BUDGET_MB or 8 GiB)."""
        _lib.check(self.lib.bgm_causal_set_event_budget(self.h, int(n_bytes)), "bgm_causal_set_event_budget")

    def outcome_cache_stats(self, reset=True):
        """(served, total) since the last reset: retained tile-iterations for the per-wave cache, retained chain-iterations for the
        event form (served = those that needed no outcome-net evaluation)."""
        out = (C.c_int64 * 2)()
        _lib.check(self.lib.bgm_causal_outcome_cache_stats(self.h, out, int(reset)), "bgm_causal_outcome_cache_stats")
        return int(out[0]), int(out[1])

    def timing_enable(self, on=True):
        _lib.check(self.lib.bgm_timing_enable(self.h, int(on)), "bgm_timing_enable")

    def timing_read(self, kind=-1, reset=True):
        """(launches, total ms) of the MH kernel launches of `kind` (EFFECT_*; -1 = all)."""
        n = C.c_int64()
        ms = C.c_double()
        _lib.check(self.lib.bgm_timing_read(self.h, int(kind), C.byref(n), C.byref(ms), int(reset)),
                   "bgm_timing_read")
        return n.value, ms.value

    # -- whole-sampler conveniences -------------------------------------------
    def mh_sample(self, x, y, v, burn_in, n_keep, q_sd, seed, chunk=None, want_draws=False,
                  effect=_lib.EFFECT_NONE, x_values=None, sample_y=True, row_base=0, adaptive=False,
                  initial_q_sd=1.0, target=0.25, tol=0.05, adj_int=50, window=100, acc_reduce=None, n_total=None, row_adapt=None,
                  row_adapt_table=None):
        """metropolis_hastings_sampler (+ fused infer_from_latent_posterior) over all rows.

        Returns dict(state, logp, acc_count [burn_in+n_keep], draws | None, adrf [n_doses,n_keep] | None,
        ite [n, n_keep] | None, q_sd).  acc_reduce / n_total: with the rows of one sampler run sharded over ranks, the all-reduce (sum)
        of the window's acceptance count and the total number of rows, so that every rank adapts the proposal scale identically.

        row_adapt = target acceptance rate (True = 0.25): every chain adapts a proposal scale of its own during burn-in, starting from
        q_sd (row_adapt.py; the fp32 LDS-resident kernels with the standard-normal prior, else RuntimeError).  One mh_run per chunk,
        no block-wide decisions; the result carries row_scale [n], the chains' final scales.  row_adapt_table = (up, dn) replaces the
        schedule of row_adapt_factors(burn_in, target)."""
        ra_target = RA.resolve_target(row_adapt)
        if ra_target is not None or row_adapt_table is not None:
            if adaptive:
                raise ValueError("mh_sample: row_adapt and the block-wide adaptive scale (adaptive=True) exclude each other")
            if q_sd is None or not float(q_sd) > 0:
                raise ValueError("mh_sample: row_adapt starts every chain from q_sd, which must be positive; got %r" % (q_sd,))
            up, dn = row_adapt_table if row_adapt_table is not None else RA.row_adapt_factors(burn_in, ra_target)
            up, dn = (_f32(np.asarray(t, dtype=np.float32).reshape(-1), self.device) for t in (up, dn))
            if up.numel() != dn.numel():
                raise ValueError("mh_sample: row_adapt_table = (up, dn) of equal length")
            scale = torch.empty(v.shape[0], device=self.device, dtype=torch.float32)
            self.set_row_scale(scale, up if up.numel() else None, dn if dn.numel() else None)
            try:
                out = self.mh_sample(x, y, v, burn_in, n_keep, q_sd, seed, chunk=chunk, want_draws=want_draws, effect=effect,
                                     x_values=x_values, sample_y=sample_y, row_base=row_base)
            finally:
                self.set_row_scale(None)
            out["row_scale"] = scale
            return out
        dev = self.device
        x, y, v = (_f32(t, dev) for t in (x, y, v))
        x = x.reshape(-1)
        y = y.reshape(-1)
        n = v.shape[0]
        total = burn_in + n_keep
        state = torch.empty((n, self.q), device=dev, dtype=torch.float32)
        logp = torch.empty(n, device=dev, dtype=torch.float32)
        acc = torch.zeros(total, device=dev, dtype=torch.int32)
        draws = torch.empty((n_keep, n, self.q), device=dev, dtype=torch.float32) if want_draws else None
        xv = partial = ite = None
        n_slots = self.mh_slots(n)
        if effect == _lib.EFFECT_ADRF:
            xv = _f32(np.atleast_1d(np.asarray(x_values, dtype=np.float32)), dev)
            partial = torch.zeros((n_slots, n_keep, xv.numel()), device=dev, dtype=torch.float32)
        elif effect == _lib.EFFECT_ITE:
            ite = torch.empty((n, n_keep), device=dev, dtype=torch.float32)
        if adaptive:
            q_sd = initial_q_sd
            chunk = adj_int  # q_sd may change every adj_int iterations during burn-in (base.py:880)
        if chunk is None:
            chunk = total
        it = 0
        while it < total:
            # segment boundaries: the adaptive rule looks at the window *after* iteration it
            # where it % adj_int == 0, i.e. q_sd changes between it and it+1.
            if adaptive and it < burn_in:
                nxt = min(((it // adj_int) + 1) * adj_int + 1, total) if it > 0 else min(adj_int + 1, total)
            else:
                nxt = min(it + (chunk if not adaptive else total), total)
            self.mh_run(x, y, v, state, logp, it, nxt - it, burn_in, q_sd, seed, init=(it == 0),
                        row_base=row_base, acc_count=acc, draws=draws, n_keep=n_keep, effect=effect,
                        sample_y=sample_y, x_values=xv, adrf_partial=partial, ite=ite)
            it = nxt
            last = it - 1  # counter value of the iteration just finished
            if adaptive and last < burn_in and last % adj_int == 0 and last > 0:
                w0 = max(0, last + 1 - window)
                cnt = acc[w0:last + 1].sum().double().reshape(1)
                if acc_reduce is not None:          # rows sharded over ranks: ONE acceptance window over all rows, the same decision everywhere
                    cnt = acc_reduce(cnt)
                rate = float(cnt.item()) / ((last + 1 - w0) * (n if n_total is None else n_total))
                if rate < target - tol:
                    q_sd *= 0.9
                elif rate > target + tol:
                    q_sd *= 1.1
        adrf = None
        if effect == _lib.EFFECT_ADRF:
            adrf = self.adrf_reduce(partial, n_slots, xv.numel(), n_keep, n)
        return dict(state=state, logp=logp, acc_count=acc, draws=draws, adrf=adrf, ite=ite, q_sd=q_sd,
                    adrf_partial=partial, n_slots=n_slots)


def flatten_varnet(g):
    """oracle/reference BaseVariationalNet dict -> flat float32 in the order of bgm_bgm_set_weights."""
    parts = [g["bn"]["gamma"], g["bn"]["beta"], g["bn"]["mean"], g["bn"]["var"]]
    for W, b in g["trunk"]:
        parts += [W, b]
    parts += [g["mean"][0], g["mean"][1], g["var"][0], g["var"][1]]
    return np.concatenate([np.asarray(a, np.float32).ravel() for a in parts]).astype(np.float32)


def missing_slots(x, k_slots=None):
    """(slot int32 [n, p], k_slots) of the NaN cells of x [n, p] on the device: the k-th missing cell of a row has slot k, observed
    cells -1 (the map of predict_draws' cells and of hmc_run_rows' cells / tails); k_slots: the largest count of a row, at least 1,
    unless given (a width shared by all ranks)."""
    miss = torch.isnan(x)
    slot = (torch.cumsum(miss, dim=1, dtype=torch.int32) - 1).to(torch.int32)
    slot.masked_fill_(~miss, -1)
    if k_slots is None:
        k_slots = max(1, int(miss.sum(dim=1).max().item())) if x.shape[0] else 1
    return slot.contiguous(), int(k_slots)


class BgmEngine(object):
    """Device-side state of one BGM generator (BaseVariationalNet, inference mode) + kernels."""

    def __init__(self, x_dim, z_dim, g_units=None, device=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("bayesgm_amd: no HIP device visible; the hot path has no CPU fallback")
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        torch.cuda.init()
        torch.zeros(1, device=self.device)
        self.p, self.q = int(x_dim), int(z_dim)
        units = list(DEFAULT_G_UNITS if g_units is None else g_units)
        self.units = units
        cfg = _lib.BgmConfig()
        cfg.x_dim, cfg.z_dim, cfg.n_hidden_g = self.p, self.q, len(units)
        for i, u in enumerate(units):
            cfg.g_units[i] = int(u)
        self.h = C.c_void_p()
        _lib.check(self.lib.bgm_create(C.byref(self.h), self.device.index), "bgm_create")
        _lib.check(self.lib.bgm_bgm_configure(self.h, C.byref(cfg)), "bgm_bgm_configure")

    def set_disc_norm(self, mode):
        """BatchNormalization mode of the EGM discriminators opened afterwards: "batch" | "fixed" (bgm_set_disc_norm)."""
        _lib.check(self.lib.bgm_set_disc_norm(self.h, {"batch": 0, "fixed": 1}[mode]), "bgm_set_disc_norm")

    HMC_PRECISIONS = {"fp32": 0, "f16x3": 2}

    def set_precision(self, mode="fp32"):
        """Arithmetic of the generator's products in logpost / hmc_run: "fp32" (default) or "f16x3" (split precision on the
        fp16 matrix instruction, opt-in; bgm_bgm_set_precision)."""
        if mode not in self.HMC_PRECISIONS:
            raise ValueError("hmc precision must be 'fp32' or 'f16x3'; got %r" % (mode,))
        _lib.check(self.lib.bgm_bgm_set_precision(self.h, self.HMC_PRECISIONS[mode]), "bgm_bgm_set_precision")

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.bgm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_weights(self, g):
        theta = flatten_varnet(g) if isinstance(g, dict) else np.ascontiguousarray(g, np.float32)
        _lib.check(self.lib.bgm_bgm_set_weights(self.h, theta.ctypes.data_as(C.c_void_p), theta.size, self._stream()),
                   "bgm_bgm_set_weights")

    def logpost(self, z, x, want_grad=False):
        """get_log_posterior (bgm/base.py:665-705); x carries NaN at missing cells."""
        z, x = _f32(z, self.device), _f32(x, self.device)
        n = x.shape[0]
        out = torch.empty(n, device=self.device, dtype=torch.float32)
        grad = torch.empty((n, self.q), device=self.device, dtype=torch.float32) if want_grad else None
        _lib.check(self.lib.bgm_bgm_logpost(self.h, _ptr(z), _ptr(x), n, _ptr(out), _ptr(grad), self._stream()),
                   "bgm_bgm_logpost")
        return (out, grad) if want_grad else out

    @staticmethod
    def _hmc_args(x, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, init, row_base, acc_prob, acc_count, draws):
        a = _lib.HmcArgs()
        a.x_dev = x.data_ptr(); a.n = x.shape[0]; a.row_base = int(row_base)
        a.state_dev, a.logp_dev, a.grad_dev = state.data_ptr(), logp.data_ptr(), grad.data_ptr()
        a.init = int(bool(init)); a.it_begin = int(it_begin); a.n_iters = int(n_iters); a.burn_in = int(burn_in)
        a.n_leapfrog = int(n_leapfrog); a.step_dev = step.data_ptr(); a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        a.acc_prob_sum_dev = acc_prob.data_ptr() if acc_prob is not None else None
        a.acc_count_dev = acc_count.data_ptr() if acc_count is not None else None
        a.draws_dev = draws.data_ptr() if draws is not None else None
        return a

    def hmc_run(self, x, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, init=False,
                row_base=0, acc_prob=None, acc_count=None, draws=None):
        a = self._hmc_args(x, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, init, row_base, acc_prob, acc_count,
                           draws)
        _lib.check(self.lib.bgm_bgm_hmc_run(self.h, C.byref(a), self._stream()), "bgm_bgm_hmc_run")

    def hmc_run_rows(self, x, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, init=False, row_base=0, up=None,
                     dn=None, s_min=RA.S_MIN, s_max=RA.S_MAX, acc_prob=None, acc_count=None, draws=None, max_trajectory=None, jitter=False,
                     n_steps=None, moments=None, cells=None, slot=None, k_slots=0, n_keep=None, add_noise=True, tails=None, k_tail=0):
        """hmc_run with a step size per chain (bgm_bgm_hmc_run_rows): step float32 [n], in / out; up / dn: the factor tables of
        row_adapt.row_adapt_factors on the device (None: the steps stay as given).

        moments (opt-in, bgm_bgm_hmc_run_rows_impute, fp32): float32 [3, n, p], in / out.  Every iteration it >= burn_in decodes the
        state it ends on and keeps, for the NaN cells of x only, plane 0 = the predictive value at it == burn_in, plane 1 += x - ref,
        plane 2 += (x - ref)^2; nothing else of the planes is written.  cells float32 [n * k_slots, n_keep] with slot int32 [n, p]:
        the values themselves as well, in predict_draws' layout.  n_keep: the retained iterations of the whole run (default: those of
        this call).  The chain is the one the call makes without these arguments, bit for bit.

        tails with k_tail = K (opt-in, bgm_bgm_hmc_run_rows_impute_tails; needs moments, slot and k_slots >= 1): float32
        [2, K, n, k_slots], in / out.  For every missing cell with a slot, tail 0 collects the K smallest and tail 1 the K largest of
        its retained predictive values, each a heap in no sorted order (row_tail_quantiles reads them); 1 <= K <= n_keep.  Retained
        draw 0 initialises the series it owns, nothing else of the buffer is written.  Chain, moments and cells are those of the call
        without tails.

        max_trajectory / jitter / n_steps (opt-in, bgm_bgm_hmc_run_rows_traj): a number of leapfrog steps per chain, from the chain's
        own step -- capped so that step x steps stays below max_trajectory (row_adapt.leapfrog_cap), drawn uniformly from 1 .. cap
        per transition with jitter; n_steps int32 [n], in / out, gains the steps every chain took.  Every transition still costs
        n_leapfrog evaluations: the option buys mixing, not time."""
        a = self._hmc_args(x, state, logp, grad, step, it_begin, n_iters, burn_in, n_leapfrog, seed, init, row_base, acc_prob, acc_count,
                           draws)
        if tails is not None and (moments is None or slot is None or int(k_slots) < 1):
            raise ValueError("hmc_run_rows: tails needs moments, slot and k_slots >= 1 (the fused imputation with the slot map of its "
                             "missing cells, bgm_bgm_hmc_run_rows_impute_tails)")
        if tails is None and k_tail:
            raise ValueError("hmc_run_rows: k_tail belongs to tails; got k_tail = %r without tails" % (k_tail,))
        if moments is not None or cells is not None:
            if moments is None:
                raise ValueError("hmc_run_rows: cells needs moments (the fused imputation, bgm_bgm_hmc_run_rows_impute)")
            try:
                T = 0.0 if max_trajectory is None else float(max_trajectory)
                jit = int(jitter)
            except (TypeError, ValueError):
                raise ValueError("hmc_run_rows: max_trajectory must be None or a number and jitter a bool; got %r, %r" % (max_trajectory, jitter))
            n, p = x.shape
            if moments.dtype != torch.float32 or tuple(moments.shape) != (3, n, p) or not moments.is_contiguous():
                raise ValueError("hmc_run_rows: moments must be a contiguous float32 tensor [3, n, p] = [3, %d, %d]; got %s %s"
                                 % (n, p, moments.dtype, tuple(moments.shape)))
            keep = max(0, int(it_begin) + int(n_iters) - int(burn_in)) if n_keep is None else int(n_keep)
            if cells is not None and (cells.dtype != torch.float32 or cells.numel() != n * int(k_slots) * keep or not cells.is_contiguous()):
                raise ValueError("hmc_run_rows: cells must be a contiguous float32 tensor of n * k_slots * n_keep = %d values; got %s %s"
                                 % (n * int(k_slots) * keep, cells.dtype, tuple(cells.shape)))
            if slot is not None and (slot.dtype != torch.int32 or tuple(slot.shape) != (n, p) or not slot.is_contiguous()):
                raise ValueError("hmc_run_rows: slot must be a contiguous int32 tensor [n, p]; got %s %s" % (slot.dtype, tuple(slot.shape)))
            if tails is not None:
                if (tails.dtype != torch.float32 or tuple(tails.shape) != (2, int(k_tail), n, int(k_slots)) or not tails.is_contiguous()
                        or int(k_tail) < 1):
                    raise ValueError("hmc_run_rows: tails must be a contiguous float32 tensor [2, k_tail, n, k_slots] = [2, %d, %d, %d] with "
                                     "k_tail >= 1; got %s %s" % (int(k_tail), n, int(k_slots), tails.dtype, tuple(tails.shape)))
                # the one way the kernel could write out of bounds: checked once per call, on the device
                if n > 0 and int(slot.max().item()) >= int(k_slots):
                    raise ValueError("hmc_run_rows: slot holds an entry >= k_slots = %d (max %d): the tails of that cell would lie outside "
                                     "its row's series" % (int(k_slots), int(slot.max().item())))
                _lib.check(self.lib.bgm_bgm_hmc_run_rows_impute_tails(self.h, C.byref(a), _ptr(up), _ptr(dn), 0 if up is None else int(up.numel()),
                                                                      float(s_min), float(s_max), T, jit, _ptr(n_steps), _ptr(moments),
                                                                      _ptr(cells), _ptr(slot), int(k_slots), keep, int(bool(add_noise)),
                                                                      _ptr(tails), int(k_tail), self._stream()),
                           "bgm_bgm_hmc_run_rows_impute_tails")
                return
            _lib.check(self.lib.bgm_bgm_hmc_run_rows_impute(self.h, C.byref(a), _ptr(up), _ptr(dn), 0 if up is None else int(up.numel()),
                                                            float(s_min), float(s_max), T, jit, _ptr(n_steps), _ptr(moments), _ptr(cells),
                                                            _ptr(slot), int(k_slots), keep, int(bool(add_noise)), self._stream()),
                       "bgm_bgm_hmc_run_rows_impute")
            return
        if max_trajectory is not None or jitter is not False or n_steps is not None:
            # (the C entry checks the two values itself, as it does s_min / s_max: what is not a number at all is refused here)
            try:
                T = 0.0 if max_trajectory is None else float(max_trajectory)
                jit = int(jitter)
            except (TypeError, ValueError):
                raise ValueError("hmc_run_rows: max_trajectory must be None or a number and jitter a bool; got %r, %r" % (max_trajectory, jitter))
            _lib.check(self.lib.bgm_bgm_hmc_run_rows_traj(self.h, C.byref(a), _ptr(up), _ptr(dn), 0 if up is None else int(up.numel()),
                                                          float(s_min), float(s_max), T, jit, _ptr(n_steps), self._stream()),
                       "bgm_bgm_hmc_run_rows_traj")
            return
        _lib.check(self.lib.bgm_bgm_hmc_run_rows(self.h, C.byref(a), _ptr(up), _ptr(dn), 0 if up is None else int(up.numel()), float(s_min),
                                                 float(s_max), self._stream()), "bgm_bgm_hmc_run_rows")

    def hmc_adapt(self, step, acc_prob, it, n_chains, target=0.75, rate=0.01):
        _lib.check(self.lib.bgm_bgm_hmc_adapt(self.h, _ptr(step), _ptr(acc_prob), int(it), float(n_chains),
                                              float(target), float(rate), self._stream()), "bgm_bgm_hmc_adapt")

    def hmc_sample(self, x, n_mcmc, burn_in, step_size=0.01, n_leapfrog=10, seed=42, row_base=0, want_draws=True,
                   n_chains_global=None, reduce_fn=None, row_adapt=None, max_trajectory=None, jitter=False, impute=False, add_noise=True,
                   tails=None):
        """tfp_mcmc_sampler (bgm/base.py:709-830): HMC + SimpleStepSizeAdaptation over int(0.8*burn_in)
        steps, all rows one chain each.  `reduce_fn(tensor)` all-reduces the per-iteration acceptance
        statistic across ranks (the step size is shared by ALL chains).

        row_adapt = target acceptance rate in (0, 1) (opt-in): every chain carries a step of its own instead, starting at step_size and
        multiplied after each of the burn_in decisions by the factor of row_adapt.row_adapt_factors(burn_in, row_adapt) for "moved" /
        "did not"; burn-in and retained draws run in ONE launch, reduce_fn is not called, and the result holds row_step [n] instead
        of step.  max_trajectory / jitter (with row_adapt only): the number of leapfrog steps per chain of hmc_run_rows; the result
        then holds n_steps int32 [n] as well, the steps every chain took over the n_mcmc retained transitions.

        impute=True (with row_adapt only, fp32): the predictive moments of the NaN cells of x are summed inside the sampler (hmc_run_rows
        with moments); the result holds moments float32 [3, n, p] (NaN where nothing was written) and no draws are allocated.
        tails = K (with impute only, 1 <= K <= n_mcmc): the K smallest and the K largest predictive values of every missing cell are
        kept as well (hmc_run_rows with tails); the result also holds tails float32 [2, K, n, k_slots] (zero where nothing was
        written), slot int32 [n, p] (the k-th missing cell of a row has slot k, observed cells -1) and k_slots, from which
        row_tail_quantiles gives the exact quantile bounds (K = causal_hmc.tail_size(alpha, n_mcmc))."""
        T, jit = RA.resolve_trajectory(row_adapt, max_trajectory, jitter, what="hmc_sample: max_trajectory / jitter")
        if impute:
            if row_adapt is None:
                raise ValueError("hmc_sample: impute needs row_adapt (the fused imputation lives in the per-chain step kernel)")
            want_draws = False
        if tails is not None:
            if not impute:
                raise ValueError("hmc_sample: tails belongs to impute=True (the tails of the fused imputation's predictive values)")
            if isinstance(tails, bool) or int(tails) != tails or not 1 <= int(tails) <= int(n_mcmc):
                raise ValueError("hmc_sample: tails must be an integer K with 1 <= K <= n_mcmc = %d; got %r" % (int(n_mcmc), tails))
        dev = self.device
        x = _f32(x, dev)
        n = x.shape[0]
        total = burn_in + n_mcmc
        state = torch.empty((n, self.q), device=dev)
        logp = torch.empty(n, device=dev)
        grad = torch.empty((n, self.q), device=dev)
        step = torch.full((1,), float(step_size), device=dev, dtype=torch.float32)
        acc_prob = torch.zeros(total, device=dev, dtype=torch.float64)
        acc_count = torch.zeros(total, device=dev, dtype=torch.int32)
        draws = torch.empty((n_mcmc, n, self.q), device=dev) if want_draws else None
        if row_adapt is not None:
            up, dn = self.row_step_table(burn_in, row_adapt)
            step = torch.full((n,), float(step_size), device=dev, dtype=torch.float32)
            if impute:      # (one launch; the planes are the only per-cell memory)
                moments = torch.full((3, n, self.p), float("nan"), device=dev, dtype=torch.float32)
                n_steps = torch.zeros(n, device=dev, dtype=torch.int32) if (T > 0.0 or jit) else None
                tr = dict(max_trajectory=T if T > 0.0 else None, jitter=bool(jit))
                tkw = {}
                if tails is not None:
                    slot, k_slots = missing_slots(x)
                    tkw = dict(slot=slot, k_slots=k_slots, k_tail=int(tails),
                               tails=torch.zeros((2, int(tails), n, k_slots), device=dev, dtype=torch.float32))
                first = 0
                if n_steps is not None and burn_in > 0:      # (n_steps counts the retained transitions alone, as below)
                    self.hmc_run_rows(x, state, logp, grad, step, 0, burn_in, burn_in, n_leapfrog, seed, init=True, row_base=row_base,
                                      up=up, dn=dn, acc_prob=acc_prob, acc_count=acc_count, **tr)
                    first = burn_in
                if total > first:
                    self.hmc_run_rows(x, state, logp, grad, step, first, total - first, burn_in, n_leapfrog, seed, init=(first == 0),
                                      row_base=row_base, up=up, dn=dn, acc_prob=acc_prob, acc_count=acc_count, n_steps=n_steps,
                                      moments=moments, n_keep=max(1, n_mcmc), add_noise=add_noise, **tr, **tkw)
                out = dict(state=state, logp=logp, grad=grad, row_step=step, acc_prob=acc_prob, acc_count=acc_count, draws=None, moments=moments)
                if tails is not None:
                    out.update(tails=tkw["tails"], slot=tkw["slot"], k_slots=tkw["k_slots"])
                if n_steps is not None:
                    out["n_steps"] = n_steps
                return out
            if T > 0.0 or jit:      # (two launches, so that n_steps counts the retained transitions alone: a cut changes nothing else)
                n_steps = torch.zeros(n, device=dev, dtype=torch.int32)
                tr = dict(max_trajectory=T if T > 0.0 else None, jitter=bool(jit))
                if burn_in > 0:
                    self.hmc_run_rows(x, state, logp, grad, step, 0, burn_in, burn_in, n_leapfrog, seed, init=True, row_base=row_base,
                                      up=up, dn=dn, acc_prob=acc_prob, acc_count=acc_count, **tr)
                if n_mcmc > 0:
                    self.hmc_run_rows(x, state, logp, grad, step, burn_in, n_mcmc, burn_in, n_leapfrog, seed, init=(burn_in == 0),
                                      row_base=row_base, up=up, dn=dn, acc_prob=acc_prob, acc_count=acc_count, draws=draws,
                                      n_steps=n_steps, **tr)
                return dict(state=state, logp=logp, grad=grad, row_step=step, n_steps=n_steps, acc_prob=acc_prob, acc_count=acc_count,
                            draws=draws)
            if total > 0:
                self.hmc_run_rows(x, state, logp, grad, step, 0, total, burn_in, n_leapfrog, seed, init=True, row_base=row_base, up=up,
                                  dn=dn, acc_prob=acc_prob, acc_count=acc_count, draws=draws)
            return dict(state=state, logp=logp, grad=grad, row_step=step, acc_prob=acc_prob, acc_count=acc_count, draws=draws)
        n_adapt = int(burn_in * 0.8)
        n_all = float(n_chains_global if n_chains_global is not None else n)
        it = 0
        while it < n_adapt:          # one launch per transition: the step size changes after each
            self.hmc_run(x, state, logp, grad, step, it, 1, burn_in, n_leapfrog, seed, init=(it == 0),
                         row_base=row_base, acc_prob=acc_prob, acc_count=acc_count, draws=draws)
            if reduce_fn is not None:
                reduce_fn(acc_prob[it:it + 1])
            self.hmc_adapt(step, acc_prob, it, n_all)
            it += 1
        if it < total:
            self.hmc_run(x, state, logp, grad, step, it, total - it, burn_in, n_leapfrog, seed, init=(it == 0),
                         row_base=row_base, acc_prob=acc_prob, acc_count=acc_count, draws=draws)
        return dict(state=state, logp=logp, grad=grad, step=step, acc_prob=acc_prob, acc_count=acc_count, draws=draws)

    def row_step_table(self, burn_in, target):
        """(up, dn) of row_adapt.row_adapt_factors(burn_in, target) on the device, or (None, None) when burn_in = 0 (nothing adapts)."""
        up, dn = RA.row_adapt_factors(burn_in, target)      # (refuses a target outside (0, 1))
        if up.size == 0:
            return None, None
        return _f32(up, self.device), _f32(dn, self.device)

    def predict_draws(self, draws, burn_in, seed, slot=None, k_slots=0, want_full=False, row_base=0, want_var=False,
                      add_noise=True):
        """predict_on_posteriors (bgm/base.py:511-525) -> (cells [n*k_slots, n_draws] | None, full | None[, var])."""
        n_draws, n, _ = draws.shape
        cells = torch.zeros((n * k_slots, n_draws), device=self.device) if slot is not None else None
        full = torch.empty((n_draws, n, self.p), device=self.device) if want_full else None
        var = torch.empty((n_draws, n, self.p), device=self.device) if want_var else None
        _lib.check(self.lib.bgm_bgm_predict_draws(self.h, _ptr(draws), n, int(row_base), n_draws, int(burn_in),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(slot), int(k_slots),
                                                  _ptr(cells), _ptr(full), _ptr(var), int(bool(add_noise)),
                                                  self._stream()), "bgm_bgm_predict_draws")
        return (cells, full, var) if want_var else (cells, full)

    # -- EGM warm start (bgm/base.py:190-340) ------------------------------------
    def egm_begin(self, batch_size, e_units, dz_units, dx_units, lr, gamma, alpha, e_net, dz, dx):
        """Session from the installed generator, the encoder `e_net` ([(W, b)..]) and the discriminators (dicts)."""
        cfg = _lib.BgmEgmConfig()
        cfg.batch_size = int(batch_size)
        for name, units in (("e", e_units), ("dz", dz_units), ("dx", dx_units)):
            setattr(cfg, "n_hidden_" + name, len(units))
            arr = getattr(cfg, name + "_units")
            for i, u in enumerate(units):
                arr[i] = int(u)
        cfg.lr, cfg.gamma, cfg.alpha = float(lr), float(gamma), float(alpha)
        te = flatten_net(e_net)
        tz, tx = CausalEngine.flatten_disc(dz), CausalEngine.flatten_disc(dx)
        _lib.check(self.lib.bgm_bgm_egm_begin(self.h, C.byref(cfg), te.ctypes.data_as(C.c_void_p), te.size,
                                              tz.ctypes.data_as(C.c_void_p), tz.size, tx.ctypes.data_as(C.c_void_p), tx.size,
                                              self._stream()), "bgm_bgm_egm_begin")
        self._egm_sizes = (self.n_theta(), te.size, tz.size, tx.size)

    def egm_disc_step(self, z, x, noise, eps_z, eps_x, apply=True, out=None):
        _lib.check(self.lib.bgm_bgm_egm_disc_step(self.h, _ptr(z), _ptr(x), _ptr(noise), float(eps_z), float(eps_x),
                                                  int(bool(apply)), _ptr(out), self._stream()), "bgm_bgm_egm_disc_step")

    def egm_gen_step(self, z, x, noise1, noise2, apply=True, out=None):
        _lib.check(self.lib.bgm_bgm_egm_gen_step(self.h, _ptr(z), _ptr(x), _ptr(noise1), _ptr(noise2), int(bool(apply)),
                                                 _ptr(out), self._stream()), "bgm_bgm_egm_gen_step")

    def egm_read(self, what):
        """0: generator side [g | e], 1: discriminators [dz | dx], 2 / 3: gradients of the last gen / disc step."""
        n_g, n_e, n_dz, n_dx = self._egm_sizes
        buf = np.empty((n_g + n_e) if what in (0, 2) else (n_dz + n_dx), np.float32)
        _lib.check(self.lib.bgm_bgm_egm_read(self.h, int(what), buf.ctypes.data_as(C.c_void_p), buf.size, self._stream()),
                   "bgm_bgm_egm_read")
        return buf

    def egm_write(self, what, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        _lib.check(self.lib.bgm_bgm_egm_write(self.h, int(what), buf.ctypes.data_as(C.c_void_p), buf.size, self._stream()),
                   "bgm_bgm_egm_write")

    def egm_encode(self, x):
        x = _f32(x, self.device)
        z = torch.empty((x.shape[0], self.q), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.bgm_bgm_egm_encode(self.h, _ptr(x), x.shape[0], _ptr(z), self._stream()), "bgm_bgm_egm_encode")
        return z

    def egm_sync(self):
        _lib.check(self.lib.bgm_bgm_egm_sync(self.h, self._stream()), "bgm_bgm_egm_sync")

    def egm_end(self):
        _lib.check(self.lib.bgm_bgm_egm_end(self.h, self._stream()), "bgm_bgm_egm_end")

    def row_mean_quantiles(self, mat, q_lo, q_hi):
        mat = mat.contiguous()
        n_rows, m = mat.shape
        mean = torch.empty(n_rows, device=self.device, dtype=torch.float32)
        lo = torch.empty_like(mean)
        hi = torch.empty_like(mean)
        _lib.check(self.lib.bgm_row_mean_quantiles(self.h, _ptr(mat), n_rows, m, float(q_lo), float(q_hi),
                                                   _ptr(mean), _ptr(lo), _ptr(hi), self._stream()),
                   "bgm_row_mean_quantiles")
        return mean, lo, hi

    def row_tail_quantiles(self, tails, m, q_lo, q_hi):
        """tails [2, K, n, k_slots] float32 on the device (hmc_run_rows with tails, hmc_sample's out["tails"]) -> (lo, hi) [n, k_slots]:
        the quantiles row_mean_quantiles gives on the m stored cells of every series, bit for bit (bgm_row_tail_quantiles); series a
        row does not use hold whatever the buffer held.  K below what (m, q_lo, q_hi) need (causal_hmc.tail_size) raises the
        library's error."""
        return _row_tail_quantiles(self, tails, m, q_lo, q_hi)

    # -- fit step functions (bgm/base.py:145-187) ---------------------------------
    def fit_begin(self, n_rows, max_batch):
        _lib.check(self.lib.bgm_bgm_fit_begin(self.h, int(n_rows), int(max_batch), self._stream()), "bgm_bgm_fit_begin")
        n = C.c_int64()
        _lib.check(self.lib.bgm_bgm_fit_n_params(self.h, C.byref(n)), "bgm_bgm_fit_n_params")
        self.n_params = n.value
        return n.value

    def fit_set_global_batch(self, batch_global):
        _lib.check(self.lib.bgm_bgm_fit_set_global_batch(self.h, int(batch_global)), "bgm_bgm_fit_set_global_batch")

    def fit_theta_grad(self, x, data_z, idx, grad, loss=None):
        _lib.check(self.lib.bgm_bgm_fit_theta_grad(self.h, _ptr(x), _ptr(data_z), _ptr(idx), int(idx.numel()), _ptr(grad),
                                                   _ptr(loss), self._stream()), "bgm_bgm_fit_theta_grad")

    def fit_theta_apply(self, grad, lr_theta):
        _lib.check(self.lib.bgm_bgm_fit_theta_apply(self.h, _ptr(grad), float(lr_theta), self._stream()),
                   "bgm_bgm_fit_theta_apply")

    def fit_z_step(self, x, data_z, idx, lr_z, loss=None):
        _lib.check(self.lib.bgm_bgm_fit_z_step(self.h, _ptr(x), _ptr(data_z), _ptr(idx), int(idx.numel()), float(lr_z),
                                               _ptr(loss), self._stream()), "bgm_bgm_fit_z_step")

    def fit_epoch(self, x, data_z, perm, n_steps, batch, lr_theta, lr_z, loss=None):
        """The minibatches perm[k * batch : (k + 1) * batch], k < n_steps, in ONE library call (bgm_bgm_fit_epoch)."""
        _lib.check(self.lib.bgm_bgm_fit_epoch(self.h, _ptr(x), _ptr(data_z), _ptr(perm), int(n_steps), int(batch), float(lr_theta),
                                              float(lr_z), _ptr(loss), self._stream()), "bgm_bgm_fit_epoch")

    def get_weights(self):
        """Device parameters -> generator dict (bn / trunk / mean / var)."""
        buf = np.empty(self.n_theta(), np.float32)
        _lib.check(self.lib.bgm_bgm_get_weights(self.h, buf.ctypes.data_as(C.c_void_p), buf.size, self._stream()),
                   "bgm_bgm_get_weights")
        q, p = self.q, self.p
        g = {"bn": {"gamma": buf[:q].copy(), "beta": buf[q:2 * q].copy(), "mean": buf[2 * q:3 * q].copy(),
                    "var": buf[3 * q:4 * q].copy()}, "trunk": []}
        o, d_in = 4 * q, q
        for u in self.units:
            g["trunk"].append((buf[o:o + d_in * u].reshape(d_in, u).copy(), buf[o + d_in * u:o + d_in * u + u].copy()))
            o += d_in * u + u
            d_in = u
        for k in ("mean", "var"):
            g[k] = (buf[o:o + d_in * p].reshape(d_in, p).copy(), buf[o + d_in * p:o + d_in * p + p].copy())
            o += d_in * p + p
        return g

    def n_theta(self):
        n, d_in = 4 * self.q, self.q
        for u in self.units:
            n += d_in * u + u
            d_in = u
        return n + 2 * (d_in * self.p + self.p)

    def fit_end(self):
        _lib.check(self.lib.bgm_bgm_fit_end(self.h, self._stream()), "bgm_bgm_fit_end")
