#!/usr/bin/env python3
"""Development aid: SHA-256 of everything the CausalBGM HMC kernels return, to show that two builds of libbgm_hip.so compute the
same bytes on one GPU (the companion of compare_code_objects.py for kernels whose code objects differ).

    BGM_HIP_LIB=A/libbgm_hip.so timeout -k 10 300 python scripts/digest_causal_hmc.py [--models] --out a.json
    BGM_HIP_LIB=B/libbgm_hip.so timeout -k 10 300 python scripts/digest_causal_hmc.py [--models] --out b.json
    python scripts/digest_causal_hmc.py --compare a.json a_again.json b.json

One process per library.  Engine.hmc_sample with burn_in = 12, n_keep = 10, n_leapfrog = 3 on the smallest shapes at which the
kernels take another path -- q = 10 continuous with n = 200, q = 18 binary with n = 150 (two K tiles in the first layers), n = 17 (a
partial second tile) -- over every kernel of chmc_run (csrc/causal_hmc_fx_kernels.h): identity mass with draws; a given non-unit
metric; a metric estimated over one window (the moment sums); ADRF or ITE inside the sampler; row effects with their draws
(continuous); sums over 3 labels (binary); the three effect routes again with the metric; and the kernels for partially observed
rows (partial=True; y NaN in a third of the rows, x and y NaN in another third): without an effect, with a metric, with the ITE
(binary) and with row effects (continuous).
--models: what the class returns and leaves on itself (hmc_row_step_, hmc_row_mass_, individual_sd_, average_effects_,
last_acceptance_rate) on a panel of n = 40 with burn_in = 24, n_mcmc = 10, n_leapfrog = 3 and, where a route takes a draw budget,
draw_budget_bytes = 1, so that the row blocks are the 16-row minimum: three blocks (16 / 16 / 8), the last a partial row tile, two
with row_base > 0.  Weights from set_weights, no fit.  predict(sampler='hmc') by draws and fused, predict_individual with both
intervals, predict_new, predict_average with 3 groups, hmc_sampler(mass='diag').
--compare FIRST SECOND OTHER: tensors whose digests differ between FIRST and SECOND (two runs of one build) are named and left out;
every other digest of OTHER must equal FIRST's.  Exit status 1 otherwise.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = [dict(z_dims=[1, 1, 1, 7], p=200, binary=False, n=200),
          dict(z_dims=[3, 3, 6, 6], p=100, binary=True, n=150),
          dict(z_dims=[1, 1, 1, 7], p=20, binary=False, n=17)]
BURN, KEEP, L, STEP0, SEED, TARGET = 12, 10, 3, 0.1, 99, 0.75


def _setup(shape, torch):
    from bayesgm_amd.engine import CausalEngine
    from oracle import causal as OC
    m = OC.init_model(31, shape["z_dims"], shape["p"], binary_treatment=shape["binary"])
    rs = np.random.RandomState(130)      # non-zero biases
    for k in ("g", "f", "h", "e"):
        m[k] = [(W.astype(np.float32), (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W, b in m[k]]
    eng = CausalEngine(m["v_dim"], m["z_dims"], binary_treatment=m["binary_treatment"], sigma_v=m.get("sigma_v"), sigma_x=m.get("sigma_x"),
                       sigma_y=m.get("sigma_y"))
    eng.set_model(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
    rs = np.random.RandomState(32)
    n, p = shape["n"], shape["p"]
    v = rs.randn(n, p).astype(np.float32)
    x = rs.exponential(size=(n, 1)).astype(np.float32)
    if shape["binary"]:
        x = (x > np.median(x)).astype(np.float32)
    y = (x + rs.randn(n, 1)).astype(np.float32)
    return eng, (x, y, v)


def _routes(shape):
    """{route: keyword arguments of hmc_sample}"""
    from bayesgm_amd import _lib
    n, q = shape["n"], sum(shape["z_dims"])
    scale = np.random.RandomState(23).uniform(0.3, 3.0, (n, q)).astype(np.float32)
    xv = np.linspace(0.0, 3.0, 6).astype(np.float32)
    r = dict(identity=dict(want_draws=True), metric=dict(want_draws=True, mass_scale=scale),
             window=dict(want_draws=True, mass="diag", mass_windows=(3, [9])))
    if shape["binary"]:
        r["ite"] = dict(effect=_lib.EFFECT_ITE)
        r["labels"] = dict(effect=_lib.EFFECT_GROUP_ITE, labels=(np.arange(n) % 3).astype(np.int32), n_labels=3)
    else:
        r["adrf"] = dict(effect=_lib.EFFECT_ADRF, x_values=xv)
        r["rows"] = dict(row_effects=True, row_draws=True, x_values=xv)
    for k in [k for k in r if k not in ("identity", "metric", "window")]:
        r[k + "_metric"] = dict(r[k], mass_scale=scale)
    r["partial"] = dict(want_draws=True, partial=True)
    r["partial_metric"] = dict(want_draws=True, mass_scale=scale, partial=True)
    if shape["binary"]:
        r["partial_ite"] = dict(effect=_lib.EFFECT_ITE, partial=True)
    else:
        r["partial_rows"] = dict(row_effects=True, row_draws=True, x_values=xv, partial=True)
    return r


def _unobserved(x, y):
    """y NaN in a third of the rows, x and y NaN in another third"""
    x, y = x.copy(), y.copy()
    rows = np.arange(len(x))
    y[rows % 3 != 0] = np.nan
    x[rows % 3 == 2] = np.nan
    return x, y


def _digest(res, key, value):
    """the digest of an array-like (a tensor, an array, a number) under `key`; tuples, lists of arrays and dicts item by item; None not at all"""
    if value is None:
        return
    if isinstance(value, dict):
        for k, t in sorted(value.items()):
            _digest(res, "%s/%s" % (key, k), t)
    elif isinstance(value, tuple):
        for i, t in enumerate(value):
            _digest(res, "%s/%d" % (key, i), t)
    else:
        a = np.ascontiguousarray(value.detach().cpu().numpy() if hasattr(value, "detach") else np.asarray(value))
        res[key] = hashlib.sha256(a.tobytes()).hexdigest() + " %s%s" % (a.dtype, list(a.shape))


def run():
    import torch
    if not torch.cuda.is_available():
        sys.exit("digest_causal_hmc: needs a HIP device")
    res = {}
    for s, shape in enumerate(SHAPES):
        eng, (x, y, v) = _setup(shape, torch)
        for route, kw in _routes(shape).items():
            xr, yr = _unobserved(x, y) if kw.get("partial") else (x, y)
            _digest(res, "shape%d/%s" % (s, route), eng.hmc_sample(xr, yr, v, BURN, KEEP, STEP0, L, SEED, adapt=TARGET, **kw))
    return dict(device=torch.cuda.get_device_name(0), lib=os.environ.get("BGM_HIP_LIB", ""), digests=res)


MODEL_N, MODEL_P, MODEL_BURN = 40, 20, 24      # 16-row blocks: 16 / 16 / 8; the shortest burn-in with a window of the metric is 20
ATTRS = ("hmc_row_step_", "hmc_row_mass_", "individual_sd_", "average_effects_", "last_acceptance_rate")


def _model_routes(binary, data):
    """[(route, method name, positional arguments, keyword arguments)] of one treatment type"""
    x, y, v = data
    xv = [0.0, 1.5, 3.0]
    x_new = _unobserved(x, y)[0].reshape(-1)
    one, hmc = dict(draw_budget_bytes=1), dict(sampler="hmc")
    r = [("predict_draws", "predict", (data,), dict(hmc, x_values=None if binary else xv, **one)),
         ("predict_fused", "predict", (data,), dict(hmc, x_values=None if binary else xv, fused_effects=True)),
         ("predict_draws_diag", "predict", (data,), dict(hmc, x_values=None if binary else xv, mass="diag", **one))]
    if binary:
        r += [("new_quantile", "predict_new", (v, x_new), dict(interval="quantile", **one)),
              ("average", "predict_average", (data,), dict(groups=np.arange(MODEL_N) % 3))]
    else:
        r += [("individual_normal", "predict_individual", (data, xv), {}),
              ("individual_quantile", "predict_individual", (data, xv), dict(interval="quantile", **one)),
              ("new_quantile", "predict_new", (v, x_new), dict(x_values=xv, interval="quantile", **one))]
    return r + [("hmc_sampler_diag", "hmc_sampler", (data,), dict(n_keep=KEEP, burn_in=MODEL_BURN, n_leapfrog=L, mass="diag"))]


def run_models():
    import tempfile
    import torch
    if not torch.cuda.is_available():
        sys.exit("digest_causal_hmc: needs a HIP device")
    from bayesgm_amd.models import CausalBGM
    from oracle import causal as OC
    res = {}
    for s, shape in enumerate(SHAPES[:2]):
        binary = shape["binary"]
        m = OC.init_model(31, shape["z_dims"], MODEL_P, binary_treatment=binary)
        rs = np.random.RandomState(130)      # non-zero biases
        for k in ("g", "f", "h", "e"):
            m[k] = [(W.astype(np.float32), (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W, b in m[k]]
        rs = np.random.RandomState(32)
        v = rs.randn(MODEL_N, MODEL_P).astype(np.float32)
        x = rs.exponential(size=(MODEL_N, 1)).astype(np.float32)
        if binary:
            x = (x > np.median(x)).astype(np.float32)
        y = (x + rs.randn(MODEL_N, 1)).astype(np.float32)
        params = dict(dataset="digest", output_dir=tempfile.mkdtemp(), save_res=False, save_model=False, binary_treatment=binary,
                      use_bnn=False, z_dims=shape["z_dims"], v_dim=MODEL_P, mixing_check=False)
        model = CausalBGM(params, random_seed=7)
        model.set_weights(g=m["g"], f=m["f"], h=m["h"], e=m["e"])
        for route, method, args, kw in _model_routes(binary, (x, y, v)):
            if method != "hmc_sampler":
                kw = dict(kw, n_mcmc=KEEP, burn_in=MODEL_BURN, n_leapfrog=L, verbose=0)
            key = "model%d/%s" % (s, route)
            _digest(res, key + "/returned", getattr(model, method)(*args, **kw))
            for name in ATTRS:
                _digest(res, key + "/" + name, getattr(model, name, None))
    return dict(device=torch.cuda.get_device_name(0), lib=os.environ.get("BGM_HIP_LIB", ""), digests=res)


def compare(first, second, other):
    a, b, c = (json.load(open(f))["digests"] for f in (first, second, other))
    unstable = sorted(k for k in a if a[k] != b.get(k))
    differ = sorted(k for k in a if k not in unstable and a[k] != c.get(k))
    missing = sorted(set(a) ^ set(c))
    print("%d tensors; %d differ between the two runs of the first build (left out): %s" % (len(a), len(unstable), unstable))
    print("%d of the remaining %d differ in the other build: %s; in one only: %s" % (len(differ), len(a) - len(unstable), differ, missing))
    return 1 if differ or missing else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", action="store_true", help="hash what the CausalBGM class returns, not the engine's hmc_sample")
    ap.add_argument("--compare", nargs=3, metavar=("FIRST", "SECOND", "OTHER"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    line = json.dumps(run_models() if a.models else run())
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
