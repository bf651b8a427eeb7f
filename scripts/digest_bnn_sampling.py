#!/usr/bin/env python3
"""Development aid: SHA-256 of everything the Bayesian CausalBGM sampling calls return (bgm_bnn_logpost / _mh_run / _effects /
_evaluate under bgm_bnn_set_precision and bgm_bnn_set_prior), to show that two builds of libbgm_hip.so compute the same bytes on one
GPU (the companion of compare_code_objects.py for a change of the host side).

    BGM_HIP_LIB=A/libbgm_hip.so timeout -k 10 300 python scripts/digest_bnn_sampling.py --out a.json
    BGM_HIP_LIB=B/libbgm_hip.so timeout -k 10 300 python scripts/digest_bnn_sampling.py --out b.json
    python scripts/digest_bnn_sampling.py --compare a.json a_again.json b.json

One process per library.  Sessions: the smallest at which each kernel family takes each of its paths, n = 40 rows in blocks of 24 (a
short last block), block0 = 3 --
  bnf   z_dims (1,1,1,7), p = 50, continuous and (3,3,6,6), p = 20, binary, inference-mode normalisation; in fp32 and in f16x3
  bns   the same two with batch statistics; (1,1,1,7), p = 3 with inference-mode normalisation (outside bnf's table)
  bnw   g_units [128, 96] with both normalisations
Per session: logpost; mh_run over 6 iterations (burn-in 3, keep 3) as two calls (4 + 2 iterations, the second with it_begin > 0) with
draws, a per-block proposal scale, acceptance counts per call and per (iteration, block), and the ADRF on 5 doses (continuous) or the
ITE (binary); effects on those draws with and without outcome noise; evaluate with encode, sums and the dose grid / the ITE (bnf has
none: the session's second family serves it).  On bnf also a share of one block (block_row0 = 5) and effects on 257 doses (served by
the second family); in one session per family the conditional prior (bgm_bnn_set_prior): logpost and two iterations.
--compare FIRST SECOND OTHER: tensors whose digests differ between FIRST and SECOND (two runs of one build) are named and left out;
only sums accumulated with floating-point atomics (ADRF sums, evaluate's sums) may be among them, and for each the largest relative
difference OTHER - FIRST is printed next to SECOND - FIRST.  Every other digest of OTHER must equal FIRST's.  Exit status 1 otherwise.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N, BS, BLOCK0, ROW_BASE, BURN, KEEP, SEED = 40, 24, 3, 72, 3, 3, (2 << 32) | 555
WIDE = dict(g_units=[128, 96])
SESSIONS = [   # name, z_dims, p, binary, inference-mode normalisation, units, precisions, with the conditional prior too
    ("bnf-cont", (1, 1, 1, 7), 50, False, True, {}, ("fp32", "f16x3"), True),
    ("bnf-bin", (3, 3, 6, 6), 20, True, True, {}, ("fp32", "f16x3"), False),
    ("bns-cont", (1, 1, 1, 7), 50, False, False, {}, ("fp32",), True),
    ("bns-bin", (3, 3, 6, 6), 20, True, False, {}, ("fp32",), False),
    ("bns-p3", (1, 1, 1, 7), 3, False, True, {}, ("fp32",), False),
    ("bnw-fixed", (1, 1, 1, 7), 20, False, True, WIDE, ("fp32",), True),
    ("bnw-batch", (1, 1, 1, 7), 20, False, False, WIDE, ("fp32",), False),
]
ATOMIC = ("adrf", "sums", "dose")      # last path component of the tensors accumulated with floating-point atomics


def _model(z_dims, p, binary, fixed, units):
    from oracle import bnn as OB
    m = OB.init_model(0, list(z_dims), p, binary, **units)
    rs = np.random.RandomState(11)
    for k in ("g", "e", "f", "h"):
        if fixed:
            m[k]["norm"] = "fixed"
        m[k]["gamma"] = (1.0 + 0.2 * rs.standard_normal(m[k]["gamma"].shape)).astype(np.float32)
        m[k]["beta"] = (0.1 * rs.standard_normal(m[k]["beta"].shape)).astype(np.float32)
    rs = np.random.RandomState(1)
    z = rs.standard_normal((N, sum(z_dims))).astype(np.float32)
    v = rs.standard_normal((N, p)).astype(np.float32)
    x = ((rs.rand(N) > 0.5) if binary else rs.exponential(size=N)).astype(np.float32)
    y = (x + rs.standard_normal(N)).astype(np.float32)
    return m, (x, y, v, z)


def _put(res, vals, key, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    res[key] = hashlib.sha256(a.tobytes()).hexdigest() + " %s%s" % (a.dtype, list(a.shape))
    if key.rsplit("/", 1)[-1] in ATOMIC:
        vals[key] = [float(f) for f in a.ravel()]


def _mh(eng, torch, data, binary, pre, res, vals, n_iters=(4, 2), rows=slice(None), block_row0=0):
    """the sampler as consecutive calls of n_iters iterations over the rows `rows` of the panel"""
    dev = eng.device
    x, y, v, z = (torch.from_numpy(np.ascontiguousarray(a[rows])).to(dev) for a in data)
    n, q = z.shape
    n_blocks = (n + BS - 1) // BS
    xs = torch.linspace(0.0, 3.0, 5, device=dev)
    state, draws = torch.zeros(n, q, device=dev), torch.zeros(KEEP, n, q, device=dev)
    adrf, ite = torch.zeros(5, KEEP, device=dev, dtype=torch.float64), torch.zeros(n, KEEP, device=dev)
    sd = torch.linspace(0.2, 0.6, n_blocks, device=dev)
    it = 0
    for c, k in enumerate(n_iters):
        acc, accb = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((k, n_blocks), dtype=torch.int32, device=dev)
        eng.mh_run(x, y, v, state, BS, it, k, BURN, 7.0, SEED, init=it == 0, row_base=ROW_BASE + block_row0, block0=BLOCK0, acc_count=acc,
                   draws=draws, n_keep=KEEP, effect=2 if binary else 1, sample_y=True, x_values=None if binary else xs,
                   adrf_sum=None if binary else adrf, ite=ite if binary else None, q_sd_blocks=sd, acc_blocks=accb, block_row0=block_row0)
        _put(res, vals, "%s/call%d/acc" % (pre, c), acc)
        _put(res, vals, "%s/call%d/acc_blocks" % (pre, c), accb)
        it += k
    _put(res, vals, pre + "/state", state)
    _put(res, vals, pre + "/draws", draws)
    _put(res, vals, pre + ("/ite" if binary else "/adrf"), ite if binary else adrf)
    return draws, xs


def _prior(eng, torch, q, fixed):
    """bgm_bnn_set_prior as tests/test_gpu_identifiable_bnn.py sets it up: 6 segments, one hidden layer of 64; returns what must stay alive"""
    from bayesgm_amd import _lib
    from bayesgm_amd.bnn_engine import flatten_bnn
    from oracle import identifiable as OI
    k = 6
    rs = np.random.RandomState(8)
    pn = OI.init_prior_bnn(rs, k, q, (64,))
    pn["gamma"] = (1.0 + 0.2 * rs.standard_normal(k)).astype(np.float32)
    pn["beta"] = (0.1 * rs.standard_normal(k)).astype(np.float32)
    if fixed:
        pn["norm"] = "fixed"
    dims = [k, 64, q + 1]
    cfg = _lib.PriorConfig(len(dims) - 1, (C.c_int32 * 5)(*(dims + [0] * (5 - len(dims)))))
    theta = torch.from_numpy(np.ascontiguousarray(flatten_bnn(pn))).to(eng.device)
    seg = torch.from_numpy(rs.randint(0, k, N).astype(np.int32)).to(eng.device)
    _lib.check(eng.lib.bgm_bnn_set_prior(eng.h, C.byref(cfg), theta.data_ptr(), seg.data_ptr()), "bgm_bnn_set_prior")
    return theta, seg


def run():
    import torch
    if not torch.cuda.is_available():
        sys.exit("digest_bnn_sampling: needs a HIP device")
    from bayesgm_amd.bnn_engine import BnnEngine
    res, vals = {}, {}
    for name, z_dims, p, binary, fixed, units, precisions, with_prior in SESSIONS:
        m, data = _model(z_dims, p, binary, fixed, units)
        for prec in precisions:
            eng = BnnEngine(p, list(z_dims), binary, kl_weight=1e-4, max_batch=32, norm_mode=1 if fixed else 0, **units)
            eng.begin(m)
            eng.set_precision(prec)
            dev, pre = eng.device, "%s/%s" % (name, prec)
            x, y, v, z = (torch.from_numpy(a).to(dev) for a in data)
            lp = lambda: eng.logpost(x, y, v, z, BS, SEED, 77, block0=BLOCK0)
            _put(res, vals, pre + "/logpost", lp())
            draws, xs = _mh(eng, torch, data, binary, pre + "/mh", res, vals)
            for noise in (True, False):
                out = eng.effects(draws, BS, SEED, it0=BURN, x_values=None if binary else xs.cpu().numpy(), sample_y=noise, row_base=ROW_BASE, block0=BLOCK0)
                _put(res, vals, "%s/effects-noise%d/%s" % (pre, noise, "ite" if binary else "adrf"), out)
            ze, sums, causal = eng.evaluate(x, y, v, None, x_values=None if binary else xs.cpu().numpy(), seed=SEED, stream_id=5)
            _put(res, vals, pre + "/evaluate/z", ze)
            _put(res, vals, pre + "/evaluate/sums", sums)
            _put(res, vals, pre + "/evaluate/" + ("ite" if binary else "dose"), causal)
            if name.startswith("bnf"):
                _mh(eng, torch, data, binary, pre + "/share", res, vals, n_iters=(5,), rows=slice(5, 15), block_row0=5)
                if not binary:
                    out = eng.effects(draws[:1], BS, SEED, it0=BURN, x_values=np.linspace(0.0, 3.0, 257).astype(np.float32), row_base=ROW_BASE, block0=BLOCK0)
                    _put(res, vals, pre + "/effects-257/adrf", out)
            if with_prior:
                keep_alive = _prior(eng, torch, sum(z_dims), fixed)
                _put(res, vals, pre + "/prior/logpost", lp())
                _mh(eng, torch, data, binary, pre + "/prior/mh", res, vals)
                del keep_alive
            eng.close()
    return dict(device=torch.cuda.get_device_name(0), lib=os.environ.get("BGM_HIP_LIB", ""), digests=res, values=vals)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-300))


def compare(first, second, other):
    A, B, Cc = (json.load(open(f)) for f in (first, second, other))
    a, b, c = A["digests"], B["digests"], Cc["digests"]
    unstable = sorted(k for k in a if a[k] != b.get(k))
    barred = [k for k in unstable if k not in A["values"]]
    differ = sorted(k for k in a if k not in unstable and a[k] != c.get(k))
    missing = sorted(set(a) ^ set(c))
    print("%d tensors; %d differ between the two runs of the first build (left out): %s" % (len(a), len(unstable), unstable))
    for k in unstable:
        if k in A["values"] and k in Cc["values"]:
            print("    %s: largest relative difference, other build %.3e, second run of the first build %.3e"
                  % (k, _rel(A["values"][k], Cc["values"][k]), _rel(A["values"][k], B["values"][k])))
    if barred:
        print("NOT sums of floating-point atomics, yet different between two runs of one build: %s" % barred)
    print("%d of the remaining %d differ in the other build: %s; in one only: %s" % (len(differ), len(a) - len(unstable), differ, missing))
    return 1 if differ or missing or barred else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=3, metavar=("FIRST", "SECOND", "OTHER"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    out = run()
    print(json.dumps(dict(out, values="%d tensors" % len(out["values"]))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
