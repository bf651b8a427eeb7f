#!/usr/bin/env python3
"""Development aid: SHA-256 of what the four EGM warm-start sessions read back (losses, gradients, trained parameters), to show that two
builds of libbgm_hip.so compute the same bytes on one GPU (the companion of compare_code_objects.py for a change of the sessions' host
side; see digest_bnn_sampling.py for the sampling calls).

    BGM_HIP_LIB=A/libbgm_hip.so timeout -k 10 600 python scripts/digest_egm_sessions.py --out a.json
    BGM_HIP_LIB=A/libbgm_hip.so timeout -k 10 600 python scripts/digest_egm_sessions.py --out a_again.json
    BGM_HIP_LIB=B/libbgm_hip.so timeout -k 10 600 python scripts/digest_egm_sessions.py --out b.json
    python scripts/digest_egm_sessions.py --compare a.json a_again.json b.json

One process per library.  The shapes and inputs are the tests' own (their builders are imported from tests/):
  causal/<case>   every case of tests/_egm_edges_ref.py CASES (all seven discriminator and seven generator routes): one discriminator and
                  one generator step with apply = 0 (losses, both gradients), then the alternating Adam rounds (both parameter sets)
  bnn/...         the Bayesian session at the shapes of test_egm_steps_match_oracle and test_egm_split_step_equals_fused_step of
                  tests/test_gpu_bnn.py: the same, and the split form (step with apply = 0, bgm_bnn_egm_grad, bgm_bnn_egm_apply)
  bgm/..., bvn/.. the two BGM sessions at the shapes of tests/test_gpu_egm.py and tests/test_gpu_bgm_bnn.py: a step pair with apply = 0,
                  four alternating iterations, the encoder over the panel, write / read of the discriminators
--compare FIRST SECOND OTHER: as digest_bnn_sampling.py -- tensors that differ between two runs of one build are named and left out,
every other digest of OTHER must equal FIRST's.  Exit status 1 otherwise."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _put(res, key, a):
    import torch
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    res[key] = hashlib.sha256(a.tobytes()).hexdigest() + " %s%s" % (a.dtype, list(a.shape))


def causal(res):
    import torch
    import _egm_edges_ref as E
    import test_gpu_egm_edges as T
    for c in E.CASES:
        pre = "causal/" + c["name"]
        g = T._grads(c, False)
        for k in ("d_losses", "g_losses", "d_grads", "g_grads"):
            _put(res, "%s/%s" % (pre, k), g[k])
        t = T._train(c, False)
        for k in ("theta_g", "theta_d", "g_first"):
            _put(res, "%s/trained/%s" % (pre, k), t[k])
        if c["split"]:
            t = T._train(c, False, split=True)
            _put(res, pre + "/split/theta_g", t["theta_g"])
            _put(res, pre + "/split/theta_d", t["theta_d"])
    torch.cuda.synchronize()


BNN_SHAPES = [   # binary, discriminator normalisation, p, z_dims, B, the nets' inference-mode normalisation
    (False, "batch", 50, (1, 1, 1, 7), 32, False), (True, "fixed", 50, (1, 1, 1, 7), 32, False), (False, "fixed", 100, (1, 1, 1, 7), 32, True),
    (True, "fixed", 200, (1, 1, 1, 7), 32, True), (False, "fixed", 45, (1, 1, 1, 7), 32, True), (True, "fixed", 177, (3, 6, 3, 6), 32, True),
    (False, "fixed", 100, (5, 5, 5, 5), 32, True), (False, "fixed", 50, (5, 5, 5, 5), 32, False), (False, "fixed", 100, (1, 1, 1, 7), 16, True),
    (False, "fixed", 200, (1, 1, 1, 7), 16, True), (False, "fixed", 210, (1, 1, 1, 7), 16, True), (False, "fixed", 50, (1, 1, 1, 7), 4, True)]


def bnn(res):
    import torch
    import test_gpu_bnn as T
    from oracle import egm as OE
    for binary, disc_norm, p, zd, B, fixed in BNN_SHAPES:
        for split in (False, True):
            pre = "bnn/p%d-q%d-B%d-%s%s%s/%s" % (p, sum(zd), B, disc_norm, "-binary" if binary else "", "-fixednets" if fixed else "", "split" if split else "fused")
            m = T._model(binary, z_dims=zd, p=p)
            n, q = 120, sum(zd)
            _, x, y, v = T._panel(m, n)
            rs = np.random.RandomState(33)
            dz = OE.init_disc(rs, q, [64, 32, 8])
            if fixed:
                for k in ("g", "e", "f", "h"):
                    m[k]["norm"] = "fixed"
            eng = T._engine(m, norm_mode=1) if fixed else T._engine(m)
            dev = eng.device
            D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            if disc_norm == "fixed":
                eng.set_disc_norm("fixed")
                dz["fixed_norm"] = True
            eng.egm_begin(dz, B, 2e-4, 1)
            n_gen, n_dz = eng.egm_sizes()
            bg, bd = torch.empty(n_gen, device=dev), torch.empty(n_dz, device=dev)
            seed, stream = (1 << 32) | 7, 500
            batch = lambda: (D(rs.standard_normal((B, q)).astype(np.float32)), D(rs.choice(n, B, replace=False).astype(np.int32)))
            if not split:      # one step pair with apply = 0: losses and gradients
                z, idx = batch()
                out_d, out_g = torch.zeros(2, device=dev), torch.zeros(6, device=dev)
                eng.egm_disc_step(z, idx, D(v), 0.37, seed, 1000, apply=False, out=out_d)
                _put(res, pre + "/d_losses", out_d)
                _put(res, pre + "/d_grads", eng.egm_read(3))
                eng.egm_gen_step(z, idx, D(v), D(x[:, 0]), D(y[:, 0]), seed, 1016, apply=False, out=out_g)
                _put(res, pre + "/g_losses", out_g)
                _put(res, pre + "/g_grads", eng.read(1))
            for it in range(3):
                for _ in range(2):
                    z, idx = batch()
                    eng.egm_disc_step(z, idx, D(v), float(rs.rand()), seed, stream, apply=not split)
                    stream += 1
                    if split:
                        eng.egm_grad(1, 1.0, bd)
                        eng.egm_apply(1, bd)
                z, idx = batch()
                eng.egm_gen_step(z, idx, D(v), D(x[:, 0]), D(y[:, 0]), seed, stream, apply=not split)
                stream += 9
                if split:
                    eng.egm_grad(0, 1.0, bg)
                    eng.egm_apply(0, bg)
            _put(res, pre + "/trained/theta", eng.read(0))
            _put(res, pre + "/trained/theta_d", eng.egm_read(1))
            eng.egm_end()
            eng.close()


def _bgm_session(res, pre, eng, x, rs, p, q, B, extra):
    """extra(s): the (seed, stream) arguments the Bayesian generator's steps take between the inputs and apply"""
    import torch
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    draw = lambda: (D(rs.randn(B, q).astype(np.float32)), D(x[rs.choice(len(x), B, replace=False)]), D(rs.randn(B, p).astype(np.float32)),
                    D(rs.randn(B, p).astype(np.float32)))
    z, xb, n1, n2 = draw()
    out_d, out_g = torch.zeros(3, device="cuda"), torch.zeros(6, device="cuda")
    eng.egm_disc_step(z, xb, n1, 0.31, 0.64, *extra(4), apply=False, out=out_d)
    _put(res, pre + "/d_losses", out_d)
    _put(res, pre + "/d_grads", eng.egm_read(3))
    eng.egm_gen_step(z, xb, n1, n2, *extra(6), apply=False, out=out_g)
    _put(res, pre + "/g_losses", out_g)
    _put(res, pre + "/g_grads", eng.egm_read(2))
    for s in range(4):
        z, xb, n1, n2 = draw()
        eng.egm_disc_step(z, xb, n1, float(rs.rand()), float(rs.rand()), *extra(20 + 4 * s))
        z, xb, n1, n2 = draw()
        eng.egm_gen_step(z, xb, n1, n2, *extra(22 + 4 * s))
    _put(res, pre + "/trained/theta_g", eng.egm_read(0))
    _put(res, pre + "/trained/theta_d", eng.egm_read(1))
    _put(res, pre + "/encode", eng.egm_encode(x))
    td = eng.egm_read(1)
    eng.egm_write(1, td[::-1])
    _put(res, pre + "/written/theta_d", eng.egm_read(1))
    eng.egm_write(1, td)


def bgm(res):
    import test_gpu_egm as TE
    import test_gpu_bgm_bnn as TV
    for case in (dict(p=20, gamma=0.0, alpha=0.0, B=32), dict(p=100, gamma=0.7, alpha=0.3, B=32), dict(p=37, gamma=1.0, alpha=0.0, B=19),
                 dict(p=20, gamma=0.5, alpha=0.2, B=32)):
        p, B = case["p"], case["B"]
        eng, g, e, dz, dx, x, rs = TE._bgm_setup(p, 10, B, gamma=case["gamma"], alpha=case["alpha"])
        pre = "bgm/p%d-B%d-gamma%g-alpha%g" % (p, B, case["gamma"], case["alpha"])
        _bgm_session(res, pre, eng, x, rs, p, 10, B, lambda s: ())
        eng.egm_end()
        _put(res, pre + "/installed", eng.get_weights()["trunk"][0][0])
    for case in (dict(p=20, B=32, gamma=0.0, alpha=0.0, seed=0), dict(p=37, B=19, gamma=0.5, alpha=0.2, seed=0), dict(p=20, B=32, gamma=0.5, alpha=0.2, seed=3)):
        p, B = case["p"], case["B"]
        eng, _, x, rs = TV._egm_setup(p, 10, B, gamma=case["gamma"], alpha=case["alpha"], seed=case["seed"])
        pre = "bvn/p%d-B%d-gamma%g-alpha%g-seed%d" % (p, B, case["gamma"], case["alpha"], case["seed"])
        _bgm_session(res, pre, eng, x, rs, p, 10, B, lambda s: (555, s))
        eng.egm_end()
        _put(res, pre + "/installed", eng.read(0))
        eng.close()


def run():
    import torch
    if not torch.cuda.is_available():
        sys.exit("digest_egm_sessions: needs a HIP device")
    res = {}
    causal(res)
    bnn(res)
    bgm(res)
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
    ap.add_argument("--compare", nargs=3, metavar=("FIRST", "SECOND", "OTHER"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    out = run()
    print(json.dumps(dict(device=out["device"], lib=out["lib"], tensors=len(out["digests"]))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=0, sort_keys=True) + "\n")
