#!/usr/bin/env python3
"""Development aid: SHA-256 of everything the BGM HMC kernels return, to show that two builds of libbgm_hip.so compute the same bytes
on one GPU (the companion of compare_code_objects.py for kernels whose code objects differ; digest_causal_hmc.py's protocol).

    BGM_HIP_LIB=A/libbgm_hip.so timeout -k 10 300 python scripts/digest_bgm_hmc.py --out a.json
    BGM_HIP_LIB=B/libbgm_hip.so timeout -k 10 300 python scripts/digest_bgm_hmc.py --out b.json
    python scripts/digest_bgm_hmc.py --compare a.json a_again.json b.json

One process per library.  One shape per compiled family of the BGM HMC kernels (csrc/bgm_kernels.h: resident with 2 and 7 head tiles and
streamed, 5 and 3 hidden layers, fp32 and split precision with x_dim % 4 == 0 and != 0), n = 1 .. 50, burn-in 6, 4 retained draws,
n_leapfrog = 3, over the three step rules: hmc_sample with the shared rule (bgm_hmc_kernel, one launch and one adapt kernel per
adapting transition); hmc_run_rows with the table (bgm_hmc_rows_kernel); hmc_run_rows with max_trajectory, jitter and n_steps
(bgm_hmc_rows_traj_kernel), in one launch and cut at iteration 5.
--compare FIRST SECOND OTHER: tensors whose digests differ between FIRST and SECOND (two runs of one build; acc_prob is a sum of
doubles by atomicAdd) are named and left out; every other digest of OTHER must equal FIRST's.  Exit status 1 otherwise.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from digest_causal_hmc import _digest, compare  # noqa: E402

SHAPES = [dict(p=20, n=50, nh=5, prec="fp32"), dict(p=100, n=50, nh=5, prec="fp32"), dict(p=61, n=50, nh=5, prec="fp32"),
          dict(p=500, n=50, nh=5, prec="fp32"), dict(p=20, n=17, nh=3, prec="fp32", q=3), dict(p=100, n=1, nh=3, prec="fp32"),
          dict(p=61, n=50, nh=5, prec="f16x3"), dict(p=500, n=50, nh=5, prec="f16x3"), dict(p=40, n=33, nh=3, prec="f16x3"),
          dict(p=61, n=33, nh=3, prec="fp32"), dict(p=61, n=33, nh=3, prec="f16x3")]
BURN, KEEP, L, STEP0, SEED, TARGET, MAX_TRAJ, CUT = 6, 4, 3, 0.02, 99, 0.75, 0.03, 5


def _setup(shape, torch):
    from bayesgm_amd.engine import BgmEngine
    from oracle import bgm as OB
    q, p, n = shape.get("q", 10), shape["p"], shape["n"]
    m = OB.init_model(11, q, p, g_units=(64,) * shape["nh"])
    rs = np.random.RandomState(18)      # non-zero biases
    g = m["g"]
    g["trunk"] = [(W, (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W, b in g["trunk"]]
    g["mean"] = (g["mean"][0], (0.1 * rs.randn(p)).astype(np.float32))
    g["var"] = (g["var"][0], (0.1 * rs.randn(p)).astype(np.float32))
    eng = BgmEngine(p, q, g_units=[64] * shape["nh"])
    eng.set_weights(g)
    eng.set_precision(shape["prec"])
    rs = np.random.RandomState(12)
    x = rs.randn(n, p).astype(np.float32)
    x[rs.rand(n, p) < 0.2] = np.nan
    x[0, :] = np.nan      # a row with nothing observed
    return eng, torch.from_numpy(x).to(eng.device)


def _traj(eng, x, torch, cuts):
    """hmc_run_rows with the table, a cap, the jitter and the step counts, over launches cut at `cuts`"""
    dev, n, total = eng.device, x.shape[0], BURN + KEEP
    r = dict(state=torch.empty((n, eng.q), device=dev), grad=torch.empty((n, eng.q), device=dev), logp=torch.empty(n, device=dev),
             step=torch.full((n,), STEP0, device=dev), acc_prob=torch.zeros(total, device=dev, dtype=torch.float64),
             acc_count=torch.zeros(total, device=dev, dtype=torch.int32), draws=torch.empty((KEEP, n, eng.q), device=dev),
             n_steps=torch.zeros(n, device=dev, dtype=torch.int32))
    up, dn = eng.row_step_table(BURN, TARGET)
    marks = [0] + list(cuts) + [total]
    for a, b in zip(marks[:-1], marks[1:]):
        eng.hmc_run_rows(x, r["state"], r["logp"], r["grad"], r["step"], a, b - a, BURN, L, SEED, init=(a == 0), up=up, dn=dn,
                         acc_prob=r["acc_prob"], acc_count=r["acc_count"], draws=r["draws"], max_trajectory=MAX_TRAJ, jitter=True,
                         n_steps=r["n_steps"])
    return r


def run():
    import torch
    if not torch.cuda.is_available():
        sys.exit("digest_bgm_hmc: needs a HIP device")
    res = {}
    for s, shape in enumerate(SHAPES):
        eng, x = _setup(shape, torch)
        key = "shape%d_p%d_n%d_nh%d_%s" % (s, shape["p"], shape["n"], shape["nh"], shape["prec"])
        _digest(res, key + "/shared", eng.hmc_sample(x, KEEP, BURN, STEP0, L, SEED))
        _digest(res, key + "/rows", eng.hmc_sample(x, KEEP, BURN, STEP0, L, SEED, row_adapt=TARGET))
        _digest(res, key + "/traj", _traj(eng, x, torch, ()))
        _digest(res, key + "/traj_cut", _traj(eng, x, torch, (CUT,)))
        eng.close()
    return dict(device=torch.cuda.get_device_name(0), lib=os.environ.get("BGM_HIP_LIB", ""), digests=res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=3, metavar=("FIRST", "SECOND", "OTHER"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    line = json.dumps(run())
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
