#!/usr/bin/env python3
"""Measurements of BGM's HMC with a number of leapfrog steps per chain (csrc/bgm_rowstep_kernels.h, bgm_hmc_rows_traj_kernel) on one GPU.

  --part cost     the three calls of the BGM HMC transition (csrc/bgm_kernels.h, bgm_rowstep_kernels.h) -- the scalar step (hmc_run), the per-chain step with the option
                  off, and the kernel with cap and jitter on -- in THIS build against the same calls in another build of the library
                  (--parent-lib, the parent commit's libbgm_hip.so), both loaded into one process and alternated after a warm-up, HIP
                  events: N rows, L leapfrog steps, p = 500 in fp32 and f16x3 and p = 100; --families: one shape per compiled family.
                  Per call: the repeats, median and max - min of each build, this / parent, and whether this build's median is
                  within the parent's median plus the parent's own spread.  And this build's kernel with cap and jitter on against
                  its own option-off call (every transition still costs L evaluations).
  --part mixing   the panel of probe_bgm_row_step.py --part mixing (rows at 0 %, 20 % and 90 % missing cells, in thirds) with per-chain
                  steps under {no cap, T = pi/2, T = pi, jitter only, T = pi + jitter}; by group: acceptance, step quantiles, mean L_i,
                  ESS median and 1 % quantile, the share of series with split R-hat > 1.01.

    python -m bayesgm_amd.csrc.build --force -o PARENT/libbgm_hip.so          (at the parent commit)
    timeout -k 10 500 python scripts/probe_bgm_trajectory.py --parent-lib PARENT/libbgm_hip.so --out profiles/bgm_trajectory_probe.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from probe_bgm_row_step import _engine, _panel, _timed  # noqa: E402


def _engine_of(lib_path, p, prec, nh=5):
    """an engine whose handle and calls belong to the library at lib_path (None: the package's own)"""
    if lib_path is None:
        return _engine(p, prec, nh=nh)
    from bayesgm_amd import _lib
    own = _lib.load()
    other = C.CDLL(os.path.abspath(lib_path))
    for name, (res, args) in _lib.SYMBOLS.items():
        if hasattr(other, name):      # (an older build lacks the newer entry points)
            fn = getattr(other, name)
            fn.restype, fn.argtypes = res, args
    _lib._lib = other
    try:
        return _engine(p, prec, nh=nh)
    finally:
        _lib._lib = own


SHAPES = ((500, "fp32", 5), (500, "f16x3", 5), (100, "fp32", 5))
# --families: with SHAPES, one shape per compiled family of the BGM HMC kernels (NTX 2 / 7 / 0, split precision with p % 4 == 0 and != 0, NH 5 / 3)
MORE_SHAPES = ((20, "fp32", 5), (61, "f16x3", 5), (500, "fp32", 3), (500, "f16x3", 3), (100, "fp32", 3), (20, "fp32", 3), (61, "f16x3", 3))


def part_cost(a):
    import torch
    out = dict(part="cost", device=torch.cuda.get_device_name(0), n=a.n, n_leapfrog=a.leapfrog, transitions=a.transitions,
               parent_lib=bool(a.parent_lib), cases=[])
    for p, prec, nh in SHAPES + (MORE_SHAPES if a.families else ()):
        engines = dict(this=_engine_of(None, p, prec, nh))
        if a.parent_lib:
            engines["parent"] = _engine_of(a.parent_lib, p, prec, nh)
        dev = engines["this"].device
        x = torch.from_numpy(_panel(a.n, p, [0.2])[0]).to(dev)
        state, grad = (torch.empty((a.n, 10), device=dev) for _ in range(2))
        logp = torch.empty(a.n, device=dev)
        one, rows = torch.full((1,), 0.02, device=dev), torch.full((a.n,), 0.02, device=dev)
        # the three calls, each in every build.  0.02 x 10 steps = 0.2: T = 0.1 gives L_i = 5, the jitter 1 .. 5
        def calls(e):
            return dict(scalar=lambda: e.hmc_run(x, state, logp, grad, one, 0, a.transitions, 0, a.leapfrog, 7, init=True),
                        rows=lambda: e.hmc_run_rows(x, state, logp, grad, rows, 0, a.transitions, 0, a.leapfrog, 7, init=True),
                        traj=lambda: e.hmc_run_rows(x, state, logp, grad, rows, 0, a.transitions, 0, a.leapfrog, 7, init=True,
                                                    max_trajectory=0.1, jitter=True))
        fns = {k: calls(e) for k, e in engines.items()}
        run = {(call, k): fns[k][call] for call in ("scalar", "rows", "traj") for k in sorted(engines)}      # (parent, this, parent, ...)
        for f in run.values():
            f()
        ms = {k: [] for k in run}
        for _ in range(a.reps):
            for k, f in run.items():
                ms[k].append(_timed(torch, f) / a.transitions)
        r = dict(p=p, precision=prec, n_hidden=nh, calls={})
        for call in ("scalar", "rows", "traj"):
            c = {k: dict(ms_per_transition=ms[call, k], median=float(np.median(ms[call, k])), spread=max(ms[call, k]) - min(ms[call, k]))
                 for k in engines}
            if a.parent_lib:      # "no slower": this build's median within the parent's median plus the parent's own max - min
                c["this_over_parent"] = c["this"]["median"] / c["parent"]["median"]
                c["within_parent_spread"] = bool(c["this"]["median"] <= c["parent"]["median"] + c["parent"]["spread"])
            r["calls"][call] = c
        r["traj_over_off"] = r["calls"]["traj"]["this"]["median"] / r["calls"]["rows"]["this"]["median"]
        print(json.dumps(r), file=sys.stderr, flush=True)
        out["cases"].append(r)
        for e in engines.values():
            e.close()
    return out


def part_mixing(a):
    import torch
    from bayesgm_amd.diagnostics import chain_diagnostics
    p, shares = a.p, [0.0, 0.2, 0.9]
    eng = _engine(p, "fp32")
    x, group = _panel(a.mixing_n, p, shares)
    xd = torch.from_numpy(x).to(eng.device)
    out = dict(part="mixing", device=torch.cuda.get_device_name(0), n=a.mixing_n, p=p, missing_shares=shares, burn_in=a.burn_in, n_mcmc=a.n_mcmc,
               n_leapfrog=a.leapfrog, start_step=0.02, target=0.75)
    settings = (("no_cap", {}), ("cap_half_pi", dict(max_trajectory=np.pi / 2)), ("cap_pi", dict(max_trajectory=np.pi)),
                ("jitter", dict(jitter=True)), ("cap_pi_jitter", dict(max_trajectory=np.pi, jitter=True)))
    for name, opt in settings:
        res = eng.hmc_sample(xd, a.n_mcmc, a.burn_in, 0.02, a.leapfrog, 7, row_adapt=0.75, **opt)
        d = chain_diagnostics(res["draws"])
        steps = res["row_step"].cpu().numpy()
        li = res["n_steps"].cpu().numpy() / float(a.n_mcmc) if "n_steps" in res else np.full(a.mixing_n, float(a.leapfrog))
        acc = float(res["acc_count"][a.burn_in:].sum().item()) / (a.n_mcmc * a.mixing_n)
        moved = d.moves[:, 0] / max(1, a.n_mcmc - 1)          # a move changes every coordinate: the acceptance frequency of the row
        r = dict(retained_acceptance=acc)
        for k, s in enumerate(shares):
            g = group == k
            ess, rhat = d.ess[g].reshape(-1), d.rhat[g].reshape(-1)
            ok = np.isfinite(ess) & np.isfinite(rhat)
            r["missing_%d" % round(100 * s)] = dict(acceptance=float(moved[g].mean()), step_quantiles_05_50_95=[float(t) for t in np.quantile(steps[g], [0.05, 0.5, 0.95])],
                                                   mean_leapfrog=float(li[g].mean()), ess_median=float(np.median(ess[ok])),
                                                   ess_q01=float(np.quantile(ess[ok], 0.01)), share_rhat_above_1_01=float(np.mean(rhat[ok] > 1.01)))
        out[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del res, d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("all", "cost", "mixing"), default="all")
    ap.add_argument("--parent-lib", default=None, help="libbgm_hip.so of the parent commit (cost part)")
    ap.add_argument("--families", action="store_true", help="cost part: the other compiled kernel families after the three default shapes")
    ap.add_argument("--n", type=int, default=200000, help="rows of the cost part")
    ap.add_argument("--mixing-n", type=int, default=6000)
    ap.add_argument("--p", type=int, default=100, help="x_dim of the mixing part")
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--n-mcmc", type=int, default=1000)
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--leapfrog", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for part, fn in (("cost", part_cost), ("mixing", part_mixing)):
        if a.part in ("all", part):
            res[part] = fn(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
