#!/usr/bin/env python3
"""Measurements of BGM's HMC with a step size per chain (csrc/bgm_rowstep_kernels.h) on one GPU.

  --part cost     the per-chain kernel on frozen equal steps against the scalar-step kernel, alternated in one process, HIP events
                  after a warm-up: N rows, p = 500 in fp32 and f16x3 and p = 100 (a resident family), L leapfrog steps.
  --part burnin   hmc_sample with the shared rule (one launch plus one adapt kernel per adapting transition) against the per-chain
                  rule (one launch), N rows, p = 500, --burn-in + --n-mcmc transitions, wall time without the draws.
  --part mixing   a panel with rows at 0 %, 20 % and 90 % missing cells, in thirds: shared rule against per-chain steps; by group:
                  acceptance, the final step(s), ESS median and 1 % quantile, the share of series with split R-hat > 1.01.

    timeout -k 10 400 python scripts/probe_bgm_row_step.py --out profiles/bgm_row_step_probe.json      (all three parts)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _engine(p, prec, q=10, nh=5):
    from bayesgm_amd.engine import BgmEngine
    from oracle import bgm as OB
    m = OB.init_model(11, q, p, g_units=(64,) * nh)
    eng = BgmEngine(p, q, g_units=[64] * nh)
    eng.set_weights(m["g"])
    eng.set_precision(prec)
    return eng


def _panel(n, p, shares, seed=12):
    """float32 [n, p] of N(0, 1) cells; rows in len(shares) equal groups, group k with shares[k] of its cells missing (NaN)"""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, p).astype(np.float32)
    group = np.minimum(np.arange(n) * len(shares) // n, len(shares) - 1)
    x[rs.rand(n, p) < np.asarray(shares)[group][:, None]] = np.nan
    return x, group


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def part_cost(a):
    import torch
    out = dict(part="cost", device=torch.cuda.get_device_name(0), n=a.n, n_leapfrog=a.leapfrog, transitions=a.transitions, cases=[])
    for p, prec in ((500, "fp32"), (500, "f16x3"), (100, "fp32")):
        eng = _engine(p, prec)
        dev = eng.device
        x = torch.from_numpy(_panel(a.n, p, [0.2])[0]).to(dev)
        state, grad = (torch.empty((a.n, eng.q), device=dev) for _ in range(2))
        logp = torch.empty(a.n, device=dev)
        one, rows = torch.full((1,), 0.02, device=dev), torch.full((a.n,), 0.02, device=dev)
        run = dict(scalar=lambda: eng.hmc_run(x, state, logp, grad, one, 0, a.transitions, 0, a.leapfrog, 7, init=True),
                   rows=lambda: eng.hmc_run_rows(x, state, logp, grad, rows, 0, a.transitions, 0, a.leapfrog, 7, init=True))
        for f in run.values():
            f()
        ms = dict(scalar=[], rows=[])
        for _ in range(a.reps):
            for k, f in run.items():
                ms[k].append(_timed(torch, f) / a.transitions)
        r = dict(p=p, precision=prec, scalar_ms_per_transition=float(np.median(ms["scalar"])), rows_ms_per_transition=float(np.median(ms["rows"])),
                 all_ms=ms)
        r["rows_over_scalar"] = r["rows_ms_per_transition"] / r["scalar_ms_per_transition"]
        print(json.dumps(r), file=sys.stderr, flush=True)
        out["cases"].append(r)
    return out


def part_burnin(a):
    import torch
    p = 500
    out = dict(part="burnin", device=torch.cuda.get_device_name(0), n=a.n, p=p, burn_in=a.burn_in, n_mcmc=a.n_mcmc, n_leapfrog=a.leapfrog, cases=[])
    for prec in ("fp32", "f16x3"):
        eng = _engine(p, prec)
        x = torch.from_numpy(_panel(a.n, p, [0.2])[0]).to(eng.device)
        eng.hmc_sample(x, 1, 1, 0.02, 1, 7, want_draws=False)
        eng.hmc_sample(x, 1, 1, 0.02, 1, 7, want_draws=False, row_adapt=0.75)
        r = dict(precision=prec)
        for name, opt in (("shared", None), ("rows", 0.75)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = eng.hmc_sample(x, a.n_mcmc, a.burn_in, 0.02, a.leapfrog, 7, want_draws=False, row_adapt=opt)
            torch.cuda.synchronize()
            r[name + "_seconds"] = time.perf_counter() - t0
            r[name + "_retained_acceptance"] = float(res["acc_count"][a.burn_in:].sum().item()) / max(1, a.n_mcmc * a.n)
        r["rows_over_shared"] = r["rows_seconds"] / r["shared_seconds"]
        print(json.dumps(r), file=sys.stderr, flush=True)
        out["cases"].append(r)
    return out


def part_mixing(a):
    import torch
    from bayesgm_amd.diagnostics import chain_diagnostics
    p, shares = a.p, [0.0, 0.2, 0.9]
    eng = _engine(p, "fp32")
    x, group = _panel(a.n, p, shares)
    out = dict(part="mixing", device=torch.cuda.get_device_name(0), n=a.n, p=p, missing_shares=shares, burn_in=a.burn_in, n_mcmc=a.n_mcmc,
               n_leapfrog=a.leapfrog, start_step=0.02)
    for name, opt in (("shared", None), ("rows", 0.75)):
        res = eng.hmc_sample(torch.from_numpy(x).to(eng.device), a.n_mcmc, a.burn_in, 0.02, a.leapfrog, 7, row_adapt=opt)
        d = chain_diagnostics(res["draws"])
        steps = res["row_step"].cpu().numpy() if opt is not None else np.full(a.n, float(res["step"].item()), np.float32)
        moved = d.moves[:, 0] / max(1, a.n_mcmc - 1)          # a move changes every coordinate: the acceptance frequency of the row
        r = {}
        for k, s in enumerate(shares):
            g = group == k
            ess, rhat = d.ess[g].reshape(-1), d.rhat[g].reshape(-1)
            ok = np.isfinite(ess) & np.isfinite(rhat)
            r["missing_%d" % round(100 * s)] = dict(acceptance=float(moved[g].mean()), step_quantiles_05_50_95=[float(t) for t in np.quantile(steps[g], [0.05, 0.5, 0.95])],
                                                   ess_median=float(np.median(ess[ok])), ess_q01=float(np.quantile(ess[ok], 0.01)),
                                                   share_rhat_above_1_01=float(np.mean(rhat[ok] > 1.01)))
        out[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("all", "cost", "burnin", "mixing"), default="all")
    ap.add_argument("--n", type=int, default=200000, help="rows of the cost and burn-in parts")
    ap.add_argument("--mixing-n", type=int, default=6000)
    ap.add_argument("--p", type=int, default=100, help="x_dim of the mixing part")
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--n-mcmc", type=int, default=None, help="default: 200 (burnin), 1000 (mixing)")
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--leapfrog", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for part, fn, n, keep in (("cost", part_cost, a.n, 0), ("burnin", part_burnin, a.n, 200), ("mixing", part_mixing, a.mixing_n, 1000)):
        if a.part in ("all", part):
            b = argparse.Namespace(**vars(a))
            b.n, b.n_mcmc = n, keep if a.n_mcmc is None else a.n_mcmc
            res[part] = fn(b)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
