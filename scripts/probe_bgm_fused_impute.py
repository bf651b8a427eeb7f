#!/usr/bin/env python3
"""Measurements of BGM's imputation inside the per-chain HMC kernel (csrc/bgm_rowstep_kernels.h, bgm_hmc_rows_impute_kernel) on one GPU.

  --part cost     ms per retained transition of the fused kernel (hmc_run_rows with moments) against bgm_hmc_rows_kernel (hmc_run_rows
                  without) on the same panel: N rows, L leapfrog steps, 50 % missing cells, p = 500 and p = 100, fp32.  The two arms
                  alternate in one process after a warm-up, HIP events; per arm the repeats, median, min and max.
  --part whole    wall time and peak device memory (torch's allocator) of the whole BGM.predict(row_adapt=True): the draws route at its
                  default max_draw_bytes against fused_predict=True, N rows, p = 500, burn-in + retained iterations as given, at 90 %
                  and at 10 % missing cells, the routes alternating, --whole-reps repeats each.

    timeout -k 10 1100 python scripts/probe_bgm_fused_impute.py --out profiles/bgm_fused_impute_probe.json
Not measured here: more than one GPU (the rank's shard is one launch either way), split precision (the fused kernel is fp32 only).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from probe_bgm_row_step import _engine, _panel, _timed  # noqa: E402


def _stats(v):
    return dict(values=[float(t) for t in v], median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def part_cost(a):
    import torch
    out = dict(part="cost", device=torch.cuda.get_device_name(0), n=a.n, n_leapfrog=a.leapfrog, transitions=a.transitions, missing=0.5, cases=[])
    for p in (500, 100):
        eng = _engine(p, "fp32")
        dev = eng.device
        x = torch.from_numpy(_panel(a.n, p, [0.5])[0]).to(dev)
        state, grad = (torch.empty((a.n, eng.q), device=dev) for _ in range(2))
        logp = torch.empty(a.n, device=dev)
        rows = torch.full((a.n,), 0.02, device=dev)
        mom = torch.full((3, a.n, p), float("nan"), device=dev)
        # every iteration is retained (burn_in = 0): the fused arm decodes after each transition
        run = dict(plain=lambda: eng.hmc_run_rows(x, state, logp, grad, rows, 0, a.transitions, 0, a.leapfrog, 7, init=True),
                   fused=lambda: eng.hmc_run_rows(x, state, logp, grad, rows, 0, a.transitions, 0, a.leapfrog, 7, init=True, moments=mom))
        for f in run.values():
            f()
        ms = {k: [] for k in run}
        for _ in range(a.reps):
            for k, f in run.items():
                ms[k].append(_timed(torch, f) / a.transitions)
        r = dict(p=p, ms_per_transition={k: _stats(v) for k, v in ms.items()})
        r["fused_over_plain"] = r["ms_per_transition"]["fused"]["median"] / r["ms_per_transition"]["plain"]["median"]
        print(json.dumps(r), file=sys.stderr, flush=True)
        out["cases"].append(r)
        eng.close()
        del x, mom
    return out


def part_whole(a):
    import torch
    from bayesgm_amd.models import BGM
    from oracle import bgm as OB
    p, q = 500, 10
    out = dict(part="whole", device=torch.cuda.get_device_name(0), n=a.whole_n, p=p, burn_in=a.burn_in, n_mcmc=a.n_mcmc, n_leapfrog=a.leapfrog,
               reps=a.whole_reps, cases=[])
    with tempfile.TemporaryDirectory() as tmp:
        params = dict(dataset="probe", output_dir=tmp, save_res=False, save_model=False, use_bnn=False, z_dim=q, x_dim=p, lr_theta=5e-3,
                      lr_z=5e-3, g_units=[64] * 5, e_units=[64] * 5, dz_units=[64, 32, 8], dx_units=[64, 32, 8], kl_weight=5e-5, lr=1e-3,
                      g_d_freq=1, use_z_rec=True, alpha=0.0, gamma=0.0)
        model = BGM(params, random_seed=0)
        model.set_weights(OB.init_model(11, q, p, g_units=(64,) * 5)["g"])
        for share in a.shares:
            x = _panel(a.whole_n, p, [share])[0]
            kw = dict(n_mcmc=a.n_mcmc, burn_in=a.burn_in, step_size=0.02, num_leapfrog_steps=a.leapfrog, seed=7, row_adapt=True)
            arms = dict(draws=dict(), fused=dict(fused_predict=True))
            sec, mem, timing = {k: [] for k in arms}, {k: [] for k in arms}, {}
            for rep in range(a.whole_reps):
                for k, extra in arms.items():
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    t0 = time.perf_counter()
                    model.predict(x, **kw, **extra)
                    torch.cuda.synchronize()
                    sec[k].append(time.perf_counter() - t0)
                    mem[k].append(torch.cuda.max_memory_allocated() / 2.0 ** 30)
                    timing[k] = {n_: float(v) for n_, v in model.last_predict_timing.items()}
                    print("missing %.2f rep %d %s: %.2f s, peak %.2f GiB" % (share, rep, k, sec[k][-1], mem[k][-1]), file=sys.stderr, flush=True)
            r = dict(missing=share, seconds={k: _stats(v) for k, v in sec.items()}, peak_gib={k: _stats(v) for k, v in mem.items()},
                     last_phase_seconds=timing)
            r["draws_over_fused"] = r["seconds"]["draws"]["median"] / r["seconds"]["fused"]["median"]
            print(json.dumps(r), file=sys.stderr, flush=True)
            out["cases"].append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("all", "cost", "whole"), default="all")
    ap.add_argument("--n", type=int, default=200000, help="rows of the cost part")
    ap.add_argument("--transitions", type=int, default=10)
    ap.add_argument("--leapfrog", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--whole-n", type=int, default=200000)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--n-mcmc", type=int, default=1000)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--shares", type=float, nargs="+", default=[0.9, 0.1])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(not_measured=["more than one GPU", "split precision (the fused kernel is fp32 only)", "exact quantiles against the normal interval"])
    for part, fn in (("cost", part_cost), ("whole", part_whole)):
        if a.part in ("all", part):
            res[part] = fn(a)
            if a.out:      # (after every part: a later part that runs out of time loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
