#!/usr/bin/env python3
"""Measurements of the trajectory options of the CausalBGM HMC sampler (csrc/causal_hmc_traj_kernels.h, max_trajectory / jitter) on
one GPU.  The setup of scripts/probe_causal_hmc_partial.py: ONE process, the arms alternated (order rotated every repeat) after a
warm-up call of each; p = 200, z_dims [1, 1, 1, 7], random weights, the Hirano-Imbens panel; HIP events around the whole call (Gram
pre-pass, LDS fill and the allocation of the outputs included in every arm), burn_in = 0, frozen steps; --reps repeats, median / min /
max of ms per transition.  Nothing here is a pass bar.

  price    at every --n, n_leapfrog 5, step 0.1:
             base       hmc_sample: the existing kernel (its code object is the parent library's, scripts/compare_code_objects.py)
             traj_free  max_trajectory = 1e9: the TRAJ kernel under a cap that never binds, the same chain bit for bit
  saving   at every --n, frozen steps, T = 0.13 of n_leapfrog 6 (step 0.05: 3 steps, step 0.03: 5 steps):
             base_L6 / base_L5 / base_L3   the existing kernel at n_leapfrog 6 (step 0.05), 5 (step 0.03) and 3 (step 0.05)
             cap_uniform                   every row 3 of 6
             cap_sorted                    the first half of the rows 3, the second half 5: every tile is uniform (the wave-level exit)
             cap_interleaved               3 and 5 alternating by row inside every tile: every wave runs 5
  mixing   the fitted model of profiles/row_adapt_tutorial.json (Hirano-Imbens N = 20000, egm_init 30000 + 100 epochs, random_seed
           123), n_leapfrog 5, step 0.1, --burn-in + --n-mcmc transitions, the same seed for every setting; panels: observed,
           y unobserved, x and y unobserved (partial=True); settings: no cap, max_trajectory pi / 2, pi, jitter alone.

    timeout -k 10 1100 python scripts/probe_causal_hmc_traj.py --out profiles/causal_hmc_traj_probe.json
"""
import argparse
import contextlib
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

Z_DIMS, P = [1, 1, 1, 7], 200
PARAMS = dict(dataset="Sim_Hirano_Imbens", output_dir=".", save_res=False, save_model=False, binary_treatment=False, use_bnn=False,
              z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
              kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, e_units=[64] * 5, dz_units=[64, 32, 8], mixing_check=False)
T_CAP, L_CAP = 0.13, 6


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _spread(vals):
    return dict(median=float(np.median(vals)), min=float(np.min(vals)), max=float(np.max(vals)), n=len(vals))


def _model(seed=0):
    from bayesgm_amd.models import CausalBGM
    with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_traj", random_seed=seed)


def _alternate(a, torch, arms, its, n, tag):
    """warm-up call of every arm, then --reps rounds with the order rotated -> {arm: spread of ms per transition}"""
    names = list(arms)
    for name in names:
        arms[name]()
    ms = {name: [] for name in names}
    for rep in range(a.reps):
        k = rep % len(names)
        for name in names[k:] + names[:k]:
            ms[name].append(_timed(torch, arms[name]) / its)
            print(json.dumps(dict(part=tag, n=n, rep=rep, arm=name, ms_per_transition=ms[name][-1])), file=sys.stderr, flush=True)
    return {name: _spread(vals) for name, vals in ms.items()}


def _panel(torch, eng, n):
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    x, y, v = Sim_Hirano_Imbens_sampler(N=n, v_dim=P, seed=0).load_all()
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(eng.device) for t in (x, y, v))
    return xd.reshape(-1), yd.reshape(-1), vd


def part_price(a, torch, eng, n):
    xd, yd, vd = _panel(torch, eng, n)
    its, L = a.transitions, 5
    arms = dict(base=lambda: eng.hmc_sample(xd, yd, vd, 0, its, 0.1, L, 7, adapt=None),
                traj_free=lambda: eng.hmc_sample(xd, yd, vd, 0, its, 0.1, L, 7, adapt=None, max_trajectory=1e9))
    same = bool(torch.equal(arms["base"]()["state"], arms["traj_free"]()["state"]))
    ms = _alternate(a, torch, arms, its, n, "price")
    base = ms["base"]
    ratio = ms["traj_free"]["median"] / base["median"]
    lo, hi = base["min"] / base["median"], base["max"] / base["median"]
    return dict(n=n, n_leapfrog=L, transitions_per_launch=its, ms_per_transition=ms, same_chain=same, traj_free_over_base=ratio,
                base_spread=dict(min_over_median=lo, max_over_median=hi), ratio_inside_base_spread=bool(lo <= ratio <= hi))


def part_saving(a, torch, eng, n):
    xd, yd, vd = _panel(torch, eng, n)
    its, dev, q = a.transitions, eng.device, eng.q
    rows = torch.arange(n, device=dev)
    steps = dict(s05=torch.full((n,), 0.05, device=dev), s03=torch.full((n,), 0.03, device=dev),
                 sorted=torch.where(rows < n // 2, 0.05, 0.03).float(), interleaved=torch.where(rows % 2 == 0, 0.05, 0.03).float())
    buf = dict(state=torch.empty((n, q), device=dev), logp=torch.empty(n, device=dev), grad=torch.empty((n, q), device=dev),
               step=torch.empty(n, device=dev), acc=torch.zeros(its, device=dev, dtype=torch.int32), n_steps=torch.zeros(n, device=dev, dtype=torch.int32))

    def run(step, L, cap):
        buf["step"].copy_(steps[step])
        buf["n_steps"].zero_()
        if cap:
            eng.set_hmc_trajectory(T_CAP, False, buf["n_steps"])
        try:
            eng.hmc_run(xd, yd, vd, buf["state"], buf["logp"], buf["grad"], buf["step"], 0, its, 0, L, 7, init=True, acc_count=buf["acc"])
        finally:
            if cap:
                eng.set_hmc_trajectory(None)

    arms = dict(base_L6=lambda: run("s05", 6, False), base_L5=lambda: run("s03", 5, False), base_L3=lambda: run("s05", 3, False),
                cap_uniform=lambda: run("s05", L_CAP, True), cap_sorted=lambda: run("sorted", L_CAP, True),
                cap_interleaved=lambda: run("interleaved", L_CAP, True))
    mean_steps = {}
    for name in ("cap_uniform", "cap_sorted", "cap_interleaved"):
        arms[name]()
        mean_steps[name] = float(buf["n_steps"].double().mean().item()) / its
    ms = _alternate(a, torch, arms, its, n, "saving")
    med = {k: w["median"] for k, w in ms.items()}
    return dict(n=n, n_leapfrog=L_CAP, max_trajectory=T_CAP, transitions_per_launch=its, ms_per_transition=ms, mean_steps=mean_steps,
                over_base_L6={k: med[k] / med["base_L6"] for k in med}, cap_uniform_over_base_L3=med["cap_uniform"] / med["base_L3"],
                cap_sorted_over_mean_L3_L5=med["cap_sorted"] / (0.5 * (med["base_L3"] + med["base_L5"])),
                cap_interleaved_over_base_L5=med["cap_interleaved"] / med["base_L5"],
                base_L6_spread=dict(min_over_median=ms["base_L6"]["min"] / med["base_L6"], max_over_median=ms["base_L6"]["max"] / med["base_L6"]))


def part_mixing(a, torch):
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    from bayesgm_amd.models import CausalBGM
    L, step0 = 5, 0.1
    x, y, v = Sim_Hirano_Imbens_sampler(N=20000, v_dim=P, seed=0).load_all()
    with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_traj_tutorial", random_seed=123)
        t0 = time.perf_counter()
        m.fit((x, y, v), epochs=100, epochs_per_eval=5, batch_size=32, use_egm_init=True, egm_n_iter=30000, egm_batches_per_eval=500, verbose=0)
        fit_s = time.perf_counter() - t0
        nan = np.full_like(np.asarray(y, np.float32), np.nan)
        panels = dict(observed=(x, y, False), y_unobserved=(x, nan, True), xy_unobserved=(nan, nan, True))
        settings = dict(no_cap=dict(), cap_half_pi=dict(max_trajectory=float(np.pi / 2)), cap_pi=dict(max_trajectory=float(np.pi)),
                        jitter=dict(jitter_leapfrog=True))
        res = {}
        for pname, (px, py, partial) in panels.items():
            res[pname] = {}
            for sname, opt in settings.items():
                m._seed_counter = 0
                torch.cuda.synchronize(); t0 = time.perf_counter()
                m.hmc_sampler((px, py, v), n_keep=a.n_mcmc, burn_in=a.burn_in, step_size=step0, n_leapfrog=L, diagnostics=True, partial=partial, **opt)
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
                d = m.mcmc_diagnostics_
                ess = d.ess[np.isfinite(d.ess)]
                steps = m.hmc_row_step_
                lf = m.hmc_row_leapfrog_
                r = dict(seconds=dt, acceptance=m.last_acceptance_rate, ess_median=float(np.median(ess)), ess_q01=float(np.quantile(ess, 0.01)),
                         share_rhat_above_1_01=float(np.mean(d.rhat[np.isfinite(d.rhat)] > 1.01)), ess_median_per_second=float(np.median(ess)) / dt,
                         step_quantiles_01_05_50_95_99=[float(t) for t in np.quantile(steps, [0.01, 0.05, 0.5, 0.95, 0.99])],
                         step_max=float(steps.max()), share_step_x_L_at_least_half_pi=float(np.mean(steps * L >= np.pi / 2)),
                         mean_leapfrog=float(L if lf is None else lf.mean()),
                         leapfrog_quantiles_01_50_99=None if lf is None else [float(t) for t in np.quantile(lf, [0.01, 0.5, 0.99])])
                res[pname][sname] = r
                print(pname, sname, json.dumps(r), file=sys.stderr, flush=True)
    return dict(setting="CausalBGM use_bnn=False, Sim_Hirano_Imbens N=20000 p=200 seed 0, egm_init 30000 + fit 100 epochs (random_seed 123), "
                        "hmc_sampler step_size 0.1 n_leapfrog %d burn_in=%d n_keep=%d, same seed for all settings; seconds include the "
                        "diagnostics and the copy of the draws to the host" % (L, a.burn_in, a.n_mcmc), fit_s=fit_s, panels=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=lambda s: [int(float(k)) for k in s.split(",")], default=[1000000, 100000])
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--n-mcmc", type=int, default=1000)
    ap.add_argument("--parts", default="price,saving,mixing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    parts = a.parts.split(",")
    res = dict(device=torch.cuda.get_device_name(0), p=P, z_dims=Z_DIMS,
               method="one process, arms alternated (order rotated every repeat) after a warm-up call of each; HIP events around the "
                      "whole call, burn_in = 0, frozen steps; median (min .. max) of %d repeats" % a.reps)
    if "price" in parts or "saving" in parts:
        eng = _model().engine
        if "price" in parts:
            res["price"] = [part_price(a, torch, eng, n) for n in a.n]
        if "saving" in parts:
            res["saving"] = [part_saving(a, torch, eng, n) for n in a.n]
    if "mixing" in parts:
        res["mixing"] = part_mixing(a, torch)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
