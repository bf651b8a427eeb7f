#!/usr/bin/env python3
"""Measurements of the CausalBGM HMC sampler for partially observed rows (csrc/causal_hmc_obs_kernels.h) on one GPU.  The setup of
scripts/probe_causal_hmc_group.py: ONE process, the arms alternated (order rotated every repeat) after a warm-up call of each;
p = 200, z_dims [1, 1, 1, 7], random weights, the Hirano-Imbens panel, n_leapfrog 5, a fixed step; HIP events around the whole
hmc_sample call (Gram pre-pass, LDS fill and the allocation of the outputs included in every arm), burn_in = 0; --reps repeats,
median / min / max of ms per transition.

  arms at every --n     observed        hmc_sample on the observed panel: the existing kernel (its code object is the parent
                                        library's, scripts/compare_code_objects.py)
                        obs_observed    the same panel with partial=True: the OBS kernel, every tile runs f and h -- the cost of the
                                        masks and of the two wave-uniform branches
                        obs_no_y        partial=True, every outcome missing: f's forward and backward passes are skipped
                        obs_no_xy       partial=True, outcome and treatment missing: f's and h's passes are skipped
  The chains of the four arms are different chains (different targets); with a fixed step and burn_in = 0 every transition costs
  the same whatever it decides.

    timeout -k 10 600 python scripts/probe_causal_hmc_partial.py --out profiles/causal_hmc_partial_probe.json
"""
import argparse
import contextlib
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

Z_DIMS, P, LEAPFROG = [1, 1, 1, 7], 200, 5
PARAMS = dict(dataset="Sim_Hirano_Imbens", output_dir=".", save_res=False, save_model=False, binary_treatment=False, use_bnn=False,
              z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
              kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, e_units=[64] * 5, dz_units=[64, 32, 8], mixing_check=False)


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _spread(vals):
    return dict(median=float(np.median(vals)), min=float(np.min(vals)), max=float(np.max(vals)), n=len(vals))


def _model():
    from bayesgm_amd.models import CausalBGM
    with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_partial", random_seed=0)


def part_transition(a, torch, model, n):
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    x, y, v = Sim_Hirano_Imbens_sampler(N=n, v_dim=P, seed=0).load_all()
    eng = model.engine
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(eng.device) for t in (x, y, v))
    xd, yd = xd.reshape(-1), yd.reshape(-1)
    nan = torch.full_like(yd, float("nan"))
    arms = dict(observed=(xd, yd, False), obs_observed=(xd, yd, True), obs_no_y=(xd, nan, True), obs_no_xy=(nan, nan, True))
    its = a.transitions

    def run(arm):
        xa, ya, partial = arm
        return eng.hmc_sample(xa, ya, vd, 0, its, 0.1, LEAPFROG, 7, adapt=None, partial=partial)      # burn_in = 0, fixed step

    names = list(arms)
    acc = {}
    for name in names:                                                                            # packs, allocates
        acc[name] = float(run(arms[name])["acc_count"].sum().item()) / (its * n)
    ms = {name: [] for name in names}
    for rep in range(a.reps):
        k = rep % len(names)
        for name in names[k:] + names[:k]:
            ms[name].append(_timed(torch, lambda: run(arms[name])) / its)
            print(json.dumps(dict(n=n, rep=rep, arm=name, ms_per_transition=ms[name][-1])), file=sys.stderr, flush=True)
    ms = {name: _spread(vals) for name, vals in ms.items()}
    base = ms["observed"]
    return dict(n=n, transitions_per_launch=its, ms_per_transition=ms, acceptance=acc,
                over_observed={name: ms[name]["median"] / base["median"] for name in names[1:]},
                observed_spread=dict(min_over_median=base["min"] / base["median"], max_over_median=base["max"] / base["median"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=lambda s: [int(float(k)) for k in s.split(",")], default=[1000000, 100000])
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    model = _model()
    n_gh = len(PARAMS["g_units"]) - 1
    res = dict(device=torch.cuda.get_device_name(0), p=P, z_dims=Z_DIMS, n_leapfrog=LEAPFROG,
               method="one process, arms alternated (order rotated every repeat) after a warm-up call of each; HIP events around "
                      "hmc_sample, burn_in = 0, fixed step 0.1",
               products_per_direction=dict(f=44, h=44, all=12 + 64 * n_gh + 64 + 88,
                                           note="16-row x 16-column tile products of one gradient evaluation, forward or backward: "
                                                "12 KT1 first layers, 64 per hidden layer of g, 64 Gram, 2 x 44 f and h"),
               transition=[part_transition(a, torch, model, n) for n in a.n])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
