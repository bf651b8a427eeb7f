#!/usr/bin/env python3
"""Measurements of the CausalBGM HMC sampler that compares the doses per retained draw beside the rows' curves
(csrc/causal_hmc_choice_kernels.h) on one GPU.  The setup of scripts/probe_causal_hmc_contrast.py: ONE process, the arms alternated
(order rotated every repeat) after a warm-up call of each; p = 200, z_dims [1, 1, 1, 7], random weights, the Hirano-Imbens panel,
n_leapfrog 5, 20 doses; HIP events around the whole hmc_sample call (Gram pre-pass, LDS fills and the allocation of the outputs
included in every arm), burn_in = 0 so that every transition is retained; --reps repeats, median / min / max of ms per retained
transition.

  at every --n   rows          hmc_sample(row_effects=True): causal_hmc_rowfx_kernel, the kernel of before.  Its code object is the
                               parent commit's, instruction for instruction (scripts/compare_code_objects.py over the two builds
                               reports 0 differences), so the arm runs from this build's library
                 choice        the same with row_choice=True: causal_hmc_choice_kernel -- one multiply, three compares and two
                               selects per (row, dose, draw), one exchange over the lane groups and one counter per (row, draw)
                 choice_above  choice with a threshold: one more load, add and store per (row, dose, draw)
Beside the times: the memory of the new route (three curve planes, the counts, the best value's two planes, the exceedance counts)
against the [n x n_doses x n_mcmc] x 4 bytes of the row_draws route at the class defaults (n_mcmc = 3000).

    timeout -k 10 600 python scripts/probe_causal_hmc_choice.py --out profiles/causal_hmc_choice_probe.json
"""
import argparse
import contextlib
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

Z_DIMS, P, LEAPFROG, N_DOSES, N_MCMC = [1, 1, 1, 7], 200, 5, 20, 3000
PARAMS = dict(dataset="Sim_Hirano_Imbens", output_dir=".", save_res=False, save_model=False, binary_treatment=False, use_bnn=False,
              z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
              kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, e_units=[64] * 5, dz_units=[64, 32, 8], mixing_check=False)
XS = np.linspace(0.0, 3.0, N_DOSES)
ARMS = dict(rows=dict(), choice=dict(row_choice=True), choice_above=dict(row_choice=True, threshold=0.0))
PAIRS = (("choice", "rows"), ("choice_above", "rows"))


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
        return CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_choice", random_seed=0)


def _panel(n):
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    return Sim_Hirano_Imbens_sampler(N=n, v_dim=P, seed=0).load_all()


def part_kernel(a, torch, model, n):
    x, y, v = _panel(n)
    eng = model.engine
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(eng.device) for t in (x, y, v))
    xd, yd = xd.reshape(-1), yd.reshape(-1)
    its = a.transitions
    run = lambda kw: eng.hmc_sample(xd, yd, vd, 0, its, 0.1, LEAPFROG, 7, adapt=None, row_effects=True, x_values=XS, sample_y=True, **kw)
    names = list(ARMS)
    for name in names:
        run(ARMS[name])                                                                           # packs, allocates
        torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for rep in range(a.reps):
        k = rep % len(names)
        for name in names[k:] + names[:k]:
            ms[name].append(_timed(torch, lambda: run(ARMS[name])) / its)
            print(json.dumps(dict(n=n, rep=rep, arm=name, ms_per_transition=ms[name][-1])), file=sys.stderr, flush=True)
    ms = {name: _spread(v_) for name, v_ in ms.items()}
    plane = N_DOSES * n * 4
    return dict(n=n, transitions_per_launch=its, ms_per_retained_transition=ms,
                ratio={"%s_over_%s" % (new, old): ms[new]["median"] / ms[old]["median"] for new, old in PAIRS},
                bytes_at_the_defaults=dict(n_mcmc=N_MCMC, choice_route=3 * plane + plane + 2 * n * 4, choice_route_with_above=5 * plane + 2 * n * 4,
                                           row_draws_route=n * N_DOSES * N_MCMC * 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=lambda s: [int(float(k)) for k in s.split(",")], default=[100000, 1000000])
    ap.add_argument("--transitions", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    model = _model()
    res = dict(device=torch.cuda.get_device_name(0), p=P, z_dims=Z_DIMS, n_leapfrog=LEAPFROG, n_doses=N_DOSES,
               method="one process, arms alternated (order rotated every repeat) after a warm-up call of each; HIP events around "
                      "hmc_sample, burn_in = 0, every retained transition in one launch",
               kernel=[part_kernel(a, torch, model, n) for n in a.n])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
