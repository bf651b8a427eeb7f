#!/usr/bin/env python3
"""Measurements of the CausalBGM HMC sampler that keeps the dose-response of every row (csrc/causal_hmc_rowfx_kernels.h) on one GPU.
The setup of scripts/probe_causal_hmc_fused.py: ONE process, the arms alternated (order rotated every repeat) after a warm-up call of
each; p = 200, z_dims [1, 1, 1, 7], random weights, the Hirano-Imbens panel, n_leapfrog 5, 20 doses; HIP events around the whole
hmc_sample call (Gram pre-pass, LDS fills and the allocation of the outputs included in every arm), burn_in = 0 so that every
transition is retained; --reps repeats, median / min / max of ms per retained transition.

  arms at every --n     off     the kernel without effects
                        adrf    hmc_sample(effect=EFFECT_ADRF): the fused panel average (causal_hmc_fx_kernels.h)
                        rows    hmc_sample(row_effects=True): the moments of every (row, dose)
  at --draws-n only     rows_long / rows_draws   --draws-transitions retained transitions in one launch, without / with the
                        [n, n_doses, transitions] draw matrix (row_draws=True); the matrix's bytes are recorded

    timeout -k 10 900 python scripts/probe_causal_hmc_rowfx.py --out profiles/causal_hmc_rowfx_probe.json
"""
import argparse
import contextlib
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

Z_DIMS, P, LEAPFROG, N_DOSES = [1, 1, 1, 7], 200, 5, 20
PARAMS = dict(dataset="Sim_Hirano_Imbens", output_dir=".", save_res=False, save_model=False, binary_treatment=False, use_bnn=False,
              z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
              kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, e_units=[64] * 5, dz_units=[64, 32, 8], mixing_check=False)
XS = np.linspace(0.0, 3.0, N_DOSES)


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
        return CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_rowfx", random_seed=0)


def _alternate(torch, run, arms, its, reps, tag):
    """ms per retained transition of every arm: a warm-up call of each, then reps rounds with the order rotated"""
    names = list(arms)
    for name in names:
        run(arms[name], its)                                                                      # packs, allocates
    ms = {name: [] for name in names}
    for rep in range(reps):
        k = rep % len(names)
        for name in names[k:] + names[:k]:
            ms[name].append(_timed(torch, lambda: run(arms[name], its)) / its)
            print(json.dumps(dict(tag, rep=rep, arm=name, ms_per_transition=ms[name][-1])), file=sys.stderr, flush=True)
    return {name: _spread(v) for name, v in ms.items()}


def part_transition(a, torch, model, n):
    from bayesgm_amd import _lib
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    x, y, v = Sim_Hirano_Imbens_sampler(N=n, v_dim=P, seed=0).load_all()
    eng = model.engine
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(eng.device) for t in (x, y, v))
    xd, yd = xd.reshape(-1), yd.reshape(-1)
    run = lambda kw, its: eng.hmc_sample(xd, yd, vd, 0, its, 0.1, LEAPFROG, 7, adapt=None, **kw)      # burn_in = 0: every transition is retained
    fx = dict(x_values=XS, sample_y=True)
    arms = dict(off=dict(), adrf=dict(effect=_lib.EFFECT_ADRF, **fx), rows=dict(row_effects=True, **fx))
    ms = _alternate(torch, run, arms, a.transitions, a.reps, dict(part="transition", n=n))
    res = dict(n=n, transitions_per_launch=a.transitions, ms_per_retained_transition=ms,
               rows_over_adrf=ms["rows"]["median"] / ms["adrf"]["median"], rows_over_off=ms["rows"]["median"] / ms["off"]["median"],
               adrf_over_off=ms["adrf"]["median"] / ms["off"]["median"],
               moment_planes_bytes=3 * N_DOSES * n * 4)
    if n == a.draws_n:
        its = a.draws_transitions
        long_arms = dict(rows_long=dict(row_effects=True, **fx), rows_draws=dict(row_effects=True, row_draws=True, **fx))
        ms = _alternate(torch, run, long_arms, its, a.reps, dict(part="draws", n=n))
        res["with_row_draws"] = dict(transitions_per_launch=its, ms_per_retained_transition=ms, row_draws_bytes=n * N_DOSES * its * 4,
                                     draws_over_moments=ms["rows_draws"]["median"] / ms["rows_long"]["median"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=lambda s: [int(float(k)) for k in s.split(",")], default=[1000000, 100000])
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws-n", type=lambda s: int(float(s)), default=100000, help="the one N at which the arm that stores the row draws runs")
    ap.add_argument("--draws-transitions", type=int, default=3000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    model = _model()
    res = dict(device=torch.cuda.get_device_name(0), p=P, z_dims=Z_DIMS, n_leapfrog=LEAPFROG, n_doses=N_DOSES,
               method="one process, arms alternated (order rotated every repeat) after a warm-up call of each; HIP events around "
                      "hmc_sample, burn_in = 0",
               transition=[part_transition(a, torch, model, n) for n in a.n])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
