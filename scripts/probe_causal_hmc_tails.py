#!/usr/bin/env python3
"""Measurements of the CausalBGM HMC sampler that keeps the two tails of every (row, dose) series (csrc/causal_hmc_tails_kernels.h) on
one GPU.  The setup of scripts/probe_causal_hmc_rowfx.py: ONE process, the arms alternated (order rotated every repeat) after a
warm-up call of each; p = 200, z_dims [1, 1, 1, 7], random weights, the Hirano-Imbens panel, n_leapfrog 5, 20 doses; HIP events
around the whole hmc_sample call (Gram pre-pass, LDS fills and the allocation of the outputs included in every arm), burn_in = 0 so
that every transition is retained; --reps repeats, median / min / max of ms per retained transition.

  kernel, at every --n   rows      hmc_sample(row_effects=True): the moments of every (row, dose) -- the kernel of before
                         tails16   the same with row_tails=16 (alpha = 0.01 at 3000 draws)
                         tails76   the same with row_tails=76 (alpha = 0.05 at 3000 draws)
     ALL --transitions (3000) retained transitions in ONE launch: a draw enters a tail at a rate that falls like K / d, so a short
     sample would overstate the cost.
  class, at --class-n    CausalBGM.predict_individual(interval='tails') against interval='quantile' at the default draw budget and the
                         class's default burn_in: wall time (time.perf_counter around the call, synchronised) and the allocator's
                         peak (torch.cuda.max_memory_allocated), --class-reps alternated repeats after a short warm-up of each.

    timeout -k 10 1100 python scripts/probe_causal_hmc_tails.py --out profiles/causal_hmc_tails_probe.json
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

Z_DIMS, P, LEAPFROG, N_DOSES = [1, 1, 1, 7], 200, 5, 20
PARAMS = dict(dataset="Sim_Hirano_Imbens", output_dir=".", save_res=False, save_model=False, binary_treatment=False, use_bnn=False,
              z_dims=Z_DIMS, v_dim=P, lr_theta=1e-4, lr_z=1e-4, g_units=[64] * 5, f_units=[64, 32, 8], h_units=[64, 32, 8],
              kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, e_units=[64] * 5, dz_units=[64, 32, 8], mixing_check=False)
XS = np.linspace(0.0, 3.0, N_DOSES)
TAILS = (16, 76)


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
        return CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_tails", random_seed=0)


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
    arms = dict(rows=dict(), **{"tails%d" % k: dict(row_tails=k) for k in TAILS})
    names = list(arms)
    for name in names:
        run(arms[name])                                                                           # packs, allocates
        torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for rep in range(a.reps):
        k = rep % len(names)
        for name in names[k:] + names[:k]:
            ms[name].append(_timed(torch, lambda: run(arms[name])) / its)
            print(json.dumps(dict(part="kernel", n=n, rep=rep, arm=name, ms_per_transition=ms[name][-1])), file=sys.stderr, flush=True)
    ms = {name: _spread(v_) for name, v_ in ms.items()}
    # how often a draw entered a tail, counted on the host from the draws of a few rows (the kernel keeps no counter)
    few = eng.hmc_sample(xd[:64], yd[:64], vd[:64], 0, its, 0.1, LEAPFROG, 7, adapt=None, row_effects=True, row_draws=True, x_values=XS)
    series = few["row_draws"].reshape(-1, its).cpu().numpy()
    entries = {}
    for k in TAILS:
        cnt = []
        for s in series[::16]:
            kept, c = sorted(s[:k]), 0
            for val in s[k:]:
                if val < kept[-1]:
                    kept[-1] = val
                    kept.sort()
                    c += 1
            cnt.append(c)
        entries["tails%d" % k] = dict(mean_entries_per_tail_after_fill=float(np.mean(cnt)), expected_k_ln_m_over_k=float(k * np.log(its / k)))
    return dict(n=n, transitions_per_launch=its, ms_per_retained_transition=ms, entries=entries,
                over_rows={name: ms[name]["median"] / ms["rows"]["median"] for name in names if name != "rows"},
                tail_bytes={"tails%d" % k: 2 * k * N_DOSES * n * 4 for k in TAILS}, moment_planes_bytes=3 * N_DOSES * n * 4,
                row_draws_bytes_if_stored=n * N_DOSES * its * 4)


def part_class(a, torch, model):
    n = a.class_n
    data = _panel(n)
    res = {name: dict(wall_s=[], peak_bytes=[]) for name in ("tails", "quantile")}

    def call(interval, **kw):
        with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return model.predict_individual(data, XS, alpha=a.alpha, interval=interval, verbose=0, **kw)
    for name in res:
        call(name, n_mcmc=40, burn_in=20)                                                         # packs, allocates
    bounds = {}
    for rep in range(a.class_reps):
        for name in (("tails", "quantile") if rep % 2 == 0 else ("quantile", "tails")):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            model._seed_counter = 1000 + rep                                                      # both intervals on one chain
            _, b = call(name, n_mcmc=a.transitions)
            torch.cuda.synchronize()
            res[name]["wall_s"].append(time.perf_counter() - t0)
            res[name]["peak_bytes"].append(int(torch.cuda.max_memory_allocated()))
            bounds[name] = b
            print(json.dumps(dict(part="class", n=n, rep=rep, arm=name, wall_s=res[name]["wall_s"][-1], peak=res[name]["peak_bytes"][-1])),
                  file=sys.stderr, flush=True)
    from bayesgm_amd import causal_hmc as HM
    k = HM.tail_size(a.alpha, a.transitions)
    return dict(n=n, alpha=a.alpha, n_mcmc=a.transitions, burn_in="class default", k_tail=k,
                blocks={name: len(HM.individual_blocks([(0, n)], a.transitions, N_DOSES, name, None, k)) for name in res},
                wall_s={name: _spread(r["wall_s"]) for name, r in res.items()}, peak_bytes={name: max(r["peak_bytes"]) for name, r in res.items()},
                bounds_bit_identical=bool(np.array_equal(bounds["tails"], bounds["quantile"])),
                quantile_over_tails_wall=float(np.median(res["quantile"]["wall_s"]) / np.median(res["tails"]["wall_s"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=lambda s: [int(float(k)) for k in s.split(",")], default=[1000000, 100000])
    ap.add_argument("--transitions", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--class-n", type=lambda s: int(float(s)), default=100000)
    ap.add_argument("--class-reps", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    model = _model()
    res = dict(device=torch.cuda.get_device_name(0), p=P, z_dims=Z_DIMS, n_leapfrog=LEAPFROG, n_doses=N_DOSES,
               method="one process, arms alternated (order rotated every repeat) after a warm-up call of each; HIP events around "
                      "hmc_sample, burn_in = 0, every retained transition in one launch",
               kernel=[part_kernel(a, torch, model, n) for n in a.n])
    if a.class_n > 0:
        res["predict_individual"] = part_class(a, torch, model)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
