"""What the per-chain proposal scale (row_adapt) costs and what it delivers, measured; nothing here is asserted.

  --part cost      burn-in and retained launch times of CausalEngine.mh_sample at the bench.py headline shape (N = 1e6, p = 200,
                   z_dims [1,1,1,7], random-init weights, 20 doses, event form), row-adaptive against the fixed q_sd = 1, alternated in
                   one process, from bgm_timing_read; the retained phase of the event form also by its served fraction
  --part tutorial  the tutorial setting of profiles/chain_diag_tutorial.json (CausalBGM use_bnn=False fitted on Hirano-Imbens N = 20000,
                   metropolis_hastings_sampler 5000 + 3000): acceptance and chain diagnostics at the fixed q_sd = 1, with the
                   reference's block-wide adaptive scale and with adaptive_sd='row', plus the quantiles of the per-row scales

    python scripts/probe_row_adapt.py --part cost [--n 1000000] [--burn-in 5000] [--n-mcmc 3000] [--reps 2] [--out profiles/row_adapt_cost.json]
    python scripts/probe_row_adapt.py --part tutorial [--out profiles/row_adapt_tutorial.json]
    rocprofv3 --kernel-trace --stats -- python scripts/probe_row_adapt.py --part cost --reps 1 --modes row      (and --modes fixed: the
        retained phase by kernel -- transitions, outcome net on the events, spread; summarised with scripts/prof_summary.py)
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
              kl_weight=1e-4, lr=2e-4, g_d_freq=5, use_z_rec=True, e_units=[64] * 5, dz_units=[64, 32, 8])


def part_cost(a):
    import torch
    from bayesgm_amd import _lib
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    from bayesgm_amd.models import CausalBGM
    x, y, v = Sim_Hirano_Imbens_sampler(N=a.n, v_dim=P, seed=0).load_all()
    model = CausalBGM(dict(PARAMS), timestamp="probe_row_adapt", random_seed=0)
    eng = model.engine
    dev = eng.device
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev) for t in (x, y, v))
    xs = np.linspace(0.0, 3.0, 20)
    eng.mh_sample(xd, yd, vd, 2, 2, 1.0, 1, effect=_lib.EFFECT_ADRF, x_values=xs)                       # packs, allocates
    eng.mh_sample(xd, yd, vd, 2, 2, 1.0, 1, effect=_lib.EFFECT_ADRF, x_values=xs, row_adapt=0.25)
    eng.timing_enable(True)
    runs = []
    for rep in range(a.reps):
        for mode in a.modes.split(","):
            eng.timing_read(kind=-1, reset=True)
            eng.outcome_cache_stats(reset=True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = eng.mh_sample(xd, yd, vd, a.burn_in, a.n_mcmc, 1.0, 7, effect=_lib.EFFECT_ADRF, x_values=xs,
                                row_adapt=0.25 if mode == "row" else None)
            torch.cuda.synchronize(); wall = time.perf_counter() - t0
            n_b, ms_b = eng.timing_read(kind=_lib.EFFECT_NONE)
            n_k, ms_k = eng.timing_read(kind=_lib.EFFECT_ADRF)
            served, total = eng.outcome_cache_stats()
            acc = out["acc_count"].double()
            r = dict(mode=mode, rep=rep, wall_s=wall, burn_in_launches=n_b, burn_in_ms=ms_b, retained_intervals=n_k, retained_ms=ms_k,
                     acceptance_burn_in=float(acc[:a.burn_in].sum()) / (a.burn_in * a.n), acceptance_retained=float(acc[a.burn_in:].sum()) / (a.n_mcmc * a.n),
                     events_per_retained_chain_iteration=1.0 - served / max(1, total))
            if mode == "row":
                s = out["row_scale"].cpu().numpy()
                r["scale_quantiles_01_05_50_95_99"] = [float(q) for q in np.quantile(s, [0.01, 0.05, 0.5, 0.95, 0.99])]
            runs.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    med = lambda mode, k: float(np.median([r[k] for r in runs if r["mode"] == mode]))
    if sorted(set(a.modes.split(","))) != ["fixed", "row"]:      # one mode alone (a run under a profiler): no ratios
        return dict(part="cost", device=torch.cuda.get_device_name(0), n=a.n, p=P, burn_in=a.burn_in, n_mcmc=a.n_mcmc, doses=20, runs=runs)
    return dict(part="cost", device=torch.cuda.get_device_name(0), n=a.n, p=P, z_dims=Z_DIMS, burn_in=a.burn_in, n_mcmc=a.n_mcmc, doses=20,
                burn_in_ms_fixed=med("fixed", "burn_in_ms"), burn_in_ms_row=med("row", "burn_in_ms"),
                burn_in_ratio=med("row", "burn_in_ms") / med("fixed", "burn_in_ms"),
                retained_ms_fixed=med("fixed", "retained_ms"), retained_ms_row=med("row", "retained_ms"),
                retained_ratio=med("row", "retained_ms") / med("fixed", "retained_ms"),
                note="the retained interval of the event form = transitions + outcome net on the events + spread; at the adapted scale "
                     "more proposals are accepted, so there are more events (events_per_retained_chain_iteration)", runs=runs)


def part_tutorial(a):
    import torch
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    from bayesgm_amd.models import CausalBGM
    x, y, v = Sim_Hirano_Imbens_sampler(N=20000, v_dim=P, seed=0).load_all()
    with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CausalBGM(dict(PARAMS, mixing_check=False), timestamp="probe_row_adapt_tutorial", random_seed=123)
        t0 = time.perf_counter()
        m.fit((x, y, v), epochs=100, epochs_per_eval=5, batch_size=32, use_egm_init=True, egm_n_iter=30000, egm_batches_per_eval=500, verbose=0)
        fit_s = time.perf_counter() - t0
        res = {}
        for name, kw in (("fixed_q_sd_1", dict(q_sd=1.0)), ("block_adaptive", dict(q_sd=None, adaptive_sd=True)),
                         ("row", dict(q_sd=1.0, adaptive_sd="row"))):
            m._seed_counter = 0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.metropolis_hastings_sampler((x, y, v), burn_in=5000, n_keep=3000, diagnostics=True, **kw)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            d = m.mcmc_diagnostics_
            r = dict(seconds=dt, acceptance=m.last_acceptance_rate, summary=d.summary(), moves_median=float(np.median(d.moves)),
                     moves_q01=float(np.quantile(d.moves, 0.01)))
            if name == "row":
                r["scale_quantiles_01_05_50_95_99"] = [float(q) for q in np.quantile(m.mh_row_scale_, [0.01, 0.05, 0.5, 0.95, 0.99])]
            res[name] = r
            print(name, json.dumps(r), file=sys.stderr, flush=True)
    return dict(part="tutorial", device=torch.cuda.get_device_name(0),
                setting="CausalBGM use_bnn=False, Sim_Hirano_Imbens N=20000 p=200 seed 0, egm_init 30000 + fit 100 epochs (random_seed 123), "
                        "metropolis_hastings_sampler burn_in=5000 n_keep=3000, same seed for the three modes", fit_s=fit_s, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("cost", "tutorial"), required=True)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--burn-in", type=int, default=5000)
    ap.add_argument("--n-mcmc", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--modes", default="fixed,row", help="cost part: fixed,row (alternated) or one of them (e.g. for a kernel trace of its own)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = part_cost(a) if a.part == "cost" else part_tutorial(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
