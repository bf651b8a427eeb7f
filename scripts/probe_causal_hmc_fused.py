#!/usr/bin/env python3
"""Measurements of the CausalBGM HMC sampler with the effect pass inside the kernel (csrc/causal_hmc_fx_kernels.h) on one GPU.
Everything runs in ONE process, the arms alternated, after a warm-up; p = 200, z_dims [1, 1, 1, 7], random weights, the
Hirano-Imbens panel, n_leapfrog 5, 20 doses.

  (a) transition   ms per RETAINED transition with the effects on (hmc_sample(effect=EFFECT_ADRF)) against off (the kernel without
                   effects), HIP events around the whole call (Gram pre-pass and LDS fills included in both arms), at every --n;
                   --reps repeats, median / min / max.
  (b) predict      CausalBGM.predict(sampler='hmc') -- the draws route at its default budget (or --budget) -- against
                   predict(sampler='hmc', fused_effects=True): wall seconds (device synchronised), peak device memory of the call
                   (torch.cuda.max_memory_allocated) and the acceptance rate predict reports; the settings are --predict N:burn:keep:reps.

    timeout -k 10 900 python scripts/probe_causal_hmc_fused.py --out profiles/causal_hmc_fused_probe.json
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
        return CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_fused", random_seed=0)


def part_transition(a, torch, model, n):
    from bayesgm_amd import _lib
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    x, y, v = Sim_Hirano_Imbens_sampler(N=n, v_dim=P, seed=0).load_all()
    eng = model.engine
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(eng.device) for t in (x, y, v))
    xd, yd = xd.reshape(-1), yd.reshape(-1)
    its = a.transitions
    arms = dict(off=dict(), on=dict(effect=_lib.EFFECT_ADRF, x_values=XS, sample_y=True))
    run = lambda kw: eng.hmc_sample(xd, yd, vd, 0, its, 0.1, LEAPFROG, 7, adapt=None, **kw)      # burn_in = 0: every transition is retained
    for kw in arms.values():
        run(kw)                                                                                   # packs, allocates
    ms = dict(off=[], on=[])
    for rep in range(a.reps):
        for name in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            ms[name].append(_timed(torch, lambda: run(arms[name])) / its)
            print(json.dumps(dict(part="transition", n=n, rep=rep, arm=name, ms_per_transition=ms[name][-1])), file=sys.stderr, flush=True)
    off, on = _spread(ms["off"]), _spread(ms["on"])
    return dict(n=n, transitions_per_launch=its, ms_per_retained_transition=dict(effects_off=off, effects_on=on),
                effect_pass_ms=on["median"] - off["median"], on_over_off=on["median"] / off["median"],
                effect_pass_over_gradient=(on["median"] - off["median"]) / (off["median"] / LEAPFROG))


def part_predict(a, torch, model, spec):
    from bayesgm_amd import causal_hmc as HM
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    n, burn, keep, reps = spec
    data = Sim_Hirano_Imbens_sampler(N=n, v_dim=P, seed=0).load_all()
    kw = dict(alpha=0.01, n_mcmc=keep, burn_in=burn, x_values=XS, verbose=0, sampler="hmc", n_leapfrog=LEAPFROG)
    arms = dict(draws=dict(draw_budget_bytes=a.budget), fused=dict(fused_effects=True))
    res = dict(draws=[], fused=[])
    out = {}
    for rep in range(reps):
        for name in (("draws", "fused") if rep % 2 == 0 else ("fused", "draws")):
            model._seed_counter = 0
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out[name] = model.predict(data, **dict(kw, **arms[name]))
            torch.cuda.synchronize()
            res[name].append(dict(seconds=time.perf_counter() - t0, peak_device_bytes=int(torch.cuda.max_memory_allocated()),
                                  acceptance=model.last_acceptance_rate))
            print(json.dumps(dict(part="predict", n=n, rep=rep, arm=name, **res[name][-1])), file=sys.stderr, flush=True)
    rows = HM.block_rows(keep, sum(Z_DIMS), a.budget)
    summary = {k: dict(seconds=_spread([r["seconds"] for r in v]), peak_device_bytes=max(r["peak_device_bytes"] for r in v),
                       acceptance=v[-1]["acceptance"]) for k, v in res.items()}
    return dict(n=n, burn_in=burn, n_mcmc=keep, repeats=reps, draws_route_block_rows=rows, draws_route_blocks=-(-n // rows),
                max_abs_difference_of_the_effect=float(np.abs(out["draws"][0] - out["fused"][0]).max()),
                fused_over_draws_seconds=summary["fused"]["seconds"]["median"] / summary["draws"]["seconds"]["median"], **summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=lambda s: [int(float(k)) for k in s.split(",")], default=[1000000, 100000])
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    spec = lambda s: tuple(int(float(k)) for k in s.split(":"))
    ap.add_argument("--predict", type=spec, action="append", default=None, help="N:burn_in:n_mcmc:repeats (repeatable)")
    ap.add_argument("--budget", type=int, default=None, help="draw_budget_bytes of the draws route (default: predict's 2 GiB)")
    ap.add_argument("--skip-transition", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    model = _model()
    res = dict(device=torch.cuda.get_device_name(0), p=P, z_dims=Z_DIMS, n_leapfrog=LEAPFROG, n_doses=N_DOSES,
               method="one process, arms alternated (order swapped every repeat) after a warm-up call of each; (a) HIP events around "
                      "hmc_sample, (b) time.perf_counter around predict with the device synchronised")
    if not a.skip_transition:
        res["transition"] = [part_transition(a, torch, model, n) for n in a.n]
    res["predict"] = [part_predict(a, torch, model, s) for s in (a.predict if a.predict is not None else [(100000, 1000, 1000, 3)])]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
