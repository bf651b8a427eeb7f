#!/usr/bin/env python3
"""Measurements of the HMC latent sampler of CausalBGM (csrc/causal_hmc_kernels.h) on one GPU.

  --part cost      ms per HMC transition and per gradient evaluation at N rows (p = 200, random weights), by HIP events after a
                   warm-up, alternated with an MH launch (fixed q_sd, burn-in kernel) on the same panel in the same process.
  --part tutorial  the setting of profiles/row_adapt_tutorial.json (CausalBGM use_bnn=False fitted on Hirano-Imbens N = 20000,
                   5000 + 3000 transitions, one seed): row-adaptive MH against HMC with n_leapfrog in {1, 3, 5, 10}; acceptance,
                   step quantiles, chain diagnostics, wall time and ESS per second.
  --part panel     the concentrated panel of the tests (sigma_v = 0.02, z_dims [3, 3, 3, 1], p = 50, random weights, no fit), --n rows:
                   HMC for every n_leapfrog, the same diagnostics.
  --mass           adds the metric axis (causal_hmc_mass_kernels.h): in `cost`, the metric kernel with mass_scale = 1 alternated with the
                   identity-mass kernel in the same process; in `tutorial` / `panel`, mass='diag' next to identity mass for every
                   n_leapfrog, with the per-coordinate quantiles of s.

    timeout -k 10 600 python scripts/probe_causal_hmc.py --part cost --n 1000000 --out profiles/causal_hmc_probe.json
    timeout -k 10 1100 python scripts/probe_causal_hmc.py --part tutorial --out profiles/causal_hmc_tutorial.json
    timeout -k 10 500 python scripts/probe_causal_hmc.py --part cost --mass --n 1000000 --out profiles/causal_hmc_mass_probe.json
    timeout -k 10 1100 python scripts/probe_causal_hmc.py --part tutorial --mass --out profiles/causal_hmc_mass_tutorial.json
    rocprofv3 --kernel-trace --stats -- python scripts/probe_causal_hmc.py --part cost --n 1000000 --reps 1      (a run of its own)
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


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def part_cost(a):
    import torch
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    from bayesgm_amd.models import CausalBGM
    x, y, v = Sim_Hirano_Imbens_sampler(N=a.n, v_dim=P, seed=0).load_all()
    eng = CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc", random_seed=0).engine
    dev = eng.device
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev) for t in (x, y, v))
    xd, yd = xd.reshape(-1), yd.reshape(-1)
    n, its = a.n, a.transitions
    eng.hmc_sample(xd, yd, vd, 1, 1, 0.1, 1, 1)                      # packs, allocates
    eng.mh_sample(xd, yd, vd, 2, 0, 1.0, 1)
    ones = torch.ones((n, eng.q), device=dev)
    if a.mass:
        eng.hmc_sample(xd, yd, vd, 1, 1, 0.1, 1, 1, mass_scale=ones)
    runs = []
    for rep in range(a.reps):
        for L in a.leapfrog:
            ms = _timed(torch, lambda: eng.hmc_sample(xd, yd, vd, its, 0, 0.1, L, 7, adapt=None))      # (+ 1 evaluation at init, the prepass and the fills)
            runs.append(dict(kind="hmc", rep=rep, n_leapfrog=L, transitions=its, ms=ms, ms_per_transition=ms / its,
                             ms_per_gradient=ms / (its * L + 1)))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
            if a.mass:      # the metric kernel on unit scales: the same chain, bit for bit
                ms = _timed(torch, lambda: eng.hmc_sample(xd, yd, vd, its, 0, 0.1, L, 7, adapt=None, mass_scale=ones))
                runs.append(dict(kind="hmc_mass", rep=rep, n_leapfrog=L, transitions=its, ms=ms, ms_per_transition=ms / its))
                print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        ms = _timed(torch, lambda: eng.mh_sample(xd, yd, vd, a.mh_transitions, 0, 1.0, 7))
        runs.append(dict(kind="mh", rep=rep, transitions=a.mh_transitions, ms=ms, ms_per_transition=ms / a.mh_transitions))
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        z = torch.randn((n, eng.q), device=dev)
        eng.logpost_grad(xd, yd, vd, z)
        ms = _timed(torch, lambda: eng.logpost_grad(xd, yd, vd, z))
        runs.append(dict(kind="logpost_grad", rep=rep, ms=ms))
    med = lambda f, k: float(np.median([r[k] for r in runs if f(r)]))
    mh = med(lambda r: r["kind"] == "mh", "ms_per_transition")
    out = dict(part="cost", device=torch.cuda.get_device_name(0), n=n, p=P, z_dims=Z_DIMS, mh_ms_per_transition=mh,
               logpost_grad_call_ms=med(lambda r: r["kind"] == "logpost_grad", "ms"), runs=runs,
               note="expectation: a gradient evaluation ~ 2 Gram-form MH transitions, a transition with L steps ~ 2 L; "
                    "logpost_grad_call_ms includes the Gram prepass over the panel and the weights' LDS fill")
    for L in a.leapfrog:
        t = med(lambda r: r["kind"] == "hmc" and r["n_leapfrog"] == L, "ms_per_transition")
        g = med(lambda r: r["kind"] == "hmc" and r["n_leapfrog"] == L, "ms_per_gradient")
        out["L%d" % L] = dict(ms_per_transition=t, ms_per_gradient=g, transition_over_mh=t / mh, gradient_over_mh=g / mh)
        if a.mass:
            tm = med(lambda r: r["kind"] == "hmc_mass" and r["n_leapfrog"] == L, "ms_per_transition")
            out["L%d" % L].update(mass_ms_per_transition=tm, mass_over_identity=tm / t)
    return out


def _mixing(a, torch, m, data, with_mh):
    """every mode on one fitted / given model with the same seed -> {mode: figures}"""
    x, y, v = data
    res = {}
    modes = ([("mh_row", None, None)] if with_mh else []) + [("hmc_L%d" % L, L, "identity") for L in a.leapfrog]
    if a.mass:
        modes += [("hmc_diag_L%d" % L, L, "diag") for L in a.leapfrog]
    for name, L, mass in modes:
        m._seed_counter = 0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if L is None:
            m.metropolis_hastings_sampler((x, y, v), q_sd=1.0, adaptive_sd="row", burn_in=a.burn_in, n_keep=a.n_mcmc, diagnostics=True)
            steps = m.mh_row_scale_
        else:
            m.hmc_sampler((x, y, v), n_keep=a.n_mcmc, burn_in=a.burn_in, step_size=0.1, n_leapfrog=L, diagnostics=True, mass=mass)
            steps = m.hmc_row_step_
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        d = m.mcmc_diagnostics_
        s = d.summary()
        ess = d.ess[np.isfinite(d.ess)]
        r = dict(seconds=dt, acceptance=m.last_acceptance_rate, summary=s, ess_median=float(np.median(ess)), ess_q01=float(np.quantile(ess, 0.01)),
                 share_rhat_above_1_01=float(np.mean(d.rhat[np.isfinite(d.rhat)] > 1.01)), ess_median_per_second=float(np.median(ess)) / dt,
                 step_quantiles_01_05_50_95_99=[float(q) for q in np.quantile(steps, [0.01, 0.05, 0.5, 0.95, 0.99])])
        if mass == "diag":      # per coordinate: the 5 % / 50 % / 95 % quantiles of s over the chains
            r["mass_scale_quantiles_05_50_95"] = [[float(t) for t in np.quantile(m.hmc_row_mass_[:, i], [0.05, 0.5, 0.95])]
                                                  for i in range(m.hmc_row_mass_.shape[1])]
        res[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    return res


def part_tutorial(a):
    import torch
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    from bayesgm_amd.models import CausalBGM
    x, y, v = Sim_Hirano_Imbens_sampler(N=20000, v_dim=P, seed=0).load_all()
    with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CausalBGM(dict(PARAMS, mixing_check=False), timestamp="probe_causal_hmc_tutorial", random_seed=123)
        t0 = time.perf_counter()
        m.fit((x, y, v), epochs=100, epochs_per_eval=5, batch_size=32, use_egm_init=True, egm_n_iter=30000, egm_batches_per_eval=500, verbose=0)
        fit_s = time.perf_counter() - t0
        res = _mixing(a, torch, m, (x, y, v), True)
    return dict(part="tutorial", device=torch.cuda.get_device_name(0),
                setting="CausalBGM use_bnn=False, Sim_Hirano_Imbens N=20000 p=200 seed 0, egm_init 30000 + fit 100 epochs (random_seed 123), "
                        "burn_in=%d n_keep=%d, same seed for all modes; seconds include the copy of the draws to the host" % (a.burn_in, a.n_mcmc),
                fit_s=fit_s, **res)


def part_panel(a):
    import torch
    from bayesgm_amd.models import CausalBGM
    from oracle import causal as OC
    from oracle.nets import mlp_forward
    z_dims, p, n = [3, 3, 3, 1], 50, a.n
    w = OC.init_model(0, z_dims, p, sigma_v=0.02, sigma_x=0.1, sigma_y=0.1)
    rs = np.random.RandomState(1)          # the model's own data at z ~ N(0, I): the posterior of a row is far narrower than the prior
    z = rs.randn(n, sum(z_dims)).astype(np.float32)
    z0, z1, z2 = OC.split_z(w, z)
    v = (mlp_forward(w["g"], z)[:, :p] + 0.02 * rs.randn(n, p)).astype(np.float32)
    x = (mlp_forward(w["h"], np.concatenate([z0, z2], axis=-1))[:, :1] + 0.1 * rs.randn(n, 1)).astype(np.float32)
    y = (mlp_forward(w["f"], np.concatenate([z0, z1, x], axis=-1))[:, :1] + 0.1 * rs.randn(n, 1)).astype(np.float32)
    with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CausalBGM(dict(PARAMS, z_dims=z_dims, v_dim=p, mixing_check=False, sigma_v=0.02, sigma_x=0.1, sigma_y=0.1),
                      timestamp="probe_causal_hmc_panel", random_seed=123)
        m.set_weights(g=w["g"], f=w["f"], h=w["h"], e=w["e"])
        res = _mixing(a, torch, m, (x, y, v), False)
    return dict(part="panel", device=torch.cuda.get_device_name(0),
                setting="concentrated panel: OC.init_model(0, [3,3,3,1], 50, sigma_v=0.02, sigma_x=0.1, sigma_y=0.1), %d rows of its own data "
                        "(seed 1), burn_in=%d n_keep=%d, same seed for all modes" % (n, a.burn_in, a.n_mcmc), **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("cost", "tutorial", "panel"), required=True)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--burn-in", type=int, default=5000)
    ap.add_argument("--n-mcmc", type=int, default=3000)
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--mh-transitions", type=int, default=200)
    ap.add_argument("--leapfrog", type=lambda s: [int(k) for k in s.split(",")], default=[1, 3, 5, 10])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--mass", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(cost=part_cost, tutorial=part_tutorial, panel=part_panel)[a.part](a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
