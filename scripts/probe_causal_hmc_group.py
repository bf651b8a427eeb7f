#!/usr/bin/env python3
"""Measurements of the CausalBGM HMC sampler that sums the individual treatment effect by row label (csrc/causal_hmc_gfx_kernels.h)
on one GPU.  The setup of scripts/probe_causal_hmc_rowfx.py: ONE process, the arms alternated (order rotated every repeat) after a
warm-up call of each; p = 200, z_dims [1, 1, 1, 7], random weights, the Hirano-Imbens panel with the treatment cut at its median
(a binary treatment), n_leapfrog 5; HIP events around the whole hmc_sample call (Gram pre-pass, LDS fills and the allocation of the
outputs included in every arm), burn_in = 0 so that every transition is retained; --reps repeats, median / min / max of ms per
retained transition.

  arms at every --n     ite           hmc_sample(effect=EFFECT_ITE): the fused ITE kernel (causal_hmc_fx_kernels.h; its code object
                                      is the parent library's, scripts/compare_code_objects.py), storing [n, transitions]
                        one_group     hmc_sample(effect=EFFECT_GROUP_ITE), labels 2 * group + x_i: one group (2 labels)
                        sorted_16     16 groups of consecutive rows (32 labels; a tile holds one group, two labels)
                        random_16     16 groups drawn at random per row (32 labels; the worst case of the label walk)
  at --long-n only      the same four arms with --long-transitions retained transitions in one launch: the per-call host work
                        (the labels' copy and check, the partials' allocation and reduction, for the ITE arm its matrix) is
                        spread over ten times as many transitions
  --memory-n            peak device memory (torch's allocator) of predict_average against predict(sampler='hmc',
                        fused_effects=True) with --memory-draws retained draws and --memory-burn burn-in iterations, and the rows
                        per launch the 32 GiB cap on the ITE matrix leaves each route

    timeout -k 10 900 python scripts/probe_causal_hmc_group.py --out profiles/causal_hmc_group_probe.json
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

Z_DIMS, P, LEAPFROG = [1, 1, 1, 7], 200, 5
PARAMS = dict(dataset="Sim_Hirano_Imbens", output_dir=".", save_res=False, save_model=False, binary_treatment=True, use_bnn=False,
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
        return CausalBGM(dict(PARAMS), timestamp="probe_causal_hmc_group", random_seed=0)


def _panel(n):
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler
    x, y, v = Sim_Hirano_Imbens_sampler(N=n, v_dim=P, seed=0).load_all()
    x = (x > np.median(x)).astype(np.float32)
    return x, np.asarray(y, np.float32), np.asarray(v, np.float32)


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
    from bayesgm_amd import causal_hmc as HM
    x, y, v = _panel(n)
    eng = model.engine
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(eng.device) for t in (x, y, v))
    xd, yd = xd.reshape(-1), yd.reshape(-1)
    run = lambda kw, its: eng.hmc_sample(xd, yd, vd, 0, its, 0.1, LEAPFROG, 7, adapt=None, **kw)      # burn_in = 0: every transition is retained
    rows = np.arange(n)
    groups = dict(one_group=np.zeros(n, np.int64), sorted_16=rows * 16 // n, random_16=np.random.RandomState(1).randint(0, 16, n))
    arms = dict(ite=dict(effect=_lib.EFFECT_ITE))
    for name, g in groups.items():
        lab = torch.from_numpy(HM.average_labels(g, x)).to(eng.device)                               # (checked on the host in every call)
        arms[name] = dict(effect=_lib.EFFECT_GROUP_ITE, labels=lab, n_labels=2 * (int(g.max()) + 1))
    ms = _alternate(torch, run, arms, a.transitions, a.reps, dict(part="transition", n=n))
    res = dict(n=n, transitions_per_launch=a.transitions, ms_per_retained_transition=ms,
               over_ite={name: ms[name]["median"] / ms["ite"]["median"] for name in groups},
               ite_matrix_bytes=n * a.transitions * 4)
    if n == a.long_n:
        its = a.long_transitions
        ms = _alternate(torch, run, arms, its, a.reps, dict(part="long", n=n))
        res["long"] = dict(transitions_per_launch=its, ms_per_retained_transition=ms,
                           over_ite={name: ms[name]["median"] / ms["ite"]["median"] for name in groups}, ite_matrix_bytes=n * its * 4)
    return res


def part_memory(a, torch, model):
    n, keep, burn = a.memory_n, a.memory_draws, a.memory_burn
    data = _panel(n)
    kw = dict(n_mcmc=keep, burn_in=burn, verbose=0, step_size=0.1, n_leapfrog=LEAPFROG)
    res = dict(n=n, n_mcmc=keep, burn_in=burn)
    for name, call in (("predict_average", lambda: model.predict_average(data, **kw)),
                       ("predict_fused", lambda: model.predict(data, sampler="hmc", fused_effects=True, **kw))):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            call()
        torch.cuda.synchronize()
        res[name] = dict(seconds=time.perf_counter() - t0, peak_device_bytes=int(torch.cuda.max_memory_allocated() - base))
        print(json.dumps(dict(part="memory", arm=name, **res[name])), file=sys.stderr, flush=True)
    cap_rows = (32 << 30) // (4 * keep)
    res["rows_per_launch_under_the_32GiB_cap"] = dict(
        predict_fused=int(cap_rows), predict_average_mh=int(cap_rows),
        predict_average_hmc="no [n x n_mcmc] matrix: a shard of any size is one launch; group_partial is n_slots * n_mcmc * n_labels * 4 bytes")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=lambda s: [int(float(k)) for k in s.split(",")], default=[1000000, 100000])
    ap.add_argument("--transitions", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long-n", type=lambda s: int(float(s)), default=100000, help="the one N at which the long launches run")
    ap.add_argument("--long-transitions", type=int, default=200)
    ap.add_argument("--memory-n", type=lambda s: int(float(s)), default=1000000, help="0: skip the memory part")
    ap.add_argument("--memory-draws", type=int, default=3000)
    ap.add_argument("--memory-burn", type=int, default=50, help="the peaks do not depend on it: nothing is stored before burn_in")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    model = _model()
    res = dict(device=torch.cuda.get_device_name(0), p=P, z_dims=Z_DIMS, n_leapfrog=LEAPFROG,
               method="one process, arms alternated (order rotated every repeat) after a warm-up call of each; HIP events around "
                      "hmc_sample, burn_in = 0",
               transition=[part_transition(a, torch, model, n) for n in a.n])
    res["memory"] = part_memory(a, torch, model) if a.memory_n > 0 else "not measured"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
