#!/usr/bin/env python3
"""Measurements of BGM's fused imputation with tail buffers (csrc/bgm_rowstep_kernels.h STEP 4, bgm_hmc_rows_impute_tails_kernel) on one GPU.

  --part cost     ms per retained transition over the whole retained phase in ONE launch (burn_in = 0, every iteration retained): the
                  impute kernel (hmc_run_rows with moments) over 1000 transitions, the tails kernel at K = tail_size(0.05, 1000) = 26
                  over 1000 and at K = tail_size(0.05, 5000) = 126 over 5000; N rows, L leapfrog steps, 50 % missing cells, p = 500 and
                  p = 100, fp32.  The arms alternate in one process after a warm-up, HIP events; per arm the repeats, median, min, max.
  --part whole    wall time, peak device memory (torch's allocator) and block count of the whole BGM.predict(row_adapt=True): the draws
                  route at its default max_draw_bytes, fused_predict=True alone and interval='tails', N rows, p = 500, burn-in +
                  retained iterations as given, at 90 % and at 10 % missing cells, the routes alternating; the bounds of 'tails' are
                  compared with the draws route's bit for bit in the same run.
  --part entries  entries per tail counted on the host from the cells of a small run (a value enters tail 0 after the fill when it is
                  strictly below the K-th smallest so far), against K ln(m / K).

    timeout -k 10 1100 python scripts/probe_bgm_impute_tails.py --part cost --out profiles/bgm_impute_tails_probe.json
Parts given one at a time merge into the same file.  Not measured here: more than one GPU, the class at n_mcmc = 5000.
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
from probe_bgm_fused_impute import _stats  # noqa: E402
from probe_bgm_row_step import _engine, _panel, _timed  # noqa: E402


def part_cost(a):
    import torch
    from bayesgm_amd import causal_hmc as HM
    from bayesgm_amd.engine import missing_slots
    out = dict(part="cost", device=torch.cuda.get_device_name(0), n=a.n, n_leapfrog=a.leapfrog, missing=0.5, reps=a.reps, cases=[])
    arms = [("impute", a.m_short, None), ("tails_K%d" % HM.tail_size(0.05, a.m_short), a.m_short, HM.tail_size(0.05, a.m_short)),
            ("tails_K%d" % HM.tail_size(0.05, a.m_long), a.m_long, HM.tail_size(0.05, a.m_long))]
    for p in a.ps:
        eng = _engine(p, "fp32")
        dev = eng.device
        x = torch.from_numpy(_panel(a.n, p, [0.5])[0]).to(dev)
        slot, k_slots = missing_slots(x)
        state, grad = (torch.empty((a.n, eng.q), device=dev) for _ in range(2))
        logp = torch.empty(a.n, device=dev)
        rows = torch.full((a.n,), 0.02, device=dev)
        mom = torch.full((3, a.n, p), float("nan"), device=dev)
        tails = {K: torch.empty((2, K, a.n, k_slots), device=dev) for _, _, K in arms if K}      # (retained draw 0 initialises the series)

        def run(m, K):
            kw = dict(slot=slot, k_slots=k_slots, tails=tails[K], k_tail=K) if K else {}
            eng.hmc_run_rows(x, state, logp, grad, rows, 0, m, 0, a.leapfrog, 7, init=True, moments=mom, n_keep=m, **kw)
        for _, m, K in arms:      # warm-up: a short launch of every arm
            run(min(m, max(20, K or 0) + 5), K)
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in arms}
        for _ in range(a.reps):
            for name, m, K in arms:
                ms[name].append(_timed(torch, lambda: run(m, K)) / m)
                print("p %d %s: %.4f ms per transition" % (p, name, ms[name][-1]), file=sys.stderr, flush=True)      # (a sign of life per launch)
        r = dict(p=p, k_slots=k_slots, transitions={name: m for name, m, _ in arms},
                 tails_gib={name: 8.0 * K * a.n * k_slots / 2.0 ** 30 for name, _, K in arms if K},
                 ms_per_transition={k: _stats(v) for k, v in ms.items()})
        base = r["ms_per_transition"]["impute"]["median"]
        r["over_impute"] = {k: v["median"] / base for k, v in r["ms_per_transition"].items() if k != "impute"}
        print(json.dumps(r), file=sys.stderr, flush=True)
        out["cases"].append(r)
        eng.close()
        del x, mom, tails, slot
        torch.cuda.empty_cache()
    return out


def _same(u, v):
    if isinstance(u, list):
        return len(u) == len(v) and all(np.array_equal(s, t) for s, t in zip(u, v))
    return np.array_equal(u, v)


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
            arms = dict(draws=dict(), fused=dict(fused_predict=True), tails=dict(fused_predict=True, interval="tails"))
            sec, mem, timing, blocks, same = {k: [] for k in arms}, {k: [] for k in arms}, {}, {}, []
            for rep in range(a.whole_reps):
                bounds = {}
                for k, extra in arms.items():
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    t0 = time.perf_counter()
                    _, bounds[k] = model.predict(x, **kw, **extra)
                    torch.cuda.synchronize()
                    sec[k].append(time.perf_counter() - t0)
                    mem[k].append(torch.cuda.max_memory_allocated() / 2.0 ** 30)
                    timing[k] = {n_: float(v) for n_, v in model.last_predict_timing.items()}
                    if k == "tails":
                        blocks[k] = model.impute_tail_blocks_
                    print("missing %.2f rep %d %s: %.2f s, peak %.2f GiB" % (share, rep, k, sec[k][-1], mem[k][-1]), file=sys.stderr, flush=True)
                same.append(bool(_same(bounds["draws"], bounds["tails"])))
                del bounds
            miss_row = np.isnan(x).sum(axis=1)
            k_slots = int(miss_row.max())
            per_row = 4 * a.n_mcmc * (q + k_slots)
            rows_blk = max(16, (64 << 30) // per_row)
            quantum = 16 * 24 * torch.cuda.get_device_properties(0).multi_processor_count
            rows_blk -= rows_blk % quantum if rows_blk > quantum else 0
            blocks["draws"], blocks["fused"] = -(-a.whole_n // rows_blk), 1
            r = dict(missing=share, k_slots=k_slots, seconds={k: _stats(v) for k, v in sec.items()}, peak_gib={k: _stats(v) for k, v in mem.items()},
                     blocks=blocks, tails_bounds_bit_equal_to_draws=same, last_phase_seconds=timing)
            r["draws_over_tails"] = r["seconds"]["draws"]["median"] / r["seconds"]["tails"]["median"]
            r["tails_over_fused"] = r["seconds"]["tails"]["median"] / r["seconds"]["fused"]["median"]
            print(json.dumps(r), file=sys.stderr, flush=True)
            out["cases"].append(r)
    return out


def part_entries(a):
    import torch
    from bayesgm_amd import causal_hmc as HM
    from bayesgm_amd.engine import missing_slots
    out = dict(part="entries", cases=[])
    p, n = 20, 64
    eng = _engine(p, "fp32")
    dev = eng.device
    x = torch.from_numpy(_panel(n, p, [0.5])[0]).to(dev)
    slot, k_slots = missing_slots(x)
    used = (torch.arange(k_slots, device=dev)[None, :] < torch.isnan(x).sum(dim=1)[:, None]).reshape(-1).cpu().numpy()
    for m in (a.m_short, a.m_long):
        K = HM.tail_size(0.05, m)
        state, grad = (torch.empty((n, eng.q), device=dev) for _ in range(2))
        cells = torch.zeros((n * k_slots, m), device=dev)
        eng.hmc_run_rows(x, state, torch.empty(n, device=dev), grad, torch.full((n,), 0.02, device=dev), 0, m, 0, a.leapfrog, 7, init=True,
                         moments=torch.full((3, n, p), float("nan"), device=dev), cells=cells, slot=slot, k_slots=k_slots, n_keep=m)
        c = cells.cpu().numpy()[used]
        counts = []
        for s in c:      # tail 0 of one series: the K smallest so far, its threshold their maximum
            held = np.sort(s[:K])
            cnt = 0
            for v in s[K:]:
                if v < held[-1]:
                    held[-1] = v
                    held.sort()
                    cnt += 1
            counts.append(cnt)
        r = dict(m=m, K=K, series=int(len(counts)), entries_after_fill_per_tail=_stats(counts), k_ln_m_over_k=float(K * np.log(m / K)),
                 share_of_draws_entering_a_tail=float(2 * (np.mean(counts) + K) / m))
        r["entries_after_fill_per_tail"].pop("values")
        r["entries_after_fill_per_tail"]["mean"] = float(np.mean(counts))
        print(json.dumps(r), file=sys.stderr, flush=True)
        out["cases"].append(r)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("all", "cost", "whole", "entries"), default="all")
    ap.add_argument("--n", type=int, default=200000, help="rows of the cost part")
    ap.add_argument("--ps", type=int, nargs="+", default=[500, 100])
    ap.add_argument("--m-short", type=int, default=1000)
    ap.add_argument("--m-long", type=int, default=5000)
    ap.add_argument("--leapfrog", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--whole-n", type=int, default=200000)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--n-mcmc", type=int, default=1000)
    ap.add_argument("--whole-reps", type=int, default=5)
    ap.add_argument("--shares", type=float, nargs="+", default=[0.9, 0.1])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(not_measured=["more than one GPU", "the class at n_mcmc = 5000"])
    if a.out and os.path.exists(a.out):      # (parts run one at a time merge into one file)
        with open(a.out) as f:
            res.update(json.loads(f.read()))
    for part, fn in (("entries", part_entries), ("cost", part_cost), ("whole", part_whole)):
        if a.part in ("all", part):
            res[part] = fn(a)
            if a.out:      # (after every part: a later part that runs out of time loses nothing)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
