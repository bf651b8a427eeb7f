"""Timing of the chain-diagnostics kernels alone at the shape of one metropolis_hastings_sampler block (n_keep = 3000 draws of
n = 10 000 rows x q = 10 latents, max_lag = 256), HIP events around repeated launches after warm-up, with two floors: one read of
the draws at the copy bandwidth measured here, and the float64 fused multiply-adds of the lag sums at the chip's vector float64
rate (256 CUs x 4 SIMDs x 16 lanes per clock at the clock the device reports).

    python scripts/probe_chain_diag.py [--n-keep 3000] [--n 10000] [--q 10] [--max-lag 256] [--reps 20] [--out profiles/chain_diag_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-keep", type=int, default=3000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--q", type=int, default=10)
    ap.add_argument("--max-lag", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayesgm_amd import _lib
    from bayesgm_amd.latent_dims import _handle

    dev = torch.device("cuda", 0)
    n_series = a.n * a.q
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    # sticky chains: every series holds a value for 1 .. 40 iterations (the kernel's time does not depend on the values)
    hold = torch.randint(1, 41, (n_series,), device=dev, generator=g)
    step = torch.arange(a.n_keep, device=dev)[:, None] // hold[None, :]
    base = torch.randn((a.n_keep, n_series), device=dev, generator=g)
    draws = torch.gather(base, 0, step).contiguous()
    del base, step
    lib = _lib.load()
    h = _handle(0)
    ws_bytes = C.c_int64()
    _lib.check(lib.bgm_chain_diagnostics_workspace(h, 1, a.n_keep, n_series, a.max_lag, C.byref(ws_bytes)), "ws")
    ws = torch.empty(ws_bytes.value // 8, dtype=torch.float64, device=dev)
    out = torch.empty((6, n_series), dtype=torch.float64, device=dev)
    flags = torch.empty(n_series, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        _lib.check(lib.bgm_chain_diagnostics(h, C.c_void_p(draws.data_ptr()), 1, a.n_keep, n_series, a.max_lag, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(flags.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes.value, stream), "diag")

    def timed(fn, reps):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(np.min(ts))

    ms, ms_min = timed(launch, a.reps)
    dst = torch.empty_like(draws)
    copy_ms, _ = timed(lambda: dst.copy_(draws), a.reps)
    draws_bytes = float(draws.numel() * 4)
    copy_gbps = 2.0 * draws_bytes / (copy_ms * 1e-3) / 1e9                 # a copy reads and writes every byte
    h2 = a.n_keep // 2
    lag = min(a.max_lag, h2 - 1)
    n_lags = 2 * ((lag + 1) // 2)
    fma = float(n_series) * 2 * sum(h2 - k for k in range(n_lags))         # products that enter acov(0 .. n_lags - 1)
    fma_issued = float(n_series) * 2 * (-(-h2 // 8) * 8) * (-(-n_lags // 16) * 16)   # what the kernel executes (zero-padded tails)
    prop = torch.cuda.get_device_properties(0)
    clock_ghz = prop.clock_rate / 1e6 if hasattr(prop, "clock_rate") else 2.4
    f64_fma_per_s = prop.multi_processor_count * 4 * 16 * clock_ghz * 1e9
    floor_read_ms = draws_bytes / (copy_gbps * 1e9) * 1e3
    floor_fma_ms = fma / f64_fma_per_s * 1e3
    s = out.cpu().numpy()
    res = dict(device=torch.cuda.get_device_name(0), n_keep=a.n_keep, n=a.n, q=a.q, n_series=n_series, max_lag=a.max_lag, reps=a.reps,
               kernel_ms_median=ms, kernel_ms_min=ms_min, draws_bytes=draws_bytes, workspace_mb=ws_bytes.value / 2 ** 20,
               copy_ms_median=copy_ms, copy_gbps=copy_gbps, floor_read_ms=floor_read_ms,
               f64_fma=fma, f64_fma_issued=fma_issued, clock_ghz=clock_ghz, compute_units=prop.multi_processor_count,
               vector_f64_fma_per_s=f64_fma_per_s, floor_fma_ms=floor_fma_ms,
               ratio_to_larger_floor=ms / max(floor_read_ms, floor_fma_ms),
               achieved_f64_tflops_issued=2 * fma_issued / (ms * 1e-3) / 1e12,
               ess_median=float(np.nanmedian(s[3])), share_truncated=float(((flags.cpu().numpy() & 2) != 0).mean()))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
