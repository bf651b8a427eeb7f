"""Timing of estimate_latent_dims at the headline panel shape (N = 1e6, p = 200; labelings of 10 slices for y and for x):
the moment kernel alone (HIP events), the whole function on device-resident inputs and on host NumPy inputs, and the FP64
matrix rate of the chip (v_mfma_f64_16x16x4_f64 back to back, probe library).

    python scripts/probe_latent_dims.py [--n 1000000] [--p 200] [--reps 20] [--out profiles/latent_dims_probe_N1e6_p200.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--p", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bayesgm_amd import _lib
    from bayesgm_amd import latent_dims as LD
    from bayesgm_amd.datasets import Sim_Hirano_Imbens_sampler

    x, y, v = Sim_Hirano_Imbens_sampler(N=a.n, v_dim=a.p, seed=0).load_all()
    n, p = v.shape
    dev = torch.device("cuda", 0)
    xd, yd, vd = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (x, y, v))
    res = {"n": n, "p": p, "device": torch.cuda.get_device_name(0)}

    # the kernel alone (moments pass: sdr_moments_kernel + sdr_reduce_kernel)
    lab_y, cnt_y = LD._device_slices(yd[:, 0], 10)
    lab_x, cnt_x = LD._device_slices(xd[:, 0], 10)
    s = (cnt_y.shape[0], cnt_x.shape[0])
    lib = _lib.load()
    h = LD._handle(0)
    ws_bytes = C.c_int64()
    _lib.check(lib.bgm_sdr_moments_workspace(h, n, p, s[0], s[1], C.byref(ws_bytes)), "ws")
    ws = torch.empty(ws_bytes.value // 8, dtype=torch.float64, device=dev)
    out = torch.empty((1 + s[0] + s[1]) * p + p * p, dtype=torch.float64, device=dev)
    shift = vd[0].double().contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        _lib.check(lib.bgm_sdr_moments(h, C.c_void_p(vd.data_ptr()), 0, n, p, p, C.c_void_p(shift.data_ptr()),
                                       C.c_void_p(lab_y.data_ptr()), s[0], C.c_void_p(lab_x.data_ptr()), s[1],
                                       C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes.value, stream), "moments")
    for _ in range(3):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.reps):
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    kernel_ms = float(np.median(times))
    flop = 2.0 * n * (p * (p + 1) / 2 + (1 + s[0] + s[1]) * p)
    bytes_read = float(n * p * v.itemsize + 2 * n * 4)
    res.update(kernel_ms_median=kernel_ms, kernel_ms_min=float(np.min(times)), slices=list(s), workspace_mb=ws_bytes.value / 2 ** 20,
               algorithmic_flop=flop, kernel_tflops=flop / (kernel_ms * 1e-3) / 1e12, bytes_read=bytes_read,
               kernel_read_gbps=bytes_read / (kernel_ms * 1e-3) / 1e9)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(3, a.reps // 4)):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3, r

    res["function_device_ms"], res["dims_device"] = timed(lambda: LD.estimate_latent_dims(xd, yd, vd))
    res["function_host_ms"], res["dims_host"] = timed(lambda: LD.estimate_latent_dims(x, y, v))

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _probe_lib import load as load_probe
    pl = load_probe()
    rates = {}
    for wpc in (4, 8):
        tf = C.c_double()
        rc = pl.bgm_probe_mfma_f64(0, wpc, 20000, C.byref(tf))
        rates["waves_per_cu_%d" % wpc] = tf.value if rc == 0 else None
    res["fp64_mfma_tflops_measured"] = rates
    peak = max(t for t in rates.values() if t)
    res["kernel_share_of_measured_fp64_rate"] = res["kernel_tflops"] / peak
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
