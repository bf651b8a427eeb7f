"""bench.py launches its own ranks: a bare `python bench.py --gpus N` (no WORLD_SIZE in the environment) re-executes itself as N ranks
under torch.distributed.run on 127.0.0.1 and refuses to time anything unless N ranks answer the all-reduce (VERDICT round 4, item 1;
SURVEY.md 8e).  The CPU tests use --plumbing-only (gloo, no device); the GPU test runs the real step with both ranks on device 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bare(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3])
def test_bare_invocation_spawns_the_ranks(n):
    r = _bare(["--gpus", str(n), "--plumbing-only", "--rows", "1001", "--scaling", "strong"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == n and d["n_ranks_in_collective"] == n
    rows = d["rows"]
    assert sum(r_[0] for r_ in rows) == 1001 and [r_[1] for r_ in rows] == [sum(x[0] for x in rows[:i]) for i in range(n)]


def test_weak_scaling_plan_and_single_rank():
    d = _json_line(_bare(["--gpus", "2", "--plumbing-only", "--rows", "500"]).stdout)
    assert d["rows"] == [[500, 0, 1000], [500, 500, 1000]]
    d = _json_line(_bare(["--plumbing-only", "--rows", "500"]).stdout)
    assert d["n_gpus"] == 1 and d["rows"] == [[500, 0, 500]]


def test_gpus_must_match_world_size():
    r = _bare(["--gpus", "2", "--plumbing-only"], env_extra={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_refuses_more_ranks_than_devices():
    import torch
    n = torch.cuda.device_count() + 1 if torch.cuda.is_available() else 2
    r = _bare(["--gpus", str(n), "--rows", "100"])
    assert r.returncode == 2 and "refusing" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_bare_two_rank_bench_on_one_device():
    """the whole step (sharded predict, ADRF all-reduce, max-over-ranks timing) from the driver's bare command form; both ranks on GPU 0
    over gloo -- the RCCL form of the same launch is tests/test_gpu_rccl.py, which needs two devices"""
    r = _bare(["--gpus", "2", "--rows", "4096", "--burn-in", "40", "--n-mcmc", "20", "--steps", "1", "--warmup", "1", "--full"],
              env_extra={"BGM_BENCH_SINGLE_DEVICE": "1", "BGM_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["n_ranks_in_collective"] == 2 and d["config"]["rows_total"] == 8192
    assert d["value"] > 0 and d["roofline"]["frac"] > 0
    # the fit side of configs[3]: the data-parallel minibatch loop with its per-step gradient all-reduce, on every rank (over gloo on
    # one device the per-minibatch host loop; over RCCL bgm_causal_fit_epoch_dp -- tests/test_gpu_rccl.py, tests/test_gpu_comm.py)
    f = d["fit_dp"]
    assert "error" not in f, f
    assert f["n_ranks_in_collective"] == 2 and f["global_minibatch"] == 64 and f["us_per_minibatch"] > 0 and 0 < f["allreduce_share_of_minibatch"] < 1


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    """a plain run is the headline alone (the secondary legs need --full); --dump-outputs writes the last timed step's ADRF and interval,
    the same from run to run (seeded panel, weights and Philox streams)"""
    got = []
    for k in range(2):
        r = _bare(["--rows", "4096", "--burn-in", "40", "--n-mcmc", "20", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / str(k))])
        assert r.returncode == 0, r.stderr[-3000:]
        d = _json_line(r.stdout)
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["roofline"]["frac"] > 0
        assert d["kernel_paths"] is None and not {"cpu_baseline", "outcome_cache", "fit", "fit_dp", "accuracy"} & set(d)
        got.append({n: np.load(str(tmp_path / str(k) / (n + ".npy"))) for n in ("adrf", "interval")})
    assert got[0]["adrf"].shape == (20,) and got[0]["interval"].shape == (20, 2)
    assert [float(a) for a in got[1]["adrf"][:3]] == d["adrf_head"]      # the ADRF of the line's last timed step
    for n in got[0]:
        assert got[0][n].dtype == np.float32 and np.array_equal(got[0][n], got[1][n])
