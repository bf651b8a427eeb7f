"""Device side of tests/test_gpu_bvn_edges.py: the runs of a case through BvnEngine, shared by the test process and by the child processes
that force a route.  BGM_BVN_NO_TILES is read once per process (csrc/bgmb_api.hip), so the runs with the workspace kernel forced for frozen
noise happen here as a program of their own:

    python tests/_bvn_edges_helper.py OUT.npz A        every frozen-noise case of part A
    python tests/_bvn_edges_helper.py OUT.npz B        the row-count panels of part B

with whatever switches the environment of the process holds; the arrays go to OUT.npz under "<case>/<array>"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bvn_edges_ref as V  # noqa: E402

CHAIN_KEYS = ("state", "logp", "grad", "draws", "acc")


def n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def engine(c, frozen, **kw):
    """An open session of the case's (or V.SMALL's) generator."""
    from bayesgm_amd.bvn_engine import BvnEngine
    eng = BvnEngine(c["p"], c["q"], g_units=c["units"], hmc_frozen_noise=frozen, **kw)
    eng.begin(V.case_net(c))
    return eng


def run_chain(eng, x, seed, row_base, step, leap, n_first, n_more):
    """hmc_run at a fixed step: the bootstrap evaluation and n_first transitions, then n_more from the stored state with their draws kept.
    x: the rows on the device.  -> dict of CHAIN_KEYS (NumPy)."""
    import torch
    dev, n, q = eng.device, x.shape[0], eng.q
    state, logp, grad = torch.empty((n, q), device=dev), torch.empty(n, device=dev), torch.empty((n, q), device=dev)
    stp = torch.full((1,), float(step), device=dev)
    draws = torch.empty((n_more, n, q), device=dev)
    acc = torch.zeros(n_first + n_more, device=dev, dtype=torch.int32)
    eng.hmc_run(x, state, logp, grad, stp, 0, n_first, n_first, leap, seed, init=True, row_base=row_base, acc_count=acc, draws=None)
    if n_more:
        eng.hmc_run(x, state, logp, grad, stp, n_first, n_more, n_first, leap, seed, row_base=row_base, acc_count=acc, draws=draws)
    return dict(state=state.cpu().numpy(), logp=logp.cpu().numpy(), grad=grad.cpu().numpy(), draws=draws.cpu().numpy(), acc=acc.cpu().numpy())


def run_case(c):
    """A part A case on the route the environment leaves it."""
    import torch
    eng = engine(c, c["frozen"])
    try:
        x = torch.from_numpy(np.array(V.panel(c["n"], c["p"], c["data_seed"]))).to(eng.device)
        return run_chain(eng, x, c["seed"], c["row_base"], c["step"], c["leap"], c["n_first"], c["n_more"])
    finally:
        eng.close()


def b_panels(cus):
    """{name: (n, tile rows of the launch, workgroups of the launch)} of the workspace kernel's row-count panels."""
    out = {"rt%d" % rt: (n,) + V.workspace_grid(n, cus)[::2] for rt, n in V.rt_rows(cus).items()}
    n = V.rows_workspace_trips(cus)
    out["trips"] = (n,) + V.workspace_grid(n, cus)[::2]
    return out


def b_tiles(name, n, rt, grid):
    """The tiles of a panel that are also run alone and meet the oracle."""
    n_tiles = (n + rt - 1) // rt
    return sorted(set(V.sampled_tiles(n, rt, grid)) | {n_tiles // 2})


def run_rows(eng, xd, tiles, rt, n):
    """B_ITERS transitions after the bootstrap for the whole panel in one launch, then for each of `tiles` as a launch of its own with
    the matching row_base.  -> whole (dict), {tile: dict}."""
    whole = run_chain(eng, xd, V.B_SEED, V.B_ROW_BASE, V.B_STEP, V.B_LEAP, V.B_ITERS, 0)
    alone = {}
    for t in tiles:
        lo, hi = t * rt, min(n, (t + 1) * rt)
        alone[t] = run_chain(eng, xd[lo:hi].contiguous(), V.B_SEED, V.B_ROW_BASE + lo, V.B_STEP, V.B_LEAP, V.B_ITERS, 0)
    return whole, alone


def main(out, job):
    import torch
    res = {}
    if job == "A":
        for c in V.A_CASES:
            if c["frozen"]:
                for k, v in run_case(c).items():
                    res["%s/%s" % (c["name"], k)] = v
    else:
        cus = n_cus()
        eng = engine(V.SMALL, True)
        for name, (n, rt, grid) in b_panels(cus).items():
            xd = torch.from_numpy(np.array(V.panel(n, V.SMALL["p"], 31))).to(eng.device)
            whole, alone = run_rows(eng, xd, b_tiles(name, n, rt, grid), rt, n)
            for k in ("state", "logp", "grad", "acc"):
                res["%s/%s" % (name, k)] = whole[k]
                for t, r in alone.items():
                    res["%s/%d/%s" % (name, t, k)] = r[k]
        eng.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
