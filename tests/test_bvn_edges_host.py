"""What the cases of tests/test_gpu_bvn_edges.py reach, shown without a device from the restated host plans of tests/_bvn_edges_ref.py
(bgmb_fill / bnn_finish_net, bgmf_session, gxf_session, bvn_rt and the grid caps of csrc/bgmb_api.hip and csrc/bgmf_api.hip), and the
conditions the float64 oracle alone puts on their inputs: flagged rows, accepted and rejected proposals, the cost of float32, the raw
variance head."""
import os
import re

import numpy as np
import pytest

import _bvn_edges_ref as V
from oracle import rng as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUS = 256          # compute units of an MI355X: the panel sizes below assume it (the GPU file takes the device's own count)

ids = [c["name"] for c in V.A_CASES]


# ---------------------------------------------------------------------------------------------------------------------------
# the plans
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", V.A_CASES, ids=ids)
def test_sign_layout_is_the_oracles(c):
    assert V.fill_ok(c["q"], c["units"], c["p"])
    assert V.sign_words(c["q"], c["units"], c["p"]) == tuple(V.sign_layout_oracle(c["q"], c["units"], c["p"]))


@pytest.mark.parametrize("c", V.A_CASES, ids=ids)
def test_case_reaches_what_its_table_entry_names(c):
    q, u, p, fz = c["q"], c["units"], c["p"], c["frozen"]
    assert V.route(q, u, p, fz) == c["want"]
    f, g = V.bgmf_plan(q, u, p), V.gxf_plan(q, u, p)
    if c["want"] == "chains":
        assert (f.ktq, f.nh) == (c["ktq"], c["nh"]) and f.fits
        assert V.route(q, u, p, fz, no_chains=True) == ("tiles" if fz else "workspace")
    if c["want"] == "tiles":
        assert g.fits and (f is None or not f.fits)
        assert V.route(q, u, p, fz, no_chains=True) == "tiles"
        for key in ("occ", "ld"):
            if key in c:
                assert getattr(g, key) == c[key], (key, getattr(g, key))
        if "chunks" in c:
            assert g.chunks == c["chunks"]
        if "n_chunks" in c:
            assert len(g.chunks) == c["n_chunks"]
    if c["want"] == "workspace" and fz:
        assert g is not None and not g.fits and f is None
    if fz:
        assert V.route(q, u, p, fz, no_tiles=True) == "workspace"
    assert V.bvn_rt(c["n"], N_CUS) == 16 and V.workspace_grid(c["n"], N_CUS) == (16, 3, 3)          # 33 rows: tiles of 16, 16 and 1
    assert V.gxf_grid(c["n"], N_CUS, 1) == 2 and V.bgmf_grid(c["n"], N_CUS) == 1                       # ... of 32 and 1; three 16-row tiles of one workgroup


def test_one_predicate_off_the_chains_each():
    base = dict(q=10, units=V.H64(5), p=20)
    assert V.bgmf_plan(**base).fits
    off = {c["off"]: c for c in V.A_CASES if "off" in c and c["name"].startswith(("off-", "lds-first"))}
    assert set(off) == {"q", "depth", "width", "lds"}
    for c in V.A_CASES:
        if "off" not in c:
            continue
        changed = [k for k, same in (("q", c["q"] <= 32), ("depth", len(c["units"]) in (3, 5)), ("width", all(w == 64 for w in c["units"])),
                                     ("lds", V.bgmf_plan(10, V.H64(5), c["p"]).fits)) if not same]
        assert changed == [c["off"]], (c["name"], changed)


def test_every_instantiation_and_both_occupancies_are_met():
    chains = {(c["ktq"], c["nh"], c["frozen"]) for c in V.A_CASES if c["want"] == "chains"}
    assert chains == {(k, h, f) for k in (1, 2) for h in (3, 5) for f in (True, False)}
    tiles = [V.gxf_plan(c["q"], c["units"], c["p"]) for c in V.A_CASES if c["want"] == "tiles"]
    assert {1, 3} <= {g.occ for g in tiles}
    assert any(len(g.chunks) == 1 for g in tiles) and any(len(g.chunks) > 1 and g.Pp % g.ch for g in tiles)          # a ragged last chunk
    assert any(len(c["units"]) == 1 for c in V.A_CASES if c["want"] == "tiles")                                    # T = 1: no backward trunk loop
    assert any(len(c["units"]) == V.BNN_MAX_LAYERS - 2 for c in V.A_CASES) and not V.fill_ok(4, (32,) * 7, 12)
    assert sum(c["want"] == "workspace" and c["frozen"] for c in V.A_CASES) == 3
    assert all(any(w % 64 for w in c["units"]) for c in V.A_CASES if c["want"] == "workspace" and not c["frozen"])


def test_switch_points_found_by_search():
    """The figures of the issue are a cross-check of the search, not its source."""
    f = V.bgmf_plan
    assert V.P_DECLINE == V.first_p_declined(10, V.H64(5)) == 897
    assert f(10, V.H64(5), 896).lds_bytes == 163200 and f(10, V.H64(5), 897).lds_bytes == 165376
    assert V.first_p_declined(32, V.H64(5)) == 641 and V.first_p_declined(10, V.H64(3)) == 1857
    # by exhaustion around the switch: the LDS need does not shrink as p grows
    need = [f(10, V.H64(5), p).lds_bytes for p in range(1, 1200)]
    assert all(a <= b for a, b in zip(need, need[1:]))
    g = V.gxf_plan
    assert g(10, (256,) * 3, 100).lds_bytes == 163536 and g(10, (256,) * 3, 100).fits
    assert g(10, (256,) * 5, 8).lds_bytes == 174800 and not g(10, (256,) * 5, 8).fits
    # the widest one-layer trunk the tiles hold: by search over the width
    q, p = 5, 20
    w = max(w for w in range(1, 600) if g(q, (w,), p).fits)
    assert w == 256 and g(q, (257,), p).ld == V.gx_ld(V.gx_pad32(257)) == 328 and g(q, (257,), p).lds_bytes > V.LDS_LIMIT
    assert g(10, (257,), 8).lds_bytes == 184016
    assert V.gxf_plan(5, (32,) * 9, 8) is None          # too deep for the tiles (bgmb_fill refuses it before)
    t = g(5, (130,), 300)
    assert (t.ld, t.ch, t.Pp, t.chunks, t.occ) == (200, 192, 320, [192, 128], 1)
    assert g(3, (16, 16), 8).occ == 3 and g(5, (24, 40), 100).occ == 3


def test_row_tile_ladder_and_grid_caps():
    rows = V.rt_rows(N_CUS)
    assert sorted(rows) == [16, 32, 48, 64]
    for rt, n in rows.items():
        assert V.bvn_rt(n, N_CUS) == rt and n % rt == 1
        assert rt == 64 or V.bvn_rt(n + rt, N_CUS) == rt + 16          # the largest such panel of the rung
        assert V.workspace_grid(n, N_CUS) == (rt, N_CUS, N_CUS)
    assert V.bvn_rt(1, N_CUS) == 16 and V.bvn_rt(140000, N_CUS) == 64          # (the two rungs tests/test_gpu_bgm_bnn.py uses)
    n = V.rows_workspace_trips(N_CUS)
    rt, n_tiles, grid = V.workspace_grid(n, N_CUS)
    assert (rt, grid, n_tiles) == (64, 8 * N_CUS, 2 * 8 * N_CUS + 2) and n - (n_tiles - 1) * rt == 1
    assert V.sampled_tiles(n, rt, grid) == [0, grid - 1, grid, 2 * grid - 1, 2 * grid, 2 * grid + 1]
    occ = V.gxf_plan(V.SMALL["q"], V.SMALL["units"], V.SMALL["p"]).occ
    assert occ == 3 and V.route(V.SMALL["q"], V.SMALL["units"], V.SMALL["p"], True) == "tiles"
    n = V.rows_tiles_trips(N_CUS, occ)
    grid = V.gxf_grid(n, N_CUS, occ)
    assert grid == occ * N_CUS and (n + 31) // 32 == 2 * grid + 2 and n % 32 == 1
    nd = V.decode_draws(N_CUS)
    tiles, grid = V.decode_grid(V.D_ROWS, nd, N_CUS)
    assert tiles == 3 * nd and grid == 4 * N_CUS and tiles > 2 * grid and V.D_ROWS == 64 + 64 + 2
    assert V.decode_refused(V.D_ROWS, 3, 1 << 31, 0) and not V.decode_refused(V.D_ROWS, 3, 1000, 40)
    assert V.C_BATCHES[0] == 2 and V.C_BATCHES[-1] == V.MAX_BATCH


def test_workspace_slices_stay_below_one_gib():
    q, u, p = V.SMALL["q"], V.SMALL["units"], V.SMALL["p"]
    wmax = max([2 * p, q] + list(u))
    shapes = V.flip_shapes(q, u, p)
    dims = [q] + list(u) + [p, p]
    hoff_total, hs_total = sum(dims), sum(dims) + u[-1]
    cache = 64 * q + 3 * q + 64 * (hoff_total + hs_total) + 2 * sum(a * b for a, b in shapes) + 64 * V.sign_words(q, u, p)[2] + 64          # bnn_cache_floats
    tile = 64 * (6 * q + 2 * p + 4 * wmax) + 96 + cache                                                                                      # bgmb_tile_floats
    assert 4 * ((tile + 63) & ~63) * 8 * N_CUS < (1 << 30)


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs, from the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", V.A_CASES, ids=ids)
def test_chain_case_is_a_fair_case(c):
    r = V.ref_chain(c["name"])
    n = c["n"]
    print("BVN-EDGE-HOST case=%s flagged=%d accepted=%s s_min=%.2f lp_max=%.1f" % (c["name"], r.flagged.sum(), r.acc.sum(axis=1).tolist(), r.s_min, r.lp_max))
    assert r.flagged.sum() <= V.CAP_A * n
    assert 0 < r.acc.sum() < r.acc.size and (r.acc.sum(axis=0) > 0).any() and (~r.acc).any()
    assert r.s_min > -3.0
    x = V.panel(n, c["p"], c["data_seed"])
    assert np.isnan(x[V.ROW_MISSING]).all() and not np.isnan(x[V.ROW_FULL]).any()
    assert 0.15 < np.isnan(x).mean() < 0.4
    rows = np.arange(n)
    z0 = R.normals(c["row_base"] + rows, 0, c["q"], R.TAG_INIT, c["seed"])
    l64, g64, _ = V.logpost_rows(V.case_net(c), z0, x, rows, c["seed"], 0, c["row_base"])
    l32, _, _ = V.logpost_rows(V.case_net(c), z0, x, rows, c["seed"], 0, c["row_base"], np.float32)
    assert np.abs(l32 - l64).max() <= 0.25 * 1e-5 * np.abs(l64).max()
    # no observed cell: the posterior is the prior
    np.testing.assert_allclose(l64[V.ROW_MISSING], -0.5 * (z0[V.ROW_MISSING].astype(np.float64) ** 2).sum(), rtol=1e-12)
    np.testing.assert_allclose(g64[V.ROW_MISSING], -z0[V.ROW_MISSING], rtol=1e-12)


def test_subset_of_rows_gives_the_rows_own_chains():
    c = V.A_BY_NAME["ws-24-40-p37-fresh"]
    r = V.ref_chain(c["name"])
    rows = np.array([0, 3, 17, 32])
    s = V.chains64(V.case_net(c), V.panel(c["n"], c["p"], c["data_seed"]), rows, c["seed"], c["row_base"], c["step"], c["leap"],
                   c["n_first"] + c["n_more"], c["n_first"], c["frozen"])
    np.testing.assert_allclose(s.state, r.state[rows], rtol=0, atol=1e-12)          # (the matrix products sum in another order)
    np.testing.assert_allclose(s.draws, r.draws[:, rows], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(s.acc, r.acc[:, rows])


def test_chains64_is_the_oracles_sampler():
    """chains64 at a fixed step against oracle/bgm_bnn.py::hmc_sampler without adaptation (burn_in < 2: n_adapt = 0)."""
    from oracle import bgm_bnn as OV
    for name in ("tiles-16-T1", "ws-24-40-p37-fresh"):
        c = V.A_BY_NAME[name]
        x = V.panel(c["n"], c["p"], c["data_seed"])
        xc, mk = V.split_nan(x)
        step = float(np.float32(c["step"]))
        ref = OV.hmc_sampler(OV.cast_vnet(V.case_net(c), np.float64), xc, mk, 4, 1, step, c["leap"], c["seed"], row0=c["row_base"], frozen=c["frozen"])
        got = V.chains64(V.case_net(c), x, np.arange(c["n"]), c["seed"], c["row_base"], c["step"], c["leap"], 5, 1, c["frozen"])
        np.testing.assert_array_equal(got.draws, ref)


def _b_sampled(n, rt, grid):
    return V.tile_rows(sorted(set(V.sampled_tiles(n, rt, grid)) | {((n + rt - 1) // rt) // 2}), rt, n)


@pytest.mark.parametrize("name", ["rt16", "rt32", "rt48", "rt64", "trips", "tiles-trips"])
def test_row_count_panels_are_fair(name):
    q, u, p = V.SMALL["q"], V.SMALL["units"], V.SMALL["p"]
    if name == "tiles-trips":
        occ = V.gxf_plan(q, u, p).occ
        n = V.rows_tiles_trips(N_CUS, occ)
        rt, grid = 32, V.gxf_grid(n, N_CUS, occ)
    else:
        n = V.rows_workspace_trips(N_CUS) if name == "trips" else V.rt_rows(N_CUS)[int(name[2:])]
        rt, _, grid = V.workspace_grid(n, N_CUS)
    rows = _b_sampled(n, rt, grid)
    r = V.chains64(V.case_net(V.SMALL), V.panel(n, p, 31), rows, V.B_SEED, V.B_ROW_BASE, V.B_STEP, V.B_LEAP, V.B_ITERS, V.B_ITERS, True)
    print("BVN-EDGE-HOST panel=%s n=%d sampled=%d flagged=%d accepted=%s s_min=%.2f" % (name, n, len(rows), r.flagged.sum(), r.acc.sum(axis=1).tolist(), r.s_min))
    assert r.flagged.sum() <= V.CAP_TRIPS * len(rows) and 0 < r.acc.sum() < r.acc.size and r.s_min > -3.0


def test_decode_and_step_panels_keep_the_variance_head_up():
    from oracle import bgm_bnn as OV
    net = OV.cast_vnet(V.case_net(V.SMALL), np.float64)
    rs = np.random.RandomState(10)
    z = rs.standard_normal((4096, V.SMALL["q"]))
    _, _, c = OV.vforward(net, z, OV.draw(net, len(z), V.D_SEED, 5, dtype=np.float64), training=False)
    assert c["s_raw"].min() > -3.0
    _, _, c = OV.vforward(net, z, OV.draw(net, len(z), V.D_SEED, 5, dtype=np.float64), training=True)
    assert c["s_raw"].min() > -3.0


# ---------------------------------------------------------------------------------------------------------------------------
# what the GPU file calls exists
# ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_engine_methods_exist():
    header = open(os.path.join(ROOT, "include", "bgm_hip.h")).read()
    for name in ("begin", "logpost", "hmc_run", "decode", "theta_step", "z_step", "read", "end"):          # (the symbols are not spelled out: ABI_MAP.md lists the files that CALL an entry point)
        assert re.search(r"\bbgm_bvn_%s\s*\(" % name, header), name
    src = open(os.path.join(ROOT, "bayesgm_amd", "bvn_engine.py")).read()
    for m in ("begin", "close", "read", "logpost", "hmc_run", "decode", "theta_step", "z_step"):
        assert re.search(r"^    def %s\(" % m, src, re.M), m
    api = open(os.path.join(ROOT, "bayesgm_amd", "csrc", "bgmb_api.hip")).read() + open(os.path.join(ROOT, "bayesgm_amd", "csrc", "bgmf_api.hip")).read()
    for switch in ("BGM_BVN_NO_TILES", "BGM_BVN_NO_CHAINS"):
        assert switch in api
