"""What the cases of tests/test_gpu_egm_edges.py reach, shown without a device from the restated host plan of tests/_egm_edges_ref.py
(egm_plan of csrc/egm_plan.h, which bgm_causal_egm_begin evaluates, and the kernel tables of csrc/egm_api.hip), and the conditions the float64 oracle alone
puts on their inputs: finite losses, gradients that are not all rounding noise, a live last column behind every mask.

The batches beyond the ones the project's tolerances were set on (B >= 40) get the oracle itself in float32 here: its deviation from
float64 is printed per case (pytest -s, EGM-EDGE-HOST lines) and must stay inside the bars of tests/test_gpu_egm.py, so a kernel that
misses them there cannot blame the summation length."""
import os
import re

import numpy as np
import pytest

import _egm_edges_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesgm_amd", "csrc")
ids = [c["name"] for c in E.CASES]
BAR_LOSS, BAR_GRAD, BAR_PARAM = 2e-5, 5e-5, 2e-5          # tests/test_gpu_egm.py


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# ---------------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.CASES, ids=ids)
def test_case_reaches_what_its_table_entry_names(c):
    pl = E.case_plan(c)
    assert (pl.disc, pl.gen) == (c["want_disc"], c["want_gen"]), (pl.disc, pl.gen)
    assert pl.disc in E.DISC_ROUTES and pl.gen in E.GEN_ROUTES
    assert pl.t0 == (1 if sum(c["z_dims"]) <= 16 else 2)
    if pl.disc.startswith("chain"):
        assert 0 < pl.chain_disc_bytes <= E.LDS_LIMIT          # checked, not assumed
    if pl.gen.startswith("chain"):
        assert 0 < pl.chain_gen_bytes <= E.LDS_LIMIT and pl.disc.startswith("chain")
    if pl.disc == "lds":
        assert pl.disc_lds == 1 and pl.arena_bytes <= E.LDS_LIMIT
    if pl.disc == "global":
        assert pl.disc_lds == 0 and pl.arena_bytes > E.LDS_LIMIT
    assert c["n"] == E.N_ROWS
    z, idx, _ = E.inputs(c["name"]).grad_batch
    assert z.shape == (c["B"], sum(c["z_dims"])) and idx.min() >= 0 and idx.max() < c["n"]
    if c["ends"]:
        for (d1, d2, g) in E.inputs(c["name"]).rounds + [(E.inputs(c["name"]).grad_batch,) * 3]:
            for b in (d1, d2, g):
                assert 0 in b[1] and c["n"] - 1 in b[1] and len(set(b[1].tolist())) == c["B"]


def test_the_table_reaches_every_route():
    assert {E.case_plan(c).disc for c in E.CASES} == set(E.DISC_ROUTES) and len(E.DISC_ROUTES) == 7
    assert {E.case_plan(c).gen for c in E.CASES} == set(E.GEN_ROUTES) and len(E.GEN_ROUTES) == 7
    ends = [c for c in E.CASES if c["ends"]]
    assert any(c["want_disc"] == "global" for c in ends) and any(E.is_chain(c) for c in ends)
    zr = {c["want_gen"] for c in E.CASES if not c["use_z_rec"]}
    assert zr == {"chain-32-n13", "chain-pad", "step"}
    assert any(c["B"] > E.EGM_THREADS for c in E.CASES) and {2, 3} <= {c["B"] for c in E.CASES}
    assert max(len(c["e_units"]) for c in E.CASES) == E.EGM_MAX_LAYERS - 1 and min(len(c["g_units"]) for c in E.CASES) == 1


def test_lds_boundary_of_the_workgroup_kernel():
    args = (E.D_DEF, E.G_DEF, E.G_DEF, E.FH_DEF, E.FH_DEF, False)
    a39, a40 = E.plan(23, E.Z10, 39, *args), E.plan(23, E.Z10, 40, *args)
    assert (a39.arena_bytes, a39.disc_lds, a39.disc) == (162560, 1, "lds")
    assert (a40.arena_bytes, a40.disc_lds, a40.disc) == (166688, 0, "global")
    assert a39.arena_bytes <= 163840 < a40.arena_bytes and E.LDS_LIMIT == 163840
    need = [E.plan(23, E.Z10, B, *args).arena_bytes for B in range(E.B_MIN, 600)]
    assert all(x < y for x, y in zip(need, need[1:]))          # by exhaustion: 39 is the only switch point
    wide = E.plan(23, E.Z10, 16, (256, 64, 8), *args[1:])
    assert wide.disc == "global" and E.plan(23, E.Z10, 8, (256, 64, 8), *args[1:]).disc == "lds"
    # the chains' own LDS need stays inside the limit at every shape their predicate admits
    assert 4 * E.ech_disc_lds_floats(32, 1) <= E.LDS_LIMIT and 4 * E.ech_disc_lds_floats(32, 2) <= E.LDS_LIMIT
    assert 4 * E.ecg_lds_floats(32, 2) <= E.LDS_LIMIT


def test_discriminator_predicate_sweep():
    chained = set()
    for d1 in range(40, 71):
        for d2 in range(10, 41):
            for d3 in range(0, 21):
                for B in (16, 32):
                    pl = E.plan(23, E.Z10, B, (d1, d2, d3), E.G_DEF, E.G_DEF, E.FH_DEF, E.FH_DEF, True)
                    if pl.disc.startswith("chain"):
                        chained.add((d1, d2, d3, B))
                    else:
                        assert pl.disc == "lds" and pl.gen == "step"
    assert chained == {(a, b, c, B) for a in range(49, 65) for b in range(17, 33) for c in range(1, 17) for B in (16, 32)}
    base = dict(p=23, z_dims=E.Z10, B=32, dz_units=E.D_DEF, g_units=E.G_DEF, e_units=E.G_DEF, f_units=E.FH_DEF, h_units=E.FH_DEF, fixed_norm=True)
    assert E.plan(**base).disc == "chain-32-stream"
    for change in (dict(fixed_norm=False), dict(B=31), dict(B=33), dict(B=17), dict(dz_units=(64, 32)), dict(dz_units=(64, 32, 8, 8)),
                   dict(e_units=(64, 63, 64)), dict(z_dims=(8, 8, 8, 9))):
        assert not E.plan(**dict(base, **change)).disc.startswith("chain"), change
    assert E.plan(**dict(base, z_dims=E.Z18)).disc == "chain-t2" and E.plan(**dict(base, z_dims=E.Z18, B=16)).disc == "lds"
    assert E.plan(**dict(base, z_dims=(8, 8, 8, 8))).disc == "chain-t2" and E.plan(**dict(base, z_dims=(4, 4, 4, 4))).disc == "chain-32-stream"


def test_generator_predicate_and_extent_sweep():
    args = (E.D_DEF, E.G_DEF, E.G_DEF, E.FH_DEF, E.FH_DEF, True)
    for p in range(90, 216):
        pl32, pl16 = E.plan(p, E.Z10, 32, *args), E.plan(p, E.Z10, 16, *args)
        kd, kg = (p + 15) // 16, (p + 16) // 16
        want_d = "chain-32-k%d" % kd if kd in (7, 13) else "chain-32-stream"
        want_g = "chain-32-n%d" % kg if kg in (7, 13) else "chain-pad" if kg <= 13 else "step"
        assert (pl32.disc, pl32.gen) == (want_d, want_g), p
        assert (pl16.disc, pl16.gen) == ("chain-16", "chain-16-n%d" % kg if kg in (7, 13) else "step"), p
        if p in E.EXTENT_PAIRS:
            assert (pl32.disc, pl32.gen) == E.EXTENT_PAIRS[p]
    assert sorted(E.EXTENT_PAIRS) == [95, 96, 111, 112, 191, 192, 207, 208]
    assert {c["p"]: (c["want_disc"], c["want_gen"]) for c in E.CASES if c["name"].startswith("p")} == E.EXTENT_PAIRS
    # the two steps disagree exactly where p + 1 opens a tile that p does not
    assert [p for p in range(90, 216) if (p + 15) // 16 != (p + 16) // 16] == [96, 112, 128, 144, 160, 176, 192, 208]
    # the heads: three hidden layers 64, 32, 1..16 and at most 16 inputs; g with 64-wide hidden layers of any depth
    base = dict(p=100, z_dims=E.Z10, B=32, dz_units=E.D_DEF, g_units=E.G_DEF, e_units=E.G_DEF, f_units=E.FH_DEF, h_units=E.FH_DEF, fixed_norm=True)
    for w in range(1, 20):
        for key in ("f_units", "h_units"):
            assert E.plan(**dict(base, **{key: (64, 32, w)})).gen == ("chain-32-n7" if w <= 16 else "step")
    for change in (dict(f_units=(64, 32)), dict(h_units=(63, 32, 8)), dict(f_units=(64, 31, 8)), dict(g_units=(64, 65)), dict(z_dims=(8, 8, 0, 0)),
                   dict(z_dims=(9, 0, 8, 0))):
        pl = E.plan(**dict(base, **change))
        assert pl.gen == "step" and pl.disc.startswith("chain"), change
    assert E.plan(**dict(base, z_dims=(8, 7, 0, 0))).gen == "chain-32-n7" and E.plan(**dict(base, z_dims=E.Z24)).gen == "chain-t2"
    for depth in range(1, E.EGM_MAX_LAYERS):
        assert E.plan(**dict(base, g_units=(64,) * depth, e_units=(64,) * (E.EGM_MAX_LAYERS - depth))).gen == "chain-32-n7"


@pytest.mark.parametrize("c", E.CASES, ids=ids)
def test_switches(c):
    off_d, off_g, off_both = E.case_plan(c, no_chain=True), E.case_plan(c, no_chain_gen=True), E.case_plan(c, no_chain=True, no_chain_gen=True)
    fallback = "lds" if off_d.disc_lds else "global"
    assert off_d.disc == fallback and off_d.gen == "step"          # chain_gen requires chain_disc_lds > 0
    assert off_g.disc == c["want_disc"] and off_g.gen == "step"
    assert (off_both.disc, off_both.gen) == (fallback, "step")
    if not E.is_chain(c):
        assert off_both[:5] == E.case_plan(c)[:5]


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement against the C++ text
# ---------------------------------------------------------------------------------------------------------------------------
def _static_asserts(src):
    """the conditions of a header's static_asserts, without their messages"""
    return " ".join(re.findall(r"static_assert\((.*?),\s*\"", src, re.S))


def test_restated_constants_are_the_sources():
    """The plan moved from the text of egm_api.hip into csrc/egm_plan.h (chain_extent, the predicates, egm_arena, egm_plan); the kernel
    tables and the calls of the LDS-size functions stay in egm_api.hip.  Where egm_plan.h pins a fact in a static_assert, the assert is
    looked for instead of the expression text."""
    api, plan, ker, chain, gen = _src("egm_api.hip"), _src("egm_plan.h"), _src("egm_kernels.h"), _src("egm_chain.h"), _src("egm_chain_gen.h")
    pins = _static_asserts(plan)
    assert "constexpr int EGM_LDS_LIMIT = 160 * 1024;" in plan and E.LDS_LIMIT == 160 * 1024
    # disc_lds and the chain's own size: both against the one limit
    assert "(64 + arena) * sizeof(float) <= (size_t)EGM_LDS_LIMIT" in plan and "chain_disc_bytes <= (size_t)EGM_LDS_LIMIT" in plan
    assert "<= 160 * 1024" not in api and len(re.findall(r"160 \* 1024", plan)) == 1
    lo, hi = re.search(r"cfg->batch_size < (\d+) \|\| cfg->batch_size > (\d+)", api).groups()
    assert (int(lo), int(hi)) == (E.B_MIN, E.B_MAX)
    assert int(re.search(r"#define EGM_THREADS (\d+)", ker).group(1)) == E.EGM_THREADS
    assert int(re.search(r"#define EGM_MAX_LAYERS (\d+)", ker).group(1)) == E.EGM_MAX_LAYERS
    assert int(re.search(r"#define ECH_ROLE_WAVES (\d+)", chain).group(1)) == E.ECH_ROLE_WAVES
    assert re.search(r"L < 1 \|\| L > EGM_MAX_LAYERS", api)
    # the tile rules of the discriminator chain
    t1, t2 = re.search(r"chain_tiles\(d\[1\]\) == (\d+) && chain_tiles\(d\[2\]\) == (\d+)", plan).groups()
    d3lo, d3hi = re.search(r"d\[3\] >= (\d+) &&\s+d\[3\] <= (\d+)", plan).groups()
    assert (int(t1), int(t2), int(d3lo), int(d3hi)) == (E.CHAIN_T[0], E.CHAIN_T[1], 1, 16 * E.CHAIN_T[2])
    assert "constexpr int chain_tiles(int n) { return (n + 15) / 16; }" in plan
    assert re.search(r"\(B == 16 \|\| B == 32\)", plan) and E.CHAIN_BATCHES == (16, 32)
    assert re.search(r"fixed_norm && n_hidden == 3 && d\[0\] <= 32 && \(d\[0\] <= 16 \|\| B == 32\)", plan)
    assert re.search(r"const int ntl_need = \(p \+ 16\) / 16, t0 = q <= 16 \? 1 : 2;", plan)
    assert "if (n.dims[l] != 64) return false;" in plan          # chain_hidden64, asked of e and of g:
    assert "chain_trunk_ok(s.e, 2, -1, s.q)" in plan and "chain_trunk_ok(s.g, 2, s.q, -1)" in plan and "&& chain_hidden64(n);" in plan
    assert set(re.findall(r"ech_disc_lds_floats<([\d, ]+)>\(d, B\)", api)) == {"4, 2, 1", "4, 2, 1, 2"}
    assert set(re.findall(r"ecg_lds_floats<([\d, ]+)>\(d, B\)", api)) == {"4, 2, 1", "4, 2, 1, 2"}
    # ... of the generator chain
    assert re.search(r"const int ntl = \(\(ntl_need == 13 \|\| ntl_need == 7\) && t0 == 1\) \? ntl_need : 13;", plan) and E.GEN_EXTENTS == (13, 7)
    assert "return x.ntl_need <= 13 && (x.ntl == x.ntl_need || B == 32);" in plan
    assert re.search(r"const bool gchain = dchain && chain_extent_ok\(x, s\.B\)", plan)
    assert re.search(r"n\.n_layers == 4 && n\.dims\[0\] <= 16 && n\.dims\[1\] == 64 && n\.dims\[2\] == 32 && n\.dims\[3\] >= 1 && n\.dims\[3\] <= 16", plan)
    assert "chain_head_ok(s.f, 1, 16) && chain_head_ok(s.h, 1, 16)" in plan
    assert E.HEAD_FIXED == (64, 32)
    assert "return {t0, ntl_need, ntl, ntl != ntl_need || t0 == 2};" in plan
    # ... of the kernel choice: the plan's routes under the names of this file, and the kernels behind them in the same order
    assert re.search(r"const int kt0 = chain_tiles\(s\.p\);", plan) and re.search(r"kt0 == 13 \?", plan) and re.search(r"kt0 == 7 \?", plan)
    assert tuple(re.findall(r'"([\w-]+)"', re.search(r"EGM_DISC_ROUTE_NAMES\[\] = \{(.*?)\};", plan).group(1))) == E.DISC_ROUTES
    assert tuple(re.findall(r'"([\w-]+)"', re.search(r"EGM_GEN_ROUTE_NAMES\[\] = \{(.*?)\};", plan).group(1))) == E.GEN_ROUTES
    assert len(re.search(r"enum class EgmDiscRoute \{(.*?)\}", plan).group(1).split(",")) == len(E.DISC_ROUTES)
    assert len(re.search(r"enum class EgmGenRoute \{(.*?)\}", plan).group(1).split(",")) == len(E.GEN_ROUTES)
    assert re.findall(r"egm_disc_chain_kernel<([\d, ]+)>", api) == ["4, 0, 4, 2, 1, 2, 2", "4, 13, 4, 2, 1, 2", "4, 7, 4, 2, 1, 2", "4, 0, 4, 2, 1, 2",
                                                                    "4, 0, 4, 2, 1, 1"]          # the rows of egm_disc_kernel, in the enum's order
    assert re.findall(r"egm_gen_chain_kernel<([\w, ]+)>", api) == ["4, 13, 4, 2, 1, 2, true, 2", "4, 13, 4, 2, 1, 2, true", "4, 13, 4, 2, 1, 2",
                                                                   "4, 7, 4, 2, 1, 2", "4, 13, 4, 2, 1, 1", "4, 7, 4, 2, 1, 1"]
    # ... pinned at the edges by the header itself
    for want in ("routes(95, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_PAD}", "routes(96, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_32_N7}",
                 "routes(111, 10, 32) == Routes{D::CHAIN_32_K7, G::CHAIN_32_N7}", "routes(112, 10, 32) == Routes{D::CHAIN_32_K7, G::CHAIN_PAD}",
                 "routes(191, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_PAD}", "routes(192, 10, 32) == Routes{D::CHAIN_32_STREAM, G::CHAIN_32_N13}",
                 "routes(207, 10, 32) == Routes{D::CHAIN_32_K13, G::CHAIN_32_N13}", "routes(208, 10, 32) == Routes{D::CHAIN_32_K13, G::STEP}",
                 "egm_arena(39, 3, DZ_DEF).lds_bytes == 162560", "(64 + egm_arena(40, 3, DZ_DEF).floats) * sizeof(float) == 166688"):
        assert want in pins, want
    # the two switches (read when a session begins, egm_switches_now) and the arena pointer
    assert 'getenv("BGM_EGM_NO_CHAIN")' in plan and 'getenv("BGM_EGM_NO_CHAIN_GEN")' in plan and "egm_switches_now()" in api
    assert "!sw.no_chain &&" in plan and "!sw.no_chain_gen;" in plan and "getenv" not in api
    assert "float *arena = a.disc_lds ? (egm_lds + 64) : wp;" in ker
    # the arena formula and the chains' LDS sizes, as text
    assert "((size_t)(2 * B + 1) * dsum + B + 3) / 4 * 4" in plan and "((size_t)B * dall + (size_t)(5 * B + 1) * dsum + 3) / 4 * 4 + 3 * (size_t)B * dmax" in plan
    assert "cache + std::max(cache + 2 * (size_t)B * dmax, gp)" in plan
    assert "64 + ech_layout<T1, T2, T3, T0>(d).total + ECH_ROLE_WAVES * D::SLOT + 16 * T0 * B + (T0 > 1 ? 3 : 4) * B * D::SW" in chain
    assert "XW = 16 * (T0 + T1 + T2), DW = 16 * (T1 + T2 + T3), SW = XW + DW" in chain and "SLOT = 2 * SL + 16 * T3 + 16" in chain
    assert "P.ld0 = 16 * T1 + 4; P.ld1 = 16 * T2 + 4; P.ld2 = 16 * T3 + 4;" in chain and "P.lt0 = 16 * T0 + 4; P.lt1 = 16 * T1 + 4; P.lt2 = 16 * T2 + 4;" in chain
    assert "64 + ech_layout<T1, T2, T3, T0>(d).total + 8 * 16 + 16 + 3 * 16 * T0 * B" in gen


def test_engine_methods_the_gpu_file_calls_exist():
    src = open(os.path.join(ROOT, "bayesgm_amd", "engine.py")).read()
    for m in ("set_disc_norm", "egm_begin", "egm_disc_step", "egm_gen_step", "egm_sizes", "egm_grad", "egm_apply", "egm_read", "egm_end", "get_weights"):
        assert re.search(r"^    def %s\(" % m, src, re.M), m


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs, from the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------
def _net_slices(I):
    out, off = {}, 0
    for k in ("g", "e", "f", "h"):
        n = sum(W.size + b.size for W, b in I.nets[k])
        out[k] = slice(off, off + n)
        off += n
    return out


@pytest.mark.parametrize("c", E.CASES, ids=ids)
def test_oracle_alone_meets_the_conditions_on_the_inputs(c):
    I, r = E.inputs(c["name"]), E.grads64(c["name"])
    assert np.isfinite(r.d_losses).all() and np.isfinite(r.g_losses).all() and np.isfinite(r.d_grads).all() and np.isfinite(r.g_grads).all()
    sl = _net_slices(I)
    tops = {k: float(np.abs(r.g_grads[s]).max()) for k, s in sl.items()}
    tops["dz"] = float(np.abs(r.d_grads).max())
    print("EGM-EDGE-HOST case=%s largest gradient entries %s" % (c["name"], {k: "%.2e" % v for k, v in tops.items()}))
    assert min(tops.values()) > 1e-6, tops
    if c["masked"]:
        live = []
        for l, w in enumerate(c["dz_units"]):          # the discriminator's masked layers: last valid column of W, b, gamma, beta and the row behind it
            if w % 16:
                live += [r.d_tree["W"][l][:, -1], r.d_tree["gamma"][l][-1:], r.d_tree["beta"][l][-1:], r.d_tree["W"][l + 1][-1, :]]
                if c["fixed"]:
                    live.append(r.d_tree["b"][l][-1:])
        for k in ("f", "h"):
            gk = r.g_tree[k]
            if c[k + "_units"][2] % 16:
                live += [gk[2][0][:, -1], gk[2][1][-1:], gk[3][0][-1, :]]
            live.append(gk[0][0][-1, :])                 # last head input: x for f, the last column of z2 for h
            live += [gk[3][0][:, -1], gk[3][1][-1:]]     # the variance output
        if (c["p"] + 1) % 16:
            live += [r.g_tree["g"][-1][0][:, -1], r.g_tree["g"][-1][1][-1:], r.g_tree["g"][-1][0][:, c["p"] - 1]]
        if c["p"] % 16:
            live.append(r.g_tree["e"][0][0][-1, :])
        live += [r.g_tree["e"][-1][0][:, -1], r.g_tree["g"][0][0][-1, :]]          # the last latent column
        assert all(np.abs(a).max() > 1e-9 for a in live), [float(np.abs(a).max()) for a in live]


BIG = [c["name"] for c in E.CASES if c["B"] >= 40]
SMALL = [c["name"] for c in E.CASES if c["B"] < 16 or (not c["fixed"] and c["B"] < 40)]


@pytest.mark.parametrize("name", BIG + SMALL)
def test_float32_oracle_stays_inside_the_project_bars(name):
    """The oracle itself in float32 against float64, one step's losses and gradients and the parameters after the alternating rounds.
    B >= 40 (more terms per sum than the batches the bars were set on): inside the bars, so no case of the table needs a bound of its own.
    The batches below 16 rows and the batch-normalised ones below 40 are held to a QUARTER of the bars (a tree sum against a sequential
    one may cost a kernel four times the oracle's own float32 error): batch statistics of two rows (8.5e-6 on the trained parameters)
    and of three rows (9.6e-5 on the generator gradient) did not pass that, so ws-b2 and ws-b3 run with fixed statistics.
    Measured: the EGM-EDGE-HOST lines; the worst is recorded in DESIGN.md."""
    a, b = E.step_grads(name, np.float32), E.grads64(name)
    dl = np.abs(a.d_losses - b.d_losses) / (BAR_LOSS * np.abs(b.d_losses) + np.array([1e-6, 1e-5]))
    gl = np.abs(a.g_losses - b.g_losses) / (BAR_LOSS * np.abs(b.g_losses) + 1e-6)
    ed, eg = E.rel(a.d_grads, b.d_grads), E.rel(a.g_grads, b.g_grads)
    t32, t64, keep = E.trained(name, np.float32), E.trained64(name), ~E.inert_disc_mask(name)
    tg, td = float(np.abs(t32.theta_g - t64.theta_g).max()), float(np.abs(t32.theta_d - t64.theta_d)[keep].max())
    print("EGM-EDGE-HOST case=%s float32 oracle vs float64: disc grads %.2e gen grads %.2e (bar %.0e), loss ratios %.3f / %.3f, trained g|e|f|h %.2e "
          "discriminator %.2e (bar %.0e)" % (name, ed, eg, BAR_GRAD, dl.max(), gl.max(), tg, td, BAR_PARAM))
    k = 4 if name in SMALL else 1
    assert k * ed <= BAR_GRAD and k * eg <= BAR_GRAD and k * dl.max() <= 1 and k * gl.max() <= 1
    assert k * tg <= BAR_PARAM and k * td <= BAR_PARAM
