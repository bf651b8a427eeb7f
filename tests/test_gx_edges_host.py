"""The CPU side of tests/test_gpu_gx_edges.py: the conditions its inputs must meet and the plan it expects of the general-width engine,
from the float64 oracle and a restatement of the engine's LDS formulas (tests/_gx_edges_ref.py) alone.

- every chain case of the GPU file: the rows whose accept decisions lie within 2 (1e-5 max|lp| + 1e-3) of their uniform (fragile_rows)
  are at most 15 % of the panel (chains of up to 35 iterations) or 6 % (the 8-iteration multi-trip panels, sized for 256 CUs), and the
  last two tiles of a multi-trip panel keep unflagged rows;
- the restated formulas are the headers' and put the LDS boundary at hidden width 576 / 577 (sum(z_dims) = 10, p = 20), the
  row-tile-per-wave boundary at sum(z_dims) = 59 / 60 of a 128-wide model and at width 128 / 129;
- which forced dose batches the LDS admits on the two models of test_forced_dose_batch;
- the panels of part A cover every value the suite is meant to."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gx_edges_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesgm_amd", "csrc")
N_CUS = 256

CHAIN_CASES = G.chain_cases(N_CUS)


@pytest.mark.parametrize("k", range(len(CHAIN_CASES)), ids=[G.case_id(c) for c, _ in CHAIN_CASES])
def test_flagged_rows_within_the_cap(k):
    c, cap = CHAIN_CASES[k]
    _, m, data = G.build(c)
    n_iter = c["burn"] + c["keep"]
    state, flagged, acc = G.fragile_rows(m, data, n_iter, G.Q_SD, c["seed"])
    print("%s: %d of %d rows flagged in %d iterations (cap %.2f), %d accepted" % (G.case_id(c), flagged.sum(), c["n"], n_iter, cap * c["n"], acc.sum()))
    assert state.shape == (c["n"], sum(c["z_dims"])) and np.isfinite(state).all()
    assert flagged.sum() <= cap * c["n"]
    assert 0 < acc.sum() < c["n"] * n_iter          # the chains both move and stand still
    if "tile" in c:
        tail = np.arange((c["n"] - 1) // c["tile"] * c["tile"] - c["tile"], c["n"])
        assert len(tail) == c["tile"] + 5 and (~flagged[tail]).sum() >= c["tile"] // 2
        # the float32 oracle follows the float64 chain on the unflagged rows (what the kernels are asked to do)
        ref32 = G.OC.mh_sampler(m, data, c["burn"], c["keep"], G.Q_SD, c["seed"])[-1]
        ok = np.abs(ref32 - state).max(axis=1) <= 1e-4
        assert ok[~flagged].all() and ok.mean() >= 0.97


def _header(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_formulas_are_the_headers():
    dev, causal, fit, gw, api = (_header(n) for n in ("gx_device.h", "gx_causal_kernels.h", "gx_fit_kernels.h", "gw_kernels.h", "gx_api.hip"))
    for text, name, value in ((dev, "GX_ROWS", G.GX_ROWS), (causal, "GX_MAXDB", G.GX_MAXDB), (gw, "GW_ROWS", G.GW_ROWS), (gw, "GW_WAVES", G.GW_WAVES)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert "return ((width + 59) / 64) * 64 + 8;" in dev
    assert "return ((width + 63) / 64) * 64 + 4;" in gw
    assert "return GX_ROWS * (ld > db * ldf ? ld : db * ldf);" in causal
    assert "return 2 * gx_buf_floats(ld, ldf, db) + 2 * GX_ROWS * q + ncg * GX_ROWS + (6 + 2 * GX_MAXDB) * GX_ROWS + 64;" in causal
    assert "return 2 * GX_ROWS * ld + GX_ROWS * q + 8 * GX_ROWS + 64;" in fit
    assert "return GW_ROWS * (ld > db * ldf ? ld : db * ldf);" in gw
    assert "return 2 * gw_buf_floats(ld, ldf, db) + ((2 * GW_ROWS * q + 3) & ~3) + 2 * GW_ROWS;" in gw
    assert "s->lds_enc = 4 * 2 * GX_ROWS * s->ld_enc;" in api and "s->kc = std::min(m.e.pad[0], std::max(wenc, 256));" in api
    assert "4 * gw_wave_floats(s->gw_ld, m.q, ldf, 1) <= 24 * 1024" in api
    assert "const int occ = std::max(1, std::min(4, (160 * 1024) / s->lds_enc));" in api
    assert "> 160 * 1024) {" in api and "too wide" in api


def test_lds_boundary_at_576_and_577():
    z_dims, p = G.C_WIDE["z_dims"], G.C_WIDE["p"]
    assert sum(z_dims) == 10 and p == 20
    a, b = G.plan(G.SHAPES["w576"], z_dims, p), G.plan(G.SHAPES["w577"], z_dims, p)
    print("576: sampling %d B, fit %d B, encoder %d B; 577: %d, %d, %d" % (a["lds_bytes"], a["lds_fit"], a["lds_enc"], b["lds_bytes"], b["lds_fit"], b["lds_enc"]))
    assert a["lds_bytes"] == 154240 and b["lds_bytes"] == 170624
    assert a["served"] and max(a["lds_bytes"], a["lds_fit"], a["lds_enc"]) <= G.LDS_BYTES
    assert not b["served"] and b["lds_bytes"] > G.LDS_BYTES
    assert a["db"] == 1 and not a["gw"]


def test_family_boundary_at_59_and_60_and_at_width_129():
    (c59, c60, c129) = G.C_SWITCH
    a, b, c = (G.plan(G.SHAPES[x["shape"]], x["z_dims"], x["p"]) for x in G.C_SWITCH)
    print("wave region: %d B at q = 59, %d B at q = 60, %d B at width 129" % (a["gw_wave_bytes"], b["gw_wave_bytes"], c["gw_wave_bytes"]))
    assert sum(c59["z_dims"]) == 59 and sum(c60["z_dims"]) == 60
    assert a["gw_wave_bytes"] == 24576 and b["gw_wave_bytes"] == 24704
    assert (a["gw"], b["gw"], c["gw"]) == (True, False, False) == (c59["gw"], c60["gw"], c129["gw"])
    assert G.plan(G.SHAPES["w128"], [1, 1, 1, 7], 20)["gw"] and all(x["served"] for x in (a, b, c))
    for x in G.A_CASES + [G.C_WIDE, G.C_DOSE, G.C_DOSE_NARROW_F] + G.b_cases(N_CUS)[:2]:
        pl = G.plan(G.SHAPES[x["shape"]], x["z_dims"], x["p"])
        assert not pl["gw"] and pl["served"], G.case_id(x)
    for x in G.AB_CASES + G.b_cases(N_CUS)[2:]:
        assert G.plan(G.SHAPES[x["shape"]], x["z_dims"], x["p"])["gw"], G.case_id(x)


def test_forced_dose_batches_the_lds_admits():
    w160 = [G.plan(G.SHAPES["w160"], G.C_DOSE["z_dims"], G.C_DOSE["p"], force_db=d)["db"] for d in (1, 2, 3, 4)]
    odd = [G.plan(G.SHAPES["odd"], G.C_DOSE_NARROW_F["z_dims"], G.C_DOSE_NARROW_F["p"], force_db=d)["db"] for d in (1, 2, 3, 4)]
    auto = G.plan(G.SHAPES["w160"], G.C_DOSE["z_dims"], G.C_DOSE["p"])["db"]
    print("dose batch in effect: w160 %s (unforced %d), odd %s" % (w160, auto, odd))
    assert w160 == [1, 2, 3, auto] and odd == [1, 2, 3, 4]
    # unforced, only a narrow outcome net beside wider g / h stacks doses (its rows fit the buffers g needs anyway): `odd` in part A runs
    # 4 per pass, the models with f as wide as g (w160, deep, f-wide, w256 of test_gpu_widths.py) one
    own = {s: G.plan(G.SHAPES[s], [4, 4, 4, 5], 77)["db"] for s in ("w160", "odd", "f-wide", "deep", "w256")}
    print("dose batch the plan chooses itself: %s" % own)
    assert own == {"w160": 1, "odd": 4, "f-wide": 1, "deep": 1, "w256": 1}


def test_part_a_covers_what_it_is_meant_to():
    A = G.A_CASES
    assert len(A) <= 12
    assert {c["p"] for c in A} == {31, 32, 77}
    assert {sum(c["z_dims"]) for c in A} == {4, 16, 17}
    assert {c["n"] for c in A} == {1, 31, 32, 33, 65}
    assert {(c["shape"], c["binary"]) for c in A} == {("w160", False), ("w160", True), ("odd", False), ("odd", True), ("f-wide", False), ("deep", False)}
    for n in (1, 33):
        assert {c["binary"] for c in A if c["n"] == n} == {False, True}
    assert len(G.SHAPES["deep"]["g_units"]) == 8          # BGM_MAX_LAYERS
    n = G.rows_b_gx(N_CUS)
    assert n == 16421 and -(-n // G.GX_ROWS) == 2 * N_CUS + 2 and n % G.GX_ROWS == 5
    n = G.rows_b_gw(N_CUS)
    assert -(-n // G.GW_ROWS) == 2 * G.GW_WAVES * N_CUS + 2 and n % G.GW_ROWS == 5
    assert G.plan(G.SHAPES["r_test"], [1, 1, 1, 1], 4)["enc_occ"] == 4
