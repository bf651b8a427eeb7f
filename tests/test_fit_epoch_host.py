"""The case table of the in-library fit epoch (tests/_fit_epoch_cases.py) reaches every kernel family, minibatch instantiation and ring
edge of bgm_causal_fit_epoch -- proved here from the plain-Python restatement of the dispatch alone (no GPU), so that an edit of the table
cannot drop one silently.  tests/test_gpu_fit_epoch.py runs the table and checks the restatement's family against the library's own
description of the open session."""
import ast
import os

import pytest

from tests import _fit_epoch_cases as FE

PLANS = {c["name"]: FE.plan_of(c) for c in FE.CASES}


def _where(**want):
    """names of the cases whose case fields / plan fields equal `want`"""
    out = []
    for c in FE.CASES:
        merged = dict(PLANS[c["name"]], **c)
        if all(merged[k] == v for k, v in want.items()):
            out.append(c["name"])
    return out


def test_the_module_imports_without_torch():
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), "_fit_epoch_cases.py")).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | {
        (n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
    assert names <= {"os", "sys"}, names


def test_panels_are_small():
    for c in FE.CASES:
        assert c["n_use"] <= c["n"] <= 400 and PLANS[c["name"]]["n_mb"] <= 9, c["name"]


@pytest.mark.parametrize("p", [192, 200, 207])
def test_unpadded_13_tile_family(p):
    assert _where(p=p, chain=True, ntl=13, t0=1, pad=False, overlap=True)


@pytest.mark.parametrize("p", [96, 100, 111])
def test_unpadded_7_tile_family(p):
    assert _where(p=p, chain=True, ntl=7, t0=1, pad=False, overlap=True)


@pytest.mark.parametrize("p", [20, 95, 112])
def test_padded_13_tile_family(p):
    assert _where(p=p, chain=True, ntl=13, t0=1, pad=True, overlap=True)


def test_two_latent_tiles_binary():
    names = _where(p=100, z_dims=(3, 3, 6, 6), binary=True, chain=True, t0=2, ntl=13, pad=True, overlap=True)
    assert names
    assert all(m["inst"] == "T2" and m["nchain"] == 1 for n in names for m in PLANS[n]["minibatches"])


def test_binary_treatment_on_an_unpadded_family():
    assert _where(binary=True, chain=True, pad=False, overlap=True)


def test_models_the_chains_decline():
    assert _where(p=208, chain=False, family="gx", overlap=False, D=1)
    assert FE.chain_setup(207, (1, 1, 1, 7), FE.G5, FE.FH, FE.FH) and not FE.chain_setup(208, (1, 1, 1, 7), FE.G5, FE.FH, FE.FH)
    assert _where(f_units=(32, 8), chain=False, family="gx", overlap=False)
    names = _where(g_units=(64,), chain=False, family="blob", overlap=False)          # default widths: the LDS-blob phase kernels
    assert names and all(FE.chain_setup(**{k: FE.BY_NAME[n][k] for k in ("p", "z_dims", "g_units", "f_units", "h_units")}) is None for n in names)
    assert _where(g_units=(96, 96), chain=False, family="gx", overlap=False)
    for n in _where(chain=False):
        assert PLANS[n]["ring_ends_on_slot0"] and not PLANS[n]["riders"], n


@pytest.mark.parametrize("B,overlap", [(32, True), (17, True), (16, True), (1, True), (33, False), (64, False)])
def test_minibatch_sizes(B, overlap):
    names = _where(p=200, B=B, lazy=2, overlap=overlap)
    assert names
    pl = PLANS[names[0]]
    if B == 17:
        assert [m["rows"] for m in pl["minibatches"][:-1]] == [17] * (pl["n_mb"] - 1) and pl["minibatches"][0]["nb"] == 2
        assert pl["minibatches"][0]["nchain"] == 2 and pl["minibatches"][0]["inst"] == "FS13"
    if B in (16, 1):
        assert all(m["nb"] == 1 and m["nchain"] == 1 and m["inst"] == "FW13" for m in pl["minibatches"])
    if B > 32:
        assert pl["family"] == "blob" and pl["D"] == 1 and not pl["chain"]
    assert _where(B=16, ntl=7, chain=True)                     # one row tile on the 7-tile family too


@pytest.mark.parametrize("rows", [1, 16, 17])
def test_short_last_minibatch_at_32(rows):
    names = [n for n in _where(B=32, chain=True, pad=False, t0=1) if PLANS[n]["sizes"][-1] == rows and PLANS[n]["n_mb"] > 1]
    assert names
    last = PLANS[names[0]]["minibatches"][-1]
    assert (last["nb"], last["nchain"]) == ((1, 1) if rows <= 16 else (2, 2))      # 1..16 rows left: the other instantiation


@pytest.mark.parametrize("n_mb", [1, 2, 3, 4, 5, 8, 9])
def test_ring_edges_in_replay_mode_on_the_headline_shape(n_mb):
    names = _where(p=200, B=32, lazy=2, n_mb=n_mb, overlap=True, D=4)
    assert names
    pl = PLANS[names[0]]
    assert pl["ring_ends_on_slot0"] == (n_mb in (4, 8))
    assert pl["waits_on_ring_slot"] == (n_mb > 4)
    assert bool(pl["replays_beyond_the_list"]) == (n_mb < 4)
    assert len(pl["riders"]) == max(0, n_mb - 4)
    assert all(r["first_block"] == 2 for r in pl["riders"])   # two chain workgroups, riders from block 2 on


@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("n_mb", [1, 4, 5])
def test_ring_edges_in_the_other_modes(n_mb, lazy):
    names = _where(p=200, B=32, lazy=lazy, n_mb=n_mb)
    assert names
    pl = PLANS[names[0]]
    assert pl["overlap"] == (lazy == 1) and pl["D"] == (4 if lazy == 1 else 1) and not pl["riders"]


def test_a_rider_targets_a_short_last_minibatch():
    names = [n for n in _where(rider_targets_short=True) if PLANS[n]["n_mb"] >= 5]
    assert names
    rows = {PLANS[n]["riders"][-1]["rows"] for n in names}
    assert {1, 16, 17} <= rows
    assert any(PLANS[n]["riders"][-1]["first_block"] == 1 for n in names)      # ... from block 1 on where the chains are one workgroup
    assert any(PLANS[n]["riders"][-1]["first_block"] == 2 for n in names)


def test_rows_outside_the_permutation():
    assert {FE.BY_NAME[n]["lazy"] for n in FE.OUTSIDE_CASES} == {0, 1, 2}
    assert len({FE.BY_NAME[n]["n_use"] for n in FE.OUTSIDE_CASES}) == 1
    assert all(FE.BY_NAME[n]["n_use"] < FE.BY_NAME[n]["n"] for n in FE.OUTSIDE_CASES)


def test_the_named_subsets():
    for n in FE.EVENT_CASES:
        c, pl = FE.BY_NAME[n], PLANS[n]
        assert c["p"] in (200, 20) and pl["n_mb"] in (3, 9) and c["lazy"] in (1, 2) and pl["overlap"]
    assert len({(FE.BY_NAME[n]["p"], PLANS[n]["n_mb"], FE.BY_NAME[n]["lazy"]) for n in FE.EVENT_CASES}) == 8
    a, b, c = (PLANS[n] for n in FE.SWITCH_CASES)       # the cases every development switch is run on
    assert not a["pad"] and a["riders"] and a["n_mb"] > 2 * a["D"] and a["sizes"][-1] == 16 and a["minibatches"][0]["inst"] == "FS13"
    assert b["pad"] and b["t0"] == 1 and b["sizes"][-1] == 17 and b["minibatches"][0]["inst"] == "PAD"
    assert b["n_mb"] % 3 != 0 and a["n_mb"] % 2 != 0           # a ring of three / two buffers ends on another slot: the copy-back
    assert c["t0"] == 2 and c["overlap"] and not c["riders"] and c["minibatches"][0]["inst"] == "T2"
    assert len(FE.EPOCH_SWITCHES) == 5 and len(FE.VARIANT_SWITCHES) == 3 and not set(FE.EPOCH_SWITCHES) & set(FE.VARIANT_SWITCHES)
    for n in FE.ORACLE_CASES:
        c, pl = FE.BY_NAME[n], PLANS[n]
        assert c["B"] == 32 and pl["sizes"] == [32, 32, 32, 17] and pl["chain"]
    assert {(FE.BY_NAME[n]["p"], PLANS[n]["t0"], FE.BY_NAME[n]["lazy"]) for n in FE.ORACLE_CASES} == {
        (p, t0, lazy) for p, t0 in ((200, 1), (100, 2), (20, 1)) for lazy in (0, 1, 2)}


def test_restatement_at_hand_checked_points():
    """Values read off fit_chain_setup / fit_chain_launch / fit_epoch_impl by hand."""
    pl = FE.plan(200, (1, 1, 1, 7), FE.G5, FE.FH, FE.FH, 32, 2, 272)
    assert (pl["ntl"], pl["t0"], pl["pad"], pl["D"], pl["n_mb"]) == (13, 1, False, 4, 9)
    assert [m["nchain"] for m in pl["minibatches"]] == [2] * 8 + [1]
    assert [(r["on"], r["target"], r["rows"], r["blocks"]) for r in pl["riders"]] == [(0, 4, 32, 10), (1, 5, 32, 10), (2, 6, 32, 10),
                                                                                      (3, 7, 32, 10), (4, 8, 16, 5)]
    pl = FE.plan(20, (1, 1, 1, 7), FE.G5, FE.FH, FE.FH, 32, 2, 2000)              # the class-level panel
    assert (pl["ntl"], pl["pad"], pl["n_mb"], pl["sizes"][-1]) == (13, True, 63, 16) and {m["nchain"] for m in pl["minibatches"]} == {1}
    pl = FE.plan(100, (3, 3, 6, 6), FE.G5, FE.FH, FE.FH, 32, 0, 113)
    assert pl["chain"] and pl["t0"] == 2 and not pl["overlap"] and pl["D"] == 1
    assert FE.plan(150, (3, 3, 6, 6), FE.G5, FE.FH, FE.FH, 32, 1, 64)["family"] == "chain"        # q + 1 = 19: 10 output tiles at most
    assert FE.plan(170, (3, 3, 6, 6), FE.G5, FE.FH, FE.FH, 64, 1, 64)["family"] == "gx"           # no blob and no chain above 32 rows
    assert FE.plan(170, (3, 3, 6, 6), FE.G5, FE.FH, FE.FH, 32, 1, 64)["family"] == "chain"
