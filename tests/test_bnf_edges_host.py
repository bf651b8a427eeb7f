"""Conditions of test_gpu_bnf_edges.py that need no device: the restated shape table (plan) at the dispatch boundaries, and for every
Metropolis-Hastings case, from the float64 oracle alone, that at most 2 % of its rows have an accept decision within 1e-3 of its
uniform (such rows are excused from the state comparison) and that at least a quarter of its proposals are accepted (a frozen sampler
cannot pass)."""
import numpy as np
import pytest

import _bnf_edges_ref as E


def _plan_of(z_dims, p):
    return E.plan(sum(z_dims), p, z_dims[0], z_dims[1])


def test_plan_at_the_dispatch_boundaries():
    for z_dims, p in E.SERVED_SHAPES:
        assert _plan_of(z_dims, p).served, (z_dims, p)
    for z_dims, p in E.UNSERVED_SHAPES:
        assert not _plan_of(z_dims, p).served, (z_dims, p)
    assert E.plan(10, 4, 1, 1).NTL == 1 and E.plan(10, 15, 1, 1).NTL == 1 and E.plan(10, 16, 1, 1).NTL == 2 and E.plan(10, 207, 1, 1).NTL == 13
    assert not E.plan(10, 3, 1, 1).served and not E.plan(10, 208, 1, 1).served
    assert E.plan(31, 40, 16, 15).served and not E.plan(32, 20, 8, 8).served
    # the LDS fit: 161 856 B at q >= 16, p = 175 (160 KiB = 163 840 B); one more output tile and the plan is wide
    for q in (16, 31):
        assert E.plan(q, 175, 4, 4).lds_bytes == 161856 and E.plan(q, 175, 4, 4).served
        assert E.plan(q, 176, 4, 4).lds_bytes > E.LDS_LIMIT and not E.plan(q, 176, 4, 4).served
    assert E.plan(15, 207, 2, 3).served and E.plan(15, 207, 2, 3).lds_bytes <= E.LDS_LIMIT
    assert not E.plan(16, 207, 4, 4).served
    # an outcome net wider than 32 inputs has no instance
    assert not E.plan(31, 40, 16, 16).served


def test_cases_sit_where_the_table_says():
    ks = {c["name"]: _plan_of(c["z_dims"], c["p"]) for c in E.CASES}
    assert all(P.served for P in ks.values())
    got = {n: (P.need_ks, P.KS) for n, P in ks.items() if n in ("A1", "A2", "A3", "A4", "A5")}
    assert got == {"A1": (4, 4), "A2": (6, 6), "A3": (7, 8), "A4": (8, 8), "A5": (2, 3)}
    got = {n: (P.need_ksf, P.KSF) for n, P in ks.items() if n[0] in "AF"}
    assert got == {"A1": (2, 2), "A2": (4, 4), "A3": (4, 4), "A4": (8, 8), "A5": (1, 1), "F5": (2, 2), "F8": (2, 2), "F13": (4, 4), "F16": (4, 4),
                   "F17": (5, 8), "F21": (6, 8), "F25": (7, 8)}
    assert [ks[c["name"]].NTL for c in E.B_CASES] == [1, 1, 2, 13, 11, 11]
    assert {KS for KS in (P.KS for P in ks.values())} == set(E.KS_TABLE)
    assert {P.KSF for P in ks.values()} == set(E.KSF_TABLE)
    # the many-item case: more items than eight times any grid the launcher can choose (grid <= n_cus), buffers under 0.5 GB
    for x3 in (False, True):
        c = E.many_case(E.MANY_N_CUS, x3)
        P = _plan_of(c["z_dims"], c["p"])
        n_blocks = c["n"] // c["bs"]
        assert E.groups_per_block(c["bs"]) == 1 and n_blocks * (2 if x3 else 1) > 8 * E.MANY_N_CUS
        assert n_blocks * 2 * P.set_floats * 4 < 0.5e9


@pytest.mark.parametrize("name", [c["name"] for c in E.CASES])
def test_case_has_few_fragile_rows_and_a_moving_sampler(name):
    c = E.BY_NAME[name]
    r = E.ref_mh(c)
    n_fragile, rate = int(r.fragile.sum()), r.acc.mean()
    print("%s: fragile rows %d of %d, acceptance %.3f" % (name, n_fragile, c["n"], rate))
    assert n_fragile <= 0.02 * c["n"]
    assert rate >= 0.25


@pytest.mark.parametrize("x3", [False, True])
def test_many_item_case_on_its_compared_blocks(x3):
    """The blocks the device test compares (first, middle, last) at the compute-unit count of an MI355X: no fragile row among them;
    acceptance over these and the first 60 blocks."""
    c = E.many_case(E.MANY_N_CUS, x3)
    _, m64, (z, x, y, v) = E.setup(c)
    cmp_blocks = E.many_blocks(c)
    r = E.run_mh(c, m64, x, y, v, z, blocks=sorted(set(range(60)) | set(cmp_blocks)))
    cmp_rows = np.concatenate([np.arange(b * c["bs"], (b + 1) * c["bs"]) for b in cmp_blocks])
    print("%s: fragile rows %d of %d compared, %d of %d run, acceptance %.3f" % (c["name"], r.fragile[cmp_rows].sum(), len(cmp_rows),
                                                                               r.fragile[r.rows].sum(), len(r.rows), r.acc[:, r.rows].mean()))
    assert not r.fragile[cmp_rows].any()
    assert r.fragile[r.rows].sum() <= 0.02 * len(r.rows)
    assert r.acc[:, r.rows].mean() >= 0.25
