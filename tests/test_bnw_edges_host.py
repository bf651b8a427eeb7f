"""Conditions of test_gpu_bnw_edges.py that need no device.  From the widths alone (_bnw_edges_ref.py restates the branches of
csrc/bnw_kernels.h): every case leaves the LDS-fragment family by the bns_plan limit it names, and reaches the branch of the layer product
it is in the table for -- K % 4 and the alignment of the eoff prefix sums (vector or element-wise fetch), N <= 32 in a hidden layer (the
K-split kernel, one or two column tiles), ceil(N / 128) passes, the parity of ceil(K / 16) chunks.  From the float64 oracle alone: every
Metropolis-Hastings case has at most 2 % of its rows with an accept decision within 1e-3 of its uniform (such rows are excused from the
state comparison), accepts some proposals but not all (neither a frozen sampler nor one that ignores the target can pass), and has a
log posterior whose float32 NumPy evaluation lies within a quarter of the bar (2e-5 max|ref| + 2e-3) of float64: no case needs a bar of
its own."""
import numpy as np
import pytest

import _bnw_edges_ref as W

A = {c["name"]: c for c in W.A_BASE}


def _layers(c):
    return {k: W.layers(d) for k, d in W.net_dims(c).items()}


def test_every_case_leaves_the_fragment_family_by_the_limit_it_names():
    for c in W.CASES + [W.many_case(W.MANY_N_CUS)]:
        assert c["breaks"] in W.bns_breaks(c), (c["name"], W.bns_breaks(c))
        assert all(len(d) - 1 <= W.MAX_LAYERS for d in W.net_dims(c).values()), c["name"]
    assert W.bns_breaks(A["W-in"]) == {"MAXK"}          # default-type widths: here for the input width alone
    assert any(len(d) - 1 > W.MAX_LAYERS for d in W.net_dims(dict(A["W-deep"], units=W.DEEP8)).values())
    # the limits themselves
    ok = W.wcase("ok", W.ZD, 207, 10, 10, W.U((64,), (64,), (64,), (64,)), None)
    assert W.bns_breaks(ok) == set()
    assert W.bns_breaks(dict(ok, units=W.U((65,), (64,), (64,), (64,)))) == {"MAXT"}
    assert W.bns_breaks(dict(ok, p=209)) == {"MAXK"} and W.bns_breaks(dict(ok, p=208)) == set()          # (g's output p + 1 is no input)
    assert W.bns_breaks(dict(ok, units=W.U((64,) * 5, (64,), (64,), (64,)))) == set()
    assert W.bns_breaks(dict(ok, units=W.U((64,) * 7, (64,), (64,), (64,)))) == {"SW"}          # 36 sign words per row of g


def test_odd_widths_reach_the_element_wise_fetch_and_the_k_split_kernel():
    c = A["W-odd"]
    L = _layers(c)
    assert W.tile_rows(c) == [6, 10, 64]
    for k, Ls in L.items():
        for l in Ls:
            assert l.K % 4 != 0 and not any(W.vector_fetch(l, B) for B in W.tile_rows(c)), (k, l.l)
    assert (L["g"][1].K, L["g"][1].N) == (65, 33) and L["g"][2].eoff == 10 * 65 + 65 * 33 and L["g"][2].eoff % 4 != 0
    narrow_hidden = {(k, l.N): l.nt for k, Ls in L.items() for l in Ls if l.hidden and l.narrow}
    assert narrow_hidden == {("f", 17): 2, ("f", 5): 1, ("h", 31): 2}
    assert (L["g"][-1].N, L["g"][-1].narrow, L["g"][-1].nt) == (20, True, 2)
    assert (L["e"][0].N, L["e"][0].passes, L["e"][0].last_pass) == (129, 2, 1)


def test_the_narrow_wide_switch_and_the_single_chunk():
    c = A["W-32"]
    L = _layers(c)
    assert [(l.N, l.narrow) for l in L["f"][:2]] == [(32, True), (33, False)] and L["f"][0].hidden and L["f"][0].nt == 2
    assert [(l.K, l.nc, l.K % W.KC) for l in L["h"][1:]] == [(16, 1, 0), (15, 1, 15)]
    assert L["g"][-1].N == 34 and not L["g"][-1].narrow
    assert c["bs"] == W.RT and W.tile_rows(c) == [22, 64]
    c = A["W-k16"]
    L = _layers(c)
    assert [(l.K, l.nc) for l in L["g"]] == [(10, 1), (80, 5), (16, 1), (17, 2), (48, 3)]          # 16 -> 17: 1 -> 2 chunks; an odd count after an even one
    assert [(l.N, l.narrow, l.hidden) for l in L["g"][1:4]] == [(16, True, True), (17, True, True), (48, False, True)]
    assert (L["e"][0].K, L["e"][0].nc, L["e"][0].narrow) == (16, 1, False)          # the staged kernel with a single chunk
    assert (L["f"][1].K, L["f"][1].N, L["f"][1].narrow) == (17, 16, True)
    assert W.tile_rows(c) == [1, 35, 64]          # bs = 65: the block's second tile is one row


def test_depth_input_width_latent_width_and_passes():
    assert all(len(d) - 1 == W.MAX_LAYERS for d in W.net_dims(A["W-deep"]).values())
    c = A["W-in"]
    L = _layers(c)
    e0 = L["e"][0]
    assert e0.K == 300 > W.BNS_MAXK and all(W.vector_fetch(e0, B) for B in W.tile_rows(c))
    assert e0.K // W.KC == 18 and e0.nc == 19 and e0.K % W.KC == 12          # 18 chunks of whole 16-byte pieces and a tail
    assert (L["g"][-1].N, L["g"][-1].passes, L["g"][-1].last_pass) == (301, 3, 45)
    assert sum(A["W-q80"]["z_dims"]) == 80 > W.BATCH_MAX_Q
    assert [v["name"] for v in W.A_CASES if v["name"].startswith("W-q80")] == ["W-q80/fixed"]
    assert sorted(v["name"] for v in W.A_CASES) == sorted([n + "/fixed" for n in A] + [n + "/batch" for n in A if n != "W-q80"])
    c = A["W-pass"]
    L = _layers(c)
    assert [(l.N, l.passes, l.last_pass) for l in L["g"][:2]] == [(129, 2, 1), (257, 3, 1)]
    assert (L["e"][0].N, L["e"][0].passes, L["e"][0].last_pass) == (128, 1, 128) and (L["f"][0].N, L["f"][0].passes, L["f"][0].last_pass) == (256, 2, 128)
    assert L["h"][0].N == 127 and W.tile_rows(c) == [2, 64]
    assert all(u == (256,) * 3 for u in A["W-256"]["units"].values()) and A["W-256"]["p"] == 120
    from test_gpu_bnn import WIDE
    assert A["W-ref"]["units"] == WIDE


def test_the_table_reaches_every_branch_of_the_layer_product():
    seen = set()
    for c in W.A_BASE:
        for k, l in W.all_layers(c):
            vec = {W.vector_fetch(l, B) for B in W.tile_rows(c)}
            seen |= {("vec", v) for v in vec}
            if l.narrow:
                seen.add(("narrow", l.hidden, l.nt))
                seen.add(("narrow chunks", min(l.nc, 5)))          # 1 .. 4: waves without a chunk; 5: a wave with two
            else:
                seen.add(("passes", min(l.passes, 3)))
                seen.add(("chunks", 1 if l.nc == 1 else "odd" if l.nc % 2 else "even"))
                if True in vec and l.K % W.KC:
                    seen.add("tail past the whole chunks")
    want = {("vec", True), ("vec", False), ("narrow", True, 1), ("narrow", True, 2), ("narrow", False, 1), ("narrow", False, 2),
            ("passes", 1), ("passes", 2), ("passes", 3), ("chunks", 1), ("chunks", "odd"), ("chunks", "even"), "tail past the whole chunks"}
    want |= {("narrow chunks", k) for k in (1, 2, 3, 4, 5)}
    assert want <= seen, want - seen


def test_rows_blocks_and_the_item_loop():
    c = W.many_case(W.MANY_N_CUS)
    n_blocks = c["n"] // c["bs"]
    assert (c["bs"] + W.RT - 1) // W.RT == 1 and n_blocks > 4 * W.MANY_N_CUS          # one item per block, more items than the largest grid
    set_floats = sum(l.K * l.N for k, l in W.all_layers(c) if k != "e")
    assert 2 * n_blocks * set_floats * 4 < 64e6
    assert [W.tile_rows(t) for t in W.B_TINY] == [[1, 3], [1, 2]]
    assert [(s["bs"] + 255) // 256 for s in W.B_STATS] == [2, 3] and all(not s["fixed"] and s["n"] == 700 for s in W.B_STATS)
    bs, n = W.B_SHARE["bs"], W.B_SHARE["n"]
    assert all(lo % bs == 0 and (hi % bs == 0 or hi == n) for lo, hi in W.B_SHARE_RANGES) and W.B_SHARE_RANGES[0][0] == 0
    assert [r[1] for r in W.B_SHARE_RANGES[:-1]] == [r[0] for r in W.B_SHARE_RANGES[1:]] and W.B_SHARE_RANGES[-1][1] == n
    assert sum(W.Q64["z_dims"]) == W.BATCH_MAX_Q and all(sum(v["z_dims"]) == W.BATCH_MAX_Q + 1 for v in W.Q65)


@pytest.mark.parametrize("name", [c["name"] for c in W.MH_CASES])
def test_case_has_few_fragile_rows_and_a_moving_sampler(name):
    c = W.BY_NAME[name]
    r = W.ref_mh(c)
    n_fragile, rate = int(r.fragile.sum()), r.acc.mean()
    print("%s: fragile rows %d of %d, acceptance %.3f" % (name, n_fragile, c["n"], rate))
    assert n_fragile <= 0.02 * c["n"]
    assert 0.0 < rate < 1.0 and all(0 < a < c["n"] for a in r.acc.sum(axis=1))
    # the log-posterior bar is not the number format's: a float32 NumPy evaluation of the oracle stays under a quarter of it
    ref = W.ref_logpost(c)
    e32, bar = np.abs(W.ref_logpost32(c) - ref).max(), 2e-5 * np.abs(ref).max() + 2e-3
    print("%s: float32 oracle %.2e from float64, %.4f of the bar" % (name, e32, e32 / bar))
    assert e32 < 0.25 * bar


def test_many_item_case_on_its_compared_blocks():
    """The blocks the device test compares (first, middle, last) at the compute-unit count of an MI355X: no fragile row among them;
    acceptance over these and the first 60 blocks."""
    c = W.register(W.many_case(W.MANY_N_CUS))
    _, m64, (z, x, y, v) = W.setup(c)
    cmp_blocks = W.many_blocks(c)
    r = W.run_mh(c, m64, x, y, v, z, blocks=sorted(set(range(60)) | set(cmp_blocks)))
    cmp_rows = np.concatenate([np.arange(b * c["bs"], (b + 1) * c["bs"]) for b in cmp_blocks])
    rate = r.acc[:, r.rows].mean()
    print("%s: fragile rows %d of %d compared, %d of %d run, acceptance %.3f" % (c["name"], r.fragile[cmp_rows].sum(), len(cmp_rows),
                                                                               r.fragile[r.rows].sum(), len(r.rows), rate))
    assert not r.fragile[cmp_rows].any()
    assert r.fragile[r.rows].sum() <= 0.02 * len(r.rows)
    assert 0.0 < rate < 1.0
