"""What tests/test_fit_epoch_host.py and tests/test_gpu_fit_epoch.py share (imports without a GPU and without torch): the case table of
the in-library fit epoch (bgm_causal_fit_epoch) and a plain-Python restatement of the dispatch it runs through -- the choices of
bgm_causal_fit_begin, fit_chain_setup, fit_chain_launch and fit_epoch_impl in csrc/fit_api.hip, read off the code, so that the CPU test
can prove from the table alone which kernel family, minibatch instantiation and ring edge every case reaches.

Run as a program (`python tests/_fit_epoch_cases.py NAME ...`, on a GPU) it runs the epoch call of the named cases and prints one
`NAME sha256` line per case: the child process of test_event_ordering_gives_the_same_bits, started with BGM_FIT_NO_FLAGS=1.  With
`--host` in front of the names the line carries a second digest, that of the host loop over the same minibatches in the same process:
the child processes of test_debug_switch_keeps_the_sequential_order, one per BGM_FIT_* switch.

The restatement covers g of at most five hidden layers (the forward blob of a deeper g may not fit the LDS, which changes the family:
tests/test_gpu_causal_depth.py) and no conditional latent prior."""
import os
import sys

ECH_THREADS = 512       # csrc/egm_chain.h: threads of a chain workgroup
RING_DEPTH = 4          # csrc/fit_api.hip fit_epoch_impl: parameter buffers in the ring when the two phases overlap
G5, FH = (64,) * 5, (64, 32, 8)
LR = 1e-3               # both learning rates of every case


def _case(name, p, n_use, lazy, B=32, z_dims=(1, 1, 1, 7), binary=False, n=320, g_units=G5, f_units=FH, h_units=FH):
    return dict(name=name, p=p, n_use=n_use, lazy=lazy, B=B, z_dims=tuple(z_dims), binary=binary, n=n, g_units=tuple(g_units),
                f_units=tuple(f_units), h_units=tuple(h_units))


T2 = dict(z_dims=(3, 3, 6, 6), binary=True)
# n_use at B = 32: 32 -> 1 minibatch, 49 -> 2 (17), 96 -> 3, 113 -> 4 (17), 129 -> 5 (1), 177 -> 6 (17), 256 -> 8, 272 -> 9 (16)
# (in brackets the rows of a short last minibatch)
CASES = [
    # ---- the headline shape: the unpadded 13-tile family, every ring edge in replay mode ...
    _case("p200-z2-mb1", 200, 32, 2), _case("p200-z2-mb2", 200, 49, 2), _case("p200-z2-mb3", 200, 96, 2),
    _case("p200-z2-mb4", 200, 113, 2), _case("p200-z2-mb5", 200, 129, 2), _case("p200-z2-mb8", 200, 256, 2),
    _case("p200-z2-mb9", 200, 272, 2),
    # ... and in batch-rows / dense mode (dense: one stream, one buffer)
    _case("p200-z1-mb1", 200, 32, 1), _case("p200-z1-mb3", 200, 96, 1), _case("p200-z1-mb4", 200, 113, 1),
    _case("p200-z1-mb5", 200, 129, 1), _case("p200-z1-mb9", 200, 272, 1),
    _case("p200-z0-mb1", 200, 32, 0), _case("p200-z0-mb4", 200, 113, 0), _case("p200-z0-mb5", 200, 129, 0),
    # ---- the edges of the unpadded 13-tile family
    _case("p192-z2", 192, 177, 2), _case("p207-z2", 207, 177, 2),
    # ---- the unpadded 7-tile family
    _case("p96-z2", 96, 177, 2), _case("p100-z2-mb9", 100, 272, 2), _case("p100-z1", 100, 177, 1),
    _case("p111-bin-z2", 111, 177, 2, binary=True), _case("p100-B16-z1", 100, 87, 1, B=16),
    # ---- the padded 13-tile family
    _case("p20-z2-mb3", 20, 96, 2), _case("p20-z2-mb9", 20, 272, 2), _case("p20-z1-mb3", 20, 96, 1), _case("p20-z1-mb9", 20, 272, 1),
    _case("p20-z0-mb4", 20, 113, 0), _case("p20-z1-mb4", 20, 113, 1), _case("p20-z2-mb4", 20, 113, 2),
    _case("p95-z2", 95, 177, 2), _case("p112-z2", 112, 177, 2),
    # ---- two latent input tiles
    _case("t2-z0-mb4", 100, 113, 0, **T2), _case("t2-z1-mb4", 100, 113, 1, **T2), _case("t2-z2-mb4", 100, 113, 2, **T2),
    _case("t2-z2-mb9", 100, 272, 2, **T2),
    # ---- models the chains decline: one stream, one buffer, the step kernels of another family
    _case("p208-z2", 208, 113, 2), _case("f32x8-z2", 200, 113, 2, f_units=(32, 8)), _case("g64-z2", 200, 113, 2, g_units=(64,)),
    _case("g96x96-z1", 50, 113, 1, g_units=(96, 96)),
    # ---- minibatch sizes on the headline shape (B = 17: 5 x 17 + 1 rows; B = 16: 5 x 16 + 7; B > 32: no overlap)
    _case("p200-B17-z2", 200, 86, 2, B=17), _case("p200-B16-z2", 200, 87, 2, B=16), _case("p200-B1-z2", 200, 6, 2, B=1),
    _case("p200-B33-z2", 200, 113, 2, B=33), _case("p200-B64-z2", 200, 200, 2, B=64),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

EVENT_CASES = ["p200-z1-mb3", "p200-z1-mb9", "p200-z2-mb3", "p200-z2-mb9", "p20-z1-mb3", "p20-z1-mb9", "p20-z2-mb3", "p20-z2-mb9"]
ORACLE_CASES = ["p200-z0-mb4", "p200-z1-mb4", "p200-z2-mb4", "t2-z0-mb4", "t2-z1-mb4", "t2-z2-mb4", "p20-z0-mb4", "p20-z1-mb4", "p20-z2-mb4"]
# unpadded with riders, a ring that wraps twice and a 16-row tail | padded, 17-row tail, copy-back from a non-zero slot | two latent tiles
SWITCH_CASES = ["p200-z2-mb9", "p20-z2-mb4", "t2-z1-mb4"]
# the development switches of the fit path (read once per process): those that only change how the epoch call orders the same launches ...
EPOCH_SWITCHES = ["BGM_FIT_NO_OVERLAP=1", "BGM_FIT_NO_FUSED_ADAM=1", "BGM_FIT_NO_REPLAY_AHEAD=1", "BGM_FIT_EPOCH_DEPTH=2", "BGM_FIT_EPOCH_DEPTH=3"]
# ... and those that change the kernel variant or family of both the epoch call and the host loop
VARIANT_SWITCHES = ["BGM_FIT_ONE_WG=1", "BGM_FIT_NO_WORKERS=1", "BGM_FIT_NO_CHAIN=1"]
OUTSIDE_CASES = ["p200-z0-mb5", "p200-z1-mb5", "p200-z2-mb5"]          # rows outside the permutation, one n_use in all three modes


# ---------------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
def blob_shape(q1, p1):
    """bgm_causal_shape (csrc/bgm_host.h): does an LDS-resident compiled shape hold q + 1 latent inputs and p + 1 outputs of g?"""
    if q1 <= 12:
        big = 13
    elif q1 <= 20:
        big = 10
    else:
        return False
    return (p1 + 15) // 16 <= big


def general_width(g_units, f_units, h_units):
    """gx_wanted (csrc/gx_api.hip): hidden widths other than g [64] x k, f / h [64, 32, 8] are fitted by the general-width engine."""
    return not (all(u == 64 for u in g_units) and tuple(f_units) == FH and tuple(h_units) == FH)


def chain_setup(p, z_dims, g_units, f_units, h_units):
    """fit_chain_setup: None when the row-tile chains decline the model, else (ntl, t0, pad)."""
    q = sum(z_dims)
    ntl_need = (p + 1 + 15) // 16
    t0 = 1 if q <= 16 else 2
    ntl = ntl_need if (ntl_need in (13, 7) and t0 == 1) else 13
    ok = q <= 32 and ntl_need <= 13
    ok = ok and len(g_units) + 1 >= 3 and all(u == 64 for u in g_units)
    for units, n_in in ((f_units, z_dims[0] + z_dims[1] + 1), (h_units, z_dims[0] + z_dims[2])):
        ok = ok and len(units) == 3 and n_in <= 16 and units[0] == 64 and units[1] == 32 and 1 <= units[2] <= 16
    if not ok:
        return None
    return ntl, t0, (ntl != ntl_need or t0 == 2)


def plan(p, z_dims, g_units, f_units, h_units, B, lazy, n_use, **_):
    """What one bgm_causal_fit_epoch call over n_use rows in minibatches of B does, in a session opened with fit_begin(N, B)."""
    assert len(g_units) <= 5, "outside the restatement: the forward blob of a deeper g may not fit the LDS"
    q = sum(z_dims)
    out = dict(chain=False, ntl=None, t0=None, pad=None)
    if general_width(g_units, f_units, h_units):
        family = "gx"                                         # bgm_causal_fit_begin: gx_fit_begin before anything else
    else:
        cs = chain_setup(p, z_dims, g_units, f_units, h_units)
        if not blob_shape(q + 1, p + 1):                      # chain_only: the chains where they apply (max_batch <= 32), else gx
            family = "chain" if (B <= 32 and cs) else "gx"
        else:                                                 # the LDS-blob session, the chains beside it for minibatches <= 32
            family = "chain" if (B <= 32 and cs) else "blob"
        if family == "chain":
            out.update(chain=True, ntl=cs[0], t0=cs[1], pad=cs[2])
    out["family"] = family
    n_mb = (n_use + B - 1) // B
    sizes = [min(B, n_use - k * B) for k in range(n_mb)]
    out["n_mb"], out["sizes"] = n_mb, sizes
    mbs = []
    for b in sizes:                                           # fit_chain_launch
        nb = 1 if b <= 16 else 2
        nchain = 2 if (out["chain"] and out["t0"] != 2 and not out["pad"] and nb == 2) else 1
        inst = None
        if out["chain"]:
            inst = "T2" if out["t0"] == 2 else "PAD" if out["pad"] else "FS%d" % out["ntl"] if nb == 2 else "FW%d" % out["ntl"]
        mbs.append(dict(rows=b, nb=nb, nchain=nchain, inst=inst))
    out["minibatches"] = mbs
    overlap = lazy != 0 and out["chain"] and B <= 32          # fit_epoch_impl
    D = RING_DEPTH if overlap else 1
    out["overlap"], out["D"] = overlap, D
    out["ring_ends_on_slot0"] = n_mb % D == 0                 # else: the copy-back into the session's own buffers
    ahead = overlap and lazy == 2
    out["replays_at_entry"] = [d for d in range(1, D) if ahead and d < n_mb]       # replay(d) beyond the list returns at once
    out["replays_beyond_the_list"] = [d for d in range(1, D) if ahead and d >= n_mb]
    riders = []                                               # latent phase k carries the replay of minibatch k + D
    for k in range(n_mb):
        if ahead and k + D < n_mb:
            rows = sizes[k + D]
            riders.append(dict(on=k, target=k + D, rows=rows, blocks=(rows * q * 16 + ECH_THREADS - 1) // ECH_THREADS,
                               first_block=mbs[k]["nchain"]))
    out["riders"] = riders
    out["rider_targets_short"] = any(r["rows"] < B for r in riders)
    out["waits_on_ring_slot"] = overlap and n_mb > D          # theta phase k >= D waits for the latent phase k - D
    return out


def plan_of(case):
    return plan(**case)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests.test_gpu_fit_epoch import _run, digest
    host = sys.argv[1:2] == ["--host"]
    for name in sys.argv[1 + host:]:
        print(name, *[digest(_run(BY_NAME[name], epoch)) for epoch in ((True, False) if host else (True,))], flush=True)
