"""Shared by test_gpu_bnw_edges.py (device) and test_bnw_edges_host.py (CPU): the run-time branches of the any-width Bayesian sampling
kernels (csrc/bnw_kernels.h bnw_gemm2 / bnw_gemm2_narrow, bnw_api.hip) restated as functions of the layer widths, the limits of the
fragment family the cases have to leave (csrc/bnn_sample_api.hip bns_plan), the case lists, and the float64 references (oracle/bnn.py) of
every case, computed once per process.  Nothing here touches a device."""
import functools
import types

import numpy as np

from oracle import bnn as OB
from _bnf_edges_ref import case, f64, run_mh          # (generic: a case record, the block-by-block Metropolis-Hastings oracle)

# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' constants and branches
# ---------------------------------------------------------------------------------------------------------------------------------
RT, KC, NP = 64, 16, 128            # BNW_RT rows of a workgroup tile, BNW_KC K of a chunk, BNW_NP output columns of a pass
MAX_LAYERS = 8                      # BNN_MAX_LAYERS: Flipout layers of a net (hidden + output)
BATCH_MAX_Q = 64                    # bnw_need: latent columns the batch statistics hold
# bns_plan (the LDS-fragment family, hidden widths <= 64): a session leaves it when one net breaks one of
BNS_MAXT = 4                        # ... a hidden width <= 16 * BNS_MAXT
BNS_MAXK = 208                      # ... the network input
BNS_SW = 32                         # ... the sign words of a row
BNS_MAXB = 1024                     # ... all biases of a net, every layer padded to whole 16-column tiles


def net_dims(c):
    """{net: [in, hidden ..., out]} of a case (bnn_fill, csrc/bnn_api.hip)."""
    z0, z1, z2, _ = c["z_dims"]
    q, p, u = sum(c["z_dims"]), c["p"], c["units"]
    return {"g": [q] + list(u["g_units"]) + [p + 1], "e": [p] + list(u["e_units"]) + [q],
            "f": [z0 + z1 + 1] + list(u["f_units"]) + [2], "h": [z0 + z2] + list(u["h_units"]) + [2]}


def sign_words(dims):
    return OB.sign_layout(dims)[2]


def bns_breaks(c):
    """The limits of bns_plan the case breaks: a set of "MAXT" | "MAXK" | "SW" | "MAXB" (empty: the fragment family would serve it)."""
    out = set()
    for d in net_dims(c).values():
        if max(d[1:-1]) > 16 * BNS_MAXT:
            out.add("MAXT")
        if d[0] > BNS_MAXK:
            out.add("MAXK")
        if sign_words(d) > BNS_SW:
            out.add("SW")
        if sum(16 * ((w + 15) // 16) for w in d[1:]) > BNS_MAXB:
            out.add("MAXB")
    return out


def tile_rows(c):
    """The distinct row counts B of the workgroup tiles of a case's blocks."""
    n, bs = c["n"], c["bs"]
    rows = set()
    for lo in range(0, n, bs):
        blk_n = min(bs, n - lo)
        rows |= {min(RT, blk_n - r) for r in range(0, blk_n, RT)}
    return sorted(rows)


def layers(dims):
    """One record per Flipout layer: K, N, hidden (not the last layer), narrow (bnw_gemm2_narrow: N <= 32), nt (its column tiles),
    passes (ceil(N / 128)) and last_pass (columns of the last pass) of the staged kernel, nc (chunks of 16 K), eoff (the layer's offset
    inside a perturbation set: the prefix sum of in * out), hoff (its input's offset per row inside the activations)."""
    out, e, h = [], 0, 0
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        out.append(types.SimpleNamespace(l=l, K=K, N=N, hidden=l < len(dims) - 2, narrow=N <= 32, nt=(N + 15) // 16, passes=(N + NP - 1) // NP,
                                         last_pass=N - NP * ((N - 1) // NP), nc=(K + KC - 1) // KC, eoff=e, hoff=h))
        e += K * N
        h += K
    return out


def vector_fetch(L, B):
    """bnw_gemm2's `vec`: lda = K and K multiples of 4 and the four operands 16-byte aligned -- the activations of the layer start at
    B * hoff floats of an aligned buffer, the transposed weights at eoff floats of an aligned set."""
    return L.K % 4 == 0 and (B * L.hoff) % 4 == 0 and L.eoff % 4 == 0


def all_layers(c):
    return [(k, L) for k, d in net_dims(c).items() for L in layers(d)]


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
ZD = (1, 1, 1, 7)
WIDE = dict(g_units=(128, 96), e_units=(100,), f_units=(80, 40), h_units=(72,))          # (test_gpu_bnn.py)
U = lambda g, e, f, h: dict(g_units=tuple(g), e_units=tuple(e), f_units=tuple(f), h_units=tuple(h))


def wcase(name, z_dims, p, n, bs, units, breaks, **kw):
    """A case of the any-width family: units = the four nets' hidden widths, breaks = the bns_plan limit it is here for, fixed = the
    input normalisation (True: inference mode, False: batch statistics), mseed / pseed = the seeds of _model / _panel."""
    kw.setdefault("fixed", True)
    kw.setdefault("mseed", 0)
    kw.setdefault("pseed", 1)
    return case(name, z_dims, p, n, bs, units=units, breaks=breaks, **kw)


def both_modes(c):
    """The case with inference-mode normalisation and with batch statistics (the default seeds of _model / _panel serve both: the
    conditions of test_bnw_edges_host.py hold for every variant)."""
    return [dict(c, name=c["name"] + "/fixed"), dict(c, name=c["name"] + "/batch", fixed=False)]


# A: layer-product edges.  What each reaches is asserted from the widths in test_bnw_edges_host.py.
A_BASE = [
    wcase("W-odd", ZD, 19, 150, 70, U((65, 33), (129,), (17, 5), (31,)), "MAXT"),
    wcase("W-32", (2, 3, 4, 6), 33, 150, 64, U((130, 66), (68,), (32, 33), (16, 15)), "MAXT", binary=True),
    wcase("W-k16", ZD, 16, 100, 65, U((80, 16, 17, 48), (72,), (17, 16), (80,)), "MAXT"),
    wcase("W-deep", ZD, 5, 100, 65, U((72,) * 7, (72,) * 7, (72,) * 7, (72,) * 7), "MAXT"),
    wcase("W-in", ZD, 300, 100, 100, U((64, 64), (64, 64), (64, 32, 8), (64, 32, 8)), "MAXK"),
    wcase("W-q80", (20, 20, 20, 20), 40, 100, 50, U((96,), (96,), (48,), (48,)), "MAXT"),
    wcase("W-pass", ZD, 128, 130, 130, U((129, 257), (128,), (256,), (127,)), "MAXT"),
    wcase("W-256", ZD, 120, 200, 70, U((256,) * 3, (256,) * 3, (256,) * 3, (256,) * 3), "MAXT"),
    wcase("W-ref", ZD, 50, 300, 128, WIDE, "MAXT"),
]
A_CASES = [v for c in A_BASE for v in both_modes(c) if v["fixed"] or sum(c["z_dims"]) <= BATCH_MAX_Q]

# B: rows, blocks and the item loop
SMALL = U((68,), (68,), (8,), (8,))
MANY_N_CUS = 256                    # compute units of an MI355X: the host check of the case below assumes it


def many_case(n_cus):
    """4 n_cus + 40 blocks of 2 rows = one item each: more items than the largest grid (4 n_cus workgroups), so every workgroup of
    bnw_rows_kernel / bnw_effects_kernel comes back for a second item.  Binary: the ITE is a per-row result."""
    n_blocks = 4 * n_cus + 40
    return wcase("B-many-%d" % n_cus, ZD, 4, 2 * n_blocks, 2, SMALL, "MAXT", binary=True, n_iters=1, q_sd=0.5)


def many_blocks(c):
    n_blocks = c["n"] // c["bs"]
    return (0, n_blocks // 2 + 1, n_blocks - 1)


B_TINY = [wcase("B-tiny-bs3", ZD, 11, 7, 3, WIDE, "MAXT"),                    # blocks of 3, 3, 1 rows
          wcase("B-tiny-bs2", ZD, 11, 7, 2, WIDE, "MAXT")]                    # the API's smallest block: 2, 2, 2, 1 rows
B_SHARE = wcase("B-share", ZD, 20, 230, 70, WIDE, "MAXT", binary=True, init=True, it_begin=0, n_iters=3, q_sd=0.4, seed=(2 << 32) | 555)
B_SHARE_RANGES = ((0, 70), (70, 210), (210, 230))          # whole blocks: the first, the two middle ones, the ragged last
B_STATS = [wcase("B-stats-bs%d" % bs, ZD, 20, 700, bs, SMALL, "MAXT", fixed=False) for bs in (257, 600)]
B_SCALE = both_modes(wcase("B-scale", ZD, 50, 300, 128, WIDE, "MAXT", q_sd=7.0, q_sd_blocks=(0.1, 0.5, 1.0)))      # the scalar is a decoy

# C: limits
Q64 = wcase("C-q64", (16, 16, 16, 16), 20, 100, 50, U((96,), (96,), (48,), (48,)), "MAXT", fixed=False)
Q65 = both_modes(wcase("C-q65", (17, 16, 16, 16), 20, 100, 50, U((96,), (96,), (48,), (48,)), "MAXT"))
PRECISION = wcase("C-f16x3", ZD, 20, 40, 24, U((128, 96), (64,) * 5, (64, 32, 8), (64, 32, 8)), "MAXT")
DEEP8 = U((72,) * 8, (72,) * 7, (72,) * 7, (72,) * 7)          # eight hidden layers: one more than a net holds

MH_CASES = A_CASES + B_TINY + B_STATS + B_SCALE + [Q64]          # compared with the oracle row by row (B-share: with itself; B-many: below)
CASES = MH_CASES + [B_SHARE, PRECISION] + Q65
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

LP_SEED, LP_STREAM, LP_BLOCK0 = (3 << 32) | 1234, 77, 2
EFF_SEED, EFF_IT0, EFF_BLOCK0, EFF_ROW_BASE = (3 << 32) | 1234, 3, 1, 40
EFF_DOSES = np.array([0.0, 0.9, 2.1], np.float32)
EVAL_SEED, EVAL_STREAM = 31337, 900
EVAL_DOSES = np.linspace(0.1, 2.5, 5).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# models, panels, references
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup(binary, z_dims, p, n, units, fixed, mseed, pseed):
    from test_gpu_bnn import _model, _panel          # (the family's own model and panel builders; importing them uses no device)
    m = _model(binary, z_dims=z_dims, p=p, seed=mseed, fixed=fixed, **dict(units))
    z, x, y, v = _panel(m, n, seed=pseed)
    for a in (z, x, y, v):
        a.setflags(write=False)
    return m, OB.cast_model(m, np.float64), (z, x, y, v)


def setup(c):
    """(model, float64 model, (z, x, y, v)) of a case; shared, read-only."""
    return _setup(c["binary"], c["z_dims"], c["p"], c["n"], tuple(sorted(c["units"].items())), c["fixed"], c["mseed"], c["pseed"])


def register(c):
    """A case made at run time (B-many: its size follows the device)."""
    BY_NAME.setdefault(c["name"], c)
    return c


def logpost_of(c, m, x, y, v, z):
    """The log posterior on the case's blocks under model m in m's precision."""
    t = m["g"]["gamma"].dtype.type
    a = lambda u: u.astype(t)
    return OB.log_posterior_blocks(m, a(x), a(y), a(v), a(z), c["bs"], LP_SEED, LP_STREAM, block0=LP_BLOCK0)


@functools.lru_cache(maxsize=None)
def _ref_logpost(name):
    c = BY_NAME[name]
    _, m64, (z, x, y, v) = setup(c)
    ref = logpost_of(c, m64, x, y, v, z)
    ref.setflags(write=False)
    return ref


def ref_logpost(c):
    return _ref_logpost(c["name"])


@functools.lru_cache(maxsize=None)
def _ref_logpost32(name):
    """float32 NumPy evaluation of the oracle: what the number format alone costs (the condition of a case's own bar)."""
    c = BY_NAME[name]
    m, _, (z, x, y, v) = setup(c)
    return f64(logpost_of(c, OB.cast_model(m, np.float32), x, y, v, z))


def ref_logpost32(c):
    return _ref_logpost32(c["name"])


@functools.lru_cache(maxsize=None)
def _ref_mh(name):
    c = BY_NAME[name]
    _, m64, (z, x, y, v) = setup(c)
    r = run_mh(c, m64, x, y, v, z)
    for a in (r.z, r.acc, r.fragile):
        a.setflags(write=False)
    return r


def ref_mh(c):
    return _ref_mh(c["name"])


def effect_draws(z):
    return np.stack([z, z[::-1].copy()])


def effects_of(c, m64, draws, d, lo=0, hi=None, block0=None):
    """Effects of draw d with outcome noise on rows [lo, hi) of the call (whole blocks; block0 = the first one's id): the ITE per row
    (binary) or the rows' outcomes per dose [n_doses, rows]."""
    hi = draws.shape[1] if hi is None else hi
    xv = [1.0, 0.0] if c["binary"] else f64(EFF_DOSES)
    r = OB.effects_draw(m64, f64(draws[d, lo:hi]), xv, d, EFF_IT0 + d, True, EFF_SEED, c["bs"], block0=EFF_BLOCK0 + lo // c["bs"] if block0 is None else block0,
                        row_base=EFF_ROW_BASE + lo)
    return r[0] - r[1] if c["binary"] else r


@functools.lru_cache(maxsize=None)
def _ref_effects(name):
    c = BY_NAME[name]
    _, m64, (z, _, _, _) = setup(c)
    draws = effect_draws(z)
    out = [effects_of(c, m64, draws, d) for d in range(2)]
    return np.stack(out) if c["binary"] else np.stack([o.mean(axis=1) for o in out], axis=1)          # ITE [2, n] | ADRF [n_doses, 2]


def ref_effects(c):
    return _ref_effects(c["name"])


@functools.lru_cache(maxsize=None)
def _ref_evaluate(name):
    c = BY_NAME[name]
    _, m64, (_, x, y, v) = setup(c)
    zr, cr, mse_x, mse_y, mse_v = OB.evaluate(m64, (f64(x), f64(y), f64(v)), None, EVAL_DOSES, EVAL_SEED, EVAL_STREAM)
    return types.SimpleNamespace(z=zr, causal=cr, mse_x=mse_x, mse_y=mse_y, mse_v=mse_v)


def ref_evaluate(c):
    return _ref_evaluate(c["name"])
