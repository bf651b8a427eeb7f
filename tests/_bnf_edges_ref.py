"""Shared by test_gpu_bnf_edges.py (device) and test_bnf_edges_host.py (CPU): the shape table of the default-shape Bayesian sampling
kernels restated from csrc/bnf_build.h, the case lists, and the float64 references (oracle/bnn.py) of every case, computed once per
process.  Nothing here touches a device."""
import functools
import types

import numpy as np

from oracle import bnn as OB

KS_TABLE = (3, 4, 5, 6, 8)          # kBnfKS: compiled first-layer k-step counts of the sampler
KSF_TABLE = (1, 2, 3, 4, 8)         # kBnfKSF: ... of the outcome net in the effects kernel
LDS_LIMIT = 160 * 1024
MAX_DOSES = 256                     # BNF_MAX_DOSES
R_TILES, WAVES = 2, 8               # BNF_R / BNF_W = BNX_R / BNX_W: row tiles per wave, waves per workgroup


def plan(q, p, z0, z1):
    """bnf_build's plan for a Bayesian session with the default widths: .served, .KS, .KSF (compiled k-steps; need_ks / need_ksf are
    the steps the inputs fill), .NTL, .lds_bytes, .set_floats / .e_set_floats (one perturbation set of the sampler / effects kernel)."""
    P = types.SimpleNamespace(served=False, KS=0, KSF=0, NTL=0, lds_bytes=0, set_floats=0, e_set_floats=0, need_ks=(q + 1 + 3) // 4,
                              need_ksf=(z0 + z1 + 1 + 3) // 4)
    if q < 1 or q > 31 or p < 4 or p + 1 > 208:
        return P
    P.KS = next((k for k in KS_TABLE if k >= P.need_ks), 0)
    P.KSF = next((k for k in KSF_TABLE if k >= P.need_ksf), 0)
    if not P.KS or not P.KSF:
        return P
    T0, P.NTL = (P.KS + 3) // 4, (p + 1 + 15) // 16
    head = 4 * T0 + 11
    n_frags = 4 * T0 + 64 + 4 * P.NTL + 2 * head
    tail = 16 * (20 + P.NTL + 16) + 3 * T0 * 32 + 3 * T0 * 16
    P.lds_bytes = (n_frags * 256 + tail) * 4
    P.set_floats = n_frags * 256
    P.e_set_floats = (4 * ((P.KSF + 3) // 4) + 11) * 256
    P.served = P.lds_bytes <= LDS_LIMIT          # above it the plan is "wide": deterministic nets only
    return P


def groups_per_block(bs):
    return ((bs + 15) // 16 + R_TILES - 1) // R_TILES


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = dict(binary=False, q_sd=0.3, q_sd_blocks=None, it_begin=5, n_iters=2, row_base=1000, block0=0, init=False,
                 seed=(9 << 32) | 4321, sigmas=None)


def case(name, z_dims, p, n, bs, **kw):
    c = dict(_DEFAULTS, name=name, z_dims=tuple(z_dims), p=p, n=n, bs=bs)
    c.update(kw)
    return c


# A: every compiled first-layer instance (log posterior, MH, MH with fused effects)
A_CASES = [
    case("A1", (2, 3, 4, 6), 60, 150, 33),                     # q = 15: KS = 4, odd block size
    case("A2", (6, 6, 6, 5), 30, 120, 50),                     # q = 23: KS = 6 full
    case("A3", (7, 7, 7, 6), 50, 150, 64, binary=True),        # q = 27: KS = 7 padded to 8, f input 15 (KSF = 4)
    case("A4", (16, 15, 0, 0), 40, 100, 100),                  # q = 31: KS = 8 full; f input 32 (bit 0 of the sign word), KSF = 8 full
    case("A5", (0, 0, 3, 2), 20, 100, 17),                     # z0 + z1 = 0: f reads the treatment alone
]
# effects only: the remaining outcome-net instances and their padded steps (f input = z0 + z1 + 1)
EFFECT_CASES = [
    case("F5", (2, 2, 1, 2), 20, 80, 33),                      # f input 5: KSF = 2, half filled
    case("F8", (3, 4, 2, 1), 20, 80, 33, binary=True),         # f input 8: KSF = 2 full
    case("F13", (6, 6, 1, 1), 20, 80, 33),                     # f input 13: KSF = 4, first column of its last step
    case("F16", (8, 7, 1, 1), 20, 80, 33, binary=True),        # f input 16: KSF = 4 full
    case("F17", (8, 8, 1, 1), 20, 80, 33),                     # f input 17: KSF = 5 padded to 8, the treatment alone in the second k-tile
    case("F21", (10, 10, 2, 2), 20, 80, 33, binary=True),      # f input 21: KSF = 6 padded to 8
    case("F25", (12, 12, 1, 1), 20, 80, 33),                   # f input 25: KSF = 7 padded to 8
]
# B: output tiles of g and the largest LDS footprints
B_CASES = [
    case("B-p4", (1, 1, 1, 7), 4, 100, 48),                    # one output tile
    case("B-p15", (1, 1, 1, 7), 15, 100, 48),                  # variance column = last column of the only tile
    case("B-p16", (1, 1, 1, 7), 16, 100, 48),                  # variance column alone in the second tile
    case("B-p207", (1, 1, 1, 7), 207, 100, 48),                # p + 1 = 208: the last admitted width, last bit of the output sign words
    case("B-q16-p175", (4, 4, 4, 4), 175, 100, 48),            # 161 856 B of LDS: the largest plan that is still served
    case("B-q31-p175", (8, 8, 8, 7), 175, 100, 48),            # ... with KS = 8
]
# D: options
D_SCALE = case("D-scale", (1, 1, 1, 7), 50, 300, 128, q_sd=7.0, q_sd_blocks=(0.1, 0.5, 1.0))      # the scalar is a decoy
D_SIGMA = case("D-sigma", (3, 3, 6, 6), 100, 130, 40, binary=True, sigmas=dict(sigma_v=0.8, sigma_x=1.3, sigma_y=0.6))
D_SHARE = [case("D-share-%s" % ("binary" if b else "continuous"), (1, 1, 1, 7), 50, 100, 100, binary=b, block0=3, row_base=500, init=True,
                 it_begin=0, n_iters=5, q_sd=0.4, seed=(2 << 32) | 555) for b in (True, False)]
# E: item queues
E_TINY = case("E-tiny", (1, 1, 1, 7), 4, 121, 2)               # 61 blocks of 2 rows, the last one of 1 row; more items than XCDs, fewer than waves
E_ONE = case("E-one", (1, 1, 1, 7), 50, 20, 32)                # one item: seven of the eight XCD queues are empty
MANY_N_CUS = 256                                                # compute units of an MI355X: the host check of the case below assumes it


def many_case(n_cus, x3=False):
    """8 n_cus + 40 blocks of 2 rows: with one item per block every XCD's queue is longer than the waves that serve it, so every
    wave comes back for a second item.  Split precision evaluates (item, state) units, two per item: half the blocks."""
    n_blocks = (8 * n_cus + 40) // (2 if x3 else 1)
    return case("E-many-%s%d" % ("x3-" if x3 else "", n_cus), (1, 1, 1, 7), 4, 2 * n_blocks, 2, n_iters=1, q_sd=0.5)


def many_blocks(c):
    n_blocks = c["n"] // c["bs"]
    return (0, n_blocks // 2 + 1, n_blocks - 1)


MH_CASES = A_CASES + B_CASES + [D_SCALE, D_SIGMA] + D_SHARE + [E_TINY, E_ONE]
CASES = MH_CASES + EFFECT_CASES
BY_NAME = {c["name"]: c for c in CASES}

LP_SEED, LP_STREAM, LP_BLOCK0 = (3 << 32) | 1234, 77, 2

# C: dispatch boundaries, (z_dims, p)
SERVED_SHAPES = [((1, 1, 1, 7), 4), ((1, 1, 1, 7), 207), ((16, 15, 0, 0), 40), ((4, 4, 4, 4), 175), ((2, 3, 4, 6), 207)]
UNSERVED_SHAPES = [((1, 1, 1, 7), 3), ((1, 1, 1, 7), 208), ((8, 8, 8, 8), 20), ((4, 4, 4, 4), 176)]
DOSE_COUNTS = (1, 16, 17, 32, 256, 257)


# ---------------------------------------------------------------------------------------------------------------------------------
# models, panels, references
# ---------------------------------------------------------------------------------------------------------------------------------
f64 = lambda a: a.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _setup(binary, z_dims, p, n, sigmas):
    from test_gpu_bnf import _model, _panel          # (the family's own model and panel builders; importing them uses no device)
    m = _model(binary, z_dims=z_dims, p=p)
    if sigmas:
        m.update(dict(sigmas))
    z, x, y, v = _panel(m, n)
    for a in (z, x, y, v):
        a.setflags(write=False)
    return m, OB.cast_model(m, np.float64), (z, x, y, v)


def setup(c, n=None):
    """(model, float64 model, (z, x, y, v)) of a case; shared, read-only."""
    return _setup(c["binary"], c["z_dims"], c["p"], c["n"] if n is None else n, tuple(sorted(c["sigmas"].items())) if c["sigmas"] else None)


@functools.lru_cache(maxsize=None)
def _ref_logpost(name):
    c = BY_NAME[name]
    _, m64, (z, x, y, v) = setup(c)
    ref = OB.log_posterior_blocks(m64, f64(x), f64(y), f64(v), f64(z), c["bs"], LP_SEED, LP_STREAM, block0=LP_BLOCK0)
    ref.setflags(write=False)
    return ref


def ref_logpost(c):
    return _ref_logpost(c["name"])


def mh_iteration_blocks(m, x, y, v, z, it, q_sd_blocks, seed, block_rows, block0=0, row_base=0):
    """OB.mh_iteration block by block: block b runs with block0 + b, row_base + its first row and its own proposal scale
    q_sd_blocks[b].  Returns (new z, accepted, lp of the proposals, lp of the current states)."""
    n = len(z)
    out, acc, lpp, lpc = z.copy(), np.zeros(n, bool), np.empty(n, z.dtype), np.empty(n, z.dtype)
    for b, lo in enumerate(range(0, n, block_rows)):
        hi = min(n, lo + block_rows)
        out[lo:hi], acc[lo:hi], lpp[lo:hi], lpc[lo:hi] = OB.mh_iteration(m, x[lo:hi], y[lo:hi], v[lo:hi], z[lo:hi], it, q_sd_blocks[b], seed,
                                                                         block_rows, block0=block0 + b, row_base=row_base + lo)
    return out, acc, lpp, lpc


def run_mh(c, m64, x, y, v, z, blocks=None):
    """The case's Metropolis-Hastings iterations in float64, for all rows or for the listed blocks only (each block is its own run).
    Returns an object with .z (final state), .acc [n_iters, n] (accept decisions), .fragile [n] (a decision within 1e-3 of its
    uniform in some iteration), .rows (the rows run)."""
    n, bs, q = c["n"], c["bs"], len(z[0])
    n_blocks = (n + bs - 1) // bs
    rows = np.arange(n) if blocks is None else np.concatenate([np.arange(b * bs, min(n, (b + 1) * bs)) for b in blocks])
    zo = f64(z)
    if c["init"]:
        zo = f64(OB.R.normals(np.arange(c["row_base"], c["row_base"] + n), 0, q, OB.R.TAG_INIT, c["seed"]))
    sds = c["q_sd_blocks"] if c["q_sd_blocks"] is not None else (c["q_sd"],) * n_blocks
    acc = np.zeros((c["n_iters"], n), bool)
    fragile = np.zeros(n, bool)
    # whole panel: one range of all blocks; listed blocks: one range per block
    ranges = [(0, n, 0)] if blocks is None else [(b * bs, min(n, (b + 1) * bs), b) for b in blocks]
    for lo, hi, b0 in ranges:
        zb = zo[lo:hi]
        for i in range(c["n_iters"]):
            it = c["it_begin"] + i
            zb, a, lpp, lpc = mh_iteration_blocks(m64, f64(x[lo:hi]), f64(y[lo:hi]), f64(v[lo:hi]), zb, it, sds[b0:], c["seed"], bs,
                                                  block0=c["block0"] + b0, row_base=c["row_base"] + lo)
            u = OB.R.uniforms(np.arange(c["row_base"] + lo, c["row_base"] + hi), it, OB.R.TAG_ACC, c["seed"])
            acc[i, lo:hi] = a
            fragile[lo:hi] |= np.abs(u - np.exp(np.minimum(lpp - lpc, 0))) < 1e-3
        zo[lo:hi] = zb
    return types.SimpleNamespace(z=zo, acc=acc, fragile=fragile, rows=rows)


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
