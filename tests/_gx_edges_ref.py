"""What tests/test_gpu_gx_edges.py and tests/test_gx_edges_host.py share (imports without a GPU): the models and panels of the
general-width engine's edge suite, a restatement of the engine's plan (the LDS formulas of csrc/gx_causal_kernels.h, gx_fit_kernels.h,
gw_kernels.h and the choices of gx_session in csrc/gx_api.hip), and fragile_rows: the float64 chain of oracle/causal.py with the rows
whose accept decisions a float32 kernel may legitimately take the other way."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_widths import SHAPES as W_SHAPES, _as64, _data, _model  # noqa: E402,F401

from oracle import causal as OC  # noqa: E402
from oracle import rng as R       # noqa: E402

GX_ROWS = 32      # csrc/gx_device.h: rows of a workgroup's tile
GX_MAXDB = 4      # csrc/gx_causal_kernels.h: most doses per pass of the effect routine
GW_ROWS = 16      # csrc/gw_kernels.h: rows of a wave's tile
GW_WAVES = 4      # csrc/gw_kernels.h: waves (row tiles) per workgroup
LDS_BYTES = 160 * 1024

SHAPES = dict(W_SHAPES)
SHAPES.update({
    "w160": dict(g_units=(160,), e_units=(160,), f_units=(160,), h_units=(160,)),
    "odd": dict(g_units=(130, 200, 150), f_units=(8, 4), h_units=(10,), e_units=(130,)),
    "f-wide": dict(g_units=(8, 8), f_units=(300,), h_units=(8, 4), e_units=(8, 8)),
    "deep": dict(g_units=(160,) * 8, f_units=(160, 160), h_units=(160,), e_units=(160,)),
    "w129": dict(g_units=(129,), e_units=(129,), f_units=(129,), h_units=(129,)),
    "w576": dict(g_units=(576,), e_units=(576,), f_units=(576,), h_units=(576,)),
    "w577": dict(g_units=(577,), e_units=(577,), f_units=(577,), h_units=(577,)),
})


# ---------------------------------------------------------------------------------------------------------------------------
# the plan of gx_session, restated
# ---------------------------------------------------------------------------------------------------------------------------
def gx_pad32(n):
    return (n + 31) & ~31


def gx_ld(width):                                   # gx_device.h
    return ((width + 59) // 64) * 64 + 8


def gw_ld(width):                                   # gw_kernels.h
    return ((width + 63) // 64) * 64 + 4


def gx_causal_lds_floats(ld, q, ncg, ldf, db):      # gx_causal_kernels.h
    buf = GX_ROWS * max(ld, db * ldf)
    return 2 * buf + 2 * GX_ROWS * q + ncg * GX_ROWS + (6 + 2 * GX_MAXDB) * GX_ROWS + 64


def gx_fit_lds_floats(ld, q):                       # gx_fit_kernels.h
    return 2 * GX_ROWS * ld + GX_ROWS * q + 8 * GX_ROWS + 64


def gx_enc_lds_bytes(e_units, p, q):                # gx_session: kc, ld_enc, lds_enc
    wenc = max([32, gx_pad32(q)] + [gx_pad32(u) for u in e_units])
    kc = min(gx_pad32(p), max(wenc, 256))
    return 4 * 2 * GX_ROWS * gx_ld(max(wenc, kc))


def gw_wave_floats(ld, q, ldf, db):                 # gw_kernels.h
    buf = GW_ROWS * max(ld, db * ldf)
    return 2 * buf + ((2 * GW_ROWS * q + 3) & ~3) + 2 * GW_ROWS


def plan(units, z_dims, p, force_db=None):
    """The choices gx_session makes for a model: dict(ld, ldf, ncg, db, lds_bytes, lds_fit, lds_enc, served, gw, gw_wave_bytes,
    enc_occ).  force_db: the BGM_GX_DB override (kept only if it fits, as there)."""
    q = int(sum(z_dims))
    z0, z1, z2, _ = z_dims
    pads = lambda din, hid, dout: [gx_pad32(w) for w in [din] + list(hid) + [dout]]
    g = pads(q, units["g_units"], p + 1)
    f = pads(z0 + z1 + 1, units["f_units"], 2)
    h = pads(z0 + z2, units["h_units"], 2)
    wmax = max([32] + g[:-1] + f + h)
    wf = max([32] + f)
    ld, ldf, ncg = gx_ld(wmax), gx_ld(wf), g[-1] // 32
    occ_of = lambda b: max(1, min(4, LDS_BYTES // max(b, 1)))
    lds = lambda db: 4 * gx_causal_lds_floats(ld, q, ncg, ldf, db)
    db = 1
    for cand in (4, 3, 2):
        if lds(cand) <= LDS_BYTES and occ_of(lds(cand)) >= min(occ_of(lds(1)), 2):
            db = cand
            break
    if force_db is not None:
        want = max(1, min(GX_MAXDB, int(force_db)))
        if lds(want) <= LDS_BYTES:
            db = want
    gw_bytes = 4 * gw_wave_floats(gw_ld(wmax), q, gw_ld(wf), 1)
    lds_fit, lds_enc = 4 * gx_fit_lds_floats(ld, q), gx_enc_lds_bytes(units["e_units"], p, q)
    return dict(ld=ld, ldf=ldf, ncg=ncg, db=db, lds_bytes=lds(db), lds_fit=lds_fit, lds_enc=lds_enc,
                served=max(lds(db), lds_fit, lds_enc) <= LDS_BYTES, gw=gw_bytes <= 24 * 1024, gw_wave_bytes=gw_bytes,
                enc_occ=max(1, min(4, LDS_BYTES // lds_enc)))


# ---------------------------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------------------------
def fragile_rows(m, data, n_iter, q_sd, seed):
    """The float64 chain of OC.mh_transition (same RNG spec) over n_iter iterations -> (final state [n, q], flagged [n] bool, accepted
    rows per iteration [n_iter]).  A row is flagged if at any iteration |log u - min(lp_prop - lp_cur, 0)| < 2 (1e-5 max|lp| + 1e-3):
    twice the engine's own log-posterior bar, both terms of the ratio carry it -- a float32 kernel may take that decision either way."""
    m64 = OC.cast_model(m, np.float64)
    x, y, v = (np.asarray(a, np.float64) for a in data)
    n, q = len(x), int(sum(m["z_dims"]))
    rows = np.arange(n)
    state = OC.mh_init_state(n, q, seed).astype(np.float64)
    logp = OC.log_posterior(m64, x, y, v, state)
    flagged = np.zeros(n, bool)
    acc_hist = np.zeros(n_iter, np.int64)
    for it in range(n_iter):
        eps = R.normals(rows, it, q, R.TAG_PROP, seed).astype(np.float64)
        u = R.uniforms(rows, it, R.TAG_ACC, seed).astype(np.float64)
        prop = state + np.float64(q_sd) * eps
        lp_prop = OC.log_posterior(m64, x, y, v, prop)
        d = np.minimum(lp_prop - logp, 0.0)
        flagged |= np.abs(np.log(u) - d) < 2.0 * (1e-5 * np.maximum(np.abs(lp_prop), np.abs(logp)) + 1e-3)
        acc = u < np.exp(d)
        state = np.where(acc[:, None], prop, state)
        logp = np.where(acc, lp_prop, logp)
        acc_hist[it] = acc.sum()
    return state, flagged, acc_hist


Q_SD = 0.3
BURN, KEEP = 20, 15            # the 35-iteration chains (parts A and C)
B_BURN, B_KEEP = 5, 3          # the 8-iteration multi-trip chains (part B)
C_BURN, C_KEEP = 8, 5          # the 13-iteration chains at the gw / workgroup switch (part C)
CAP_35, CAP_8 = 0.15, 0.06     # largest flagged share of a panel: a condition on the inputs

# Part A: name, binary, p, z_dims, n, (model seed, data seed, sampler seed)
A_CASES = [
    dict(shape="w160", binary=False, p=31, z_dims=[1, 1, 1, 1], n=1),
    dict(shape="w160", binary=True, p=32, z_dims=[4, 4, 4, 4], n=1),
    dict(shape="w160", binary=False, p=32, z_dims=[4, 4, 4, 5], n=33),
    dict(shape="w160", binary=True, p=77, z_dims=[1, 1, 1, 1], n=33),
    dict(shape="odd", binary=False, p=77, z_dims=[4, 4, 4, 5], n=65),
    dict(shape="odd", binary=True, p=31, z_dims=[4, 4, 4, 4], n=33),
    dict(shape="odd", binary=False, p=32, z_dims=[1, 1, 1, 1], n=31),
    dict(shape="odd", binary=True, p=77, z_dims=[4, 4, 4, 5], n=32),
    dict(shape="f-wide", binary=False, p=31, z_dims=[4, 4, 4, 4], n=32),
    dict(shape="f-wide", binary=False, p=77, z_dims=[2, 5, 4, 6], n=65),
    dict(shape="deep", binary=False, p=32, z_dims=[1, 1, 1, 1], n=33),
    dict(shape="deep", binary=False, p=31, z_dims=[4, 4, 4, 5], n=31),
]
for _i, _c in enumerate(A_CASES):
    _c.update(model_seed=21, data_seed=22, seed=77 if _i % 2 else 1234567890123, burn=BURN, keep=KEEP)
A_CASES[7]["seed"] = 1234567890123      # (seed 77 flags 5 of its 32 rows: above the cap)


def case_id(c):
    return "%s-%s-p%d-q%d-n%d" % (c["shape"], "bin" if c["binary"] else "cont", c["p"], sum(c["z_dims"]), c["n"])


# the same model through both kernel families (part A, subprocess): continuous treatment
AB_CASES = [
    dict(shape="r_test", binary=False, p=4, z_dims=[1, 1, 1, 1], n=64, model_seed=21, data_seed=22, seed=77, burn=BURN, keep=KEEP),
    dict(shape="mixed", binary=False, p=77, z_dims=[2, 3, 4, 5], n=45, model_seed=21, data_seed=22, seed=1234567890123, burn=BURN, keep=KEEP),
    dict(shape="w128", binary=False, p=200, z_dims=[1, 1, 1, 7], n=65, model_seed=21, data_seed=22, seed=1234567890123, burn=BURN, keep=KEEP),
]

# Part C: the gw / workgroup switch (4 gw_wave_floats(132, q, 132, 1) = 24 576 B at q = 59, 24 704 B at q = 60) and the LDS limit
C_SWITCH = [
    dict(shape="w128", binary=False, p=20, z_dims=[15, 15, 15, 14], n=33, gw=True),
    dict(shape="w128", binary=False, p=20, z_dims=[15, 15, 15, 15], n=33, gw=False),
    dict(shape="w129", binary=False, p=20, z_dims=[1, 1, 1, 7], n=33, gw=False),
]
for _c in C_SWITCH:
    _c.update(model_seed=21, data_seed=22, seed=77, burn=C_BURN, keep=C_KEEP)
C_WIDE = dict(shape="w576", binary=False, p=20, z_dims=[1, 1, 1, 7], n=33, model_seed=21, data_seed=22, seed=77, burn=BURN, keep=KEEP)
C_DOSE = dict(shape="w160", binary=False, p=20, z_dims=[1, 1, 1, 7], n=65, model_seed=21, data_seed=22, seed=77, burn=BURN, keep=KEEP)
C_DOSE_NARROW_F = dict(shape="odd", binary=False, p=20, z_dims=[1, 1, 1, 7], n=65, model_seed=21, data_seed=22, seed=77, burn=BURN, keep=KEEP)


# Part B: panels sized by the device (n_cus workgroups at one per CU)
def rows_b_gx(n_cus):
    """Two full trips of n_cus workgroups of 32 rows, then two workgroups take a third trip, the last tile holding 5 rows."""
    return GX_ROWS * (2 * n_cus) + 37


def rows_b_gw(n_cus):
    """Two full trips of n_cus workgroups of GW_WAVES 16-row tiles, then two waves take a third, the last tile holding 5 rows."""
    return GW_ROWS * (2 * GW_WAVES * n_cus) + 21


def rows_b_enc(n_cus, occ=4):
    """The encoder runs min(4, 160 KB // lds_enc) workgroups per CU (gx_encode): one full trip and a ragged second one."""
    return GX_ROWS * (occ * n_cus) + 37


def b_cases(n_cus):
    return [
        dict(shape="w160", binary=False, p=4, z_dims=[1, 1, 1, 1], n=rows_b_gx(n_cus), tile=GX_ROWS, family="gx"),
        dict(shape="w160", binary=True, p=4, z_dims=[1, 1, 1, 1], n=rows_b_gx(n_cus), tile=GX_ROWS, family="gx"),
        dict(shape="r_test", binary=False, p=4, z_dims=[1, 1, 1, 1], n=rows_b_gw(n_cus), tile=GW_ROWS, family="gw"),
    ]


def b_case(n_cus, k):
    c = b_cases(n_cus)[k]
    c.update(model_seed=21, data_seed=22, seed=77, burn=B_BURN, keep=B_KEEP)
    return c


def build(c):
    """(units, model, (x, y, v)) of a case."""
    u = SHAPES[c["shape"]]
    m = _model(c["model_seed"], c["z_dims"], c["p"], c["binary"], **u)
    return u, m, _data(c["n"], c["p"], c["data_seed"], c["binary"])


def chain_cases(n_cus):
    """Every case whose chain the GPU file compares with fragile_rows, with the flagged share it may have at most."""
    out = [(c, CAP_35) for c in A_CASES + AB_CASES + C_SWITCH + [C_WIDE]]
    out += [(b_case(n_cus, k), CAP_8) for k in range(3)]
    return out
