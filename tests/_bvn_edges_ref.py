"""What tests/test_gpu_bvn_edges.py, tests/test_bvn_edges_host.py and tests/_bvn_edges_helper.py share (NumPy only, imports without a
device): the host plans behind the bgm_bvn_* entry points restated as functions of the shape (each names the C++ it restates), route(),
the case tables, the nets and panels of the cases, and chains64: the float64 chain of oracle/bgm_bnn.py::hmc_sampler at a fixed step
size with the rows whose accept decisions a float32 kernel may legitimately take the other way."""
import functools
import types

import numpy as np

from oracle import bgm_bnn as OV
from oracle import bnn as OB
from oracle import rng as R

LDS_LIMIT = 160 * 1024            # what bgmf_session and gxf_session compare their LDS need with
BGMB_RT = 64                      # csrc/bgmb_kernels.h: rows of a workspace tile at most
BNN_MAX_LAYERS = 8                # csrc/bnn_kernels.h: Flipout layers of a net (trunk + the two heads)
GX_ROWS, GX_MAXL = 32, 9          # csrc/gx_device.h
BGM_PAIR = 2 * 64 * 17            # csrc/bgm_kernels.h
BGMF_CHUNK, BGMF_WAVES = 2 * BGM_PAIR, 8          # csrc/bgmf_kernels.h
MAX_BATCH = 4096                  # csrc/bgmb_kernels.h BGMB_MAX_BATCH


# ---------------------------------------------------------------------------------------------------------------------------
# the host plans, restated
# ---------------------------------------------------------------------------------------------------------------------------
def flip_shapes(q, units, p):
    """bgmb_fill + bnn_finish_net (csrc/bgmb_api.hip, csrc/bnn_kernels.h): (in, out) of the Flipout layers trunk ..., mean head, variance
    head; both heads read the last trunk layer."""
    dims = [q] + list(units)
    return [(dims[i], dims[i + 1]) for i in range(len(units))] + [(dims[-1], p), (dims[-1], p)]


def fill_ok(q, units, p):
    """bgmb_fill: T + 2 <= BNN_MAX_LAYERS Flipout layers, every width >= 1."""
    return p >= 1 and q >= 1 and 1 <= len(units) <= BNN_MAX_LAYERS - 2 and min(units) >= 1


def sign_words(q, units, p):
    """bnn_finish_net: sin_w[l], sout_w[l] (word offsets of a row's sign string: input bits then output bits of every layer, each rounded
    to whole words) and swords (rounded to 4)."""
    sin_w, sout_w, w = [], [], 0
    for fi, fo in flip_shapes(q, units, p):
        sin_w.append(w)
        w += (fi + 31) // 32
        sout_w.append(w)
        w += (fo + 31) // 32
    return sin_w, sout_w, (w + 3) // 4 * 4


def bgmf_plan(q, units, p, no_chains=False):
    """bgmf_session (csrc/bgmf_api.hip): None when the register-chained row tiles decline the shape, else (ktq, nh, ntx, lds_bytes,
    fits).  no_chains: BGM_BVN_NO_CHAINS is set."""
    nh = len(units)
    if not ((nh == 3 or nh == 5) and 1 <= q <= 32 and p >= 1 and not no_chains and all(u == 64 for u in units)):
        return None
    ktq, ntx = (q + 15) // 16, (p + 15) // 16
    take = lambda cnt: (cnt + 3) // 4 * 4
    resident = (2 * take(4 * 16 * ktq * 17) + take(64) + take((nh - 1) * 4 * 64 * 17) + take((nh - 1) * 64) + take(2 * 16 * ntx) +
                2 * take(16 * ktq))
    swp = ((sign_words(q, units, p)[2] + 3) // 4 * 4) | 1
    sign = resident + 2 * BGMF_CHUNK
    lds = 4 * (sign + 16 * BGMF_WAVES * swp)
    return types.SimpleNamespace(ktq=ktq, nh=nh, ntx=ntx, lds_bytes=lds, fits=lds <= LDS_LIMIT)


def gx_pad32(n):
    return (n + 31) & ~31          # csrc/gx_device.h


def gx_ld(width):
    return ((width + 59) // 64) * 64 + 8          # csrc/gx_device.h


def gx_bgm_lds_bytes(ld, q, mask_bytes):
    return 4 * (4 * GX_ROWS * ld + 5 * GX_ROWS * q + 3 * GX_ROWS + 2 * q + 128) + ((mask_bytes + 15) & ~15)          # csrc/gx_bgm_kernels.h


def gxf_plan(q, units, p):
    """gxf_session (csrc/bgmb_api.hip): None when the trunk is too deep, else (ld, ch, chunks = the head chunks' column counts, Pp,
    mask_bytes, lds_bytes, pack_floats, fits, occ = workgroups per CU of the launch in bgm_bvn_hmc_run)."""
    T = len(units)
    if T < 1 or T + 1 > GX_MAXL:
        return None
    Pp = gx_pad32(p)
    pad = [gx_pad32(q)] + [gx_pad32(u) for u in units] + [2 * Pp]
    off, wmax, mb = 0, 32, 0
    for l in range(T + 1):
        Kp, Np = pad[l], pad[l + 1]
        off += Kp * Np + Np
        wmax = max(wmax, Kp)
        if l < T:
            mb += GX_ROWS * (Np >> 1)
    ld = gx_ld(wmax)
    ch = min(Pp, (ld - 8) // 32 * 32)
    lds = gx_bgm_lds_bytes(ld, q, mb) + GX_ROWS * sign_words(q, units, p)[2] * 4
    return types.SimpleNamespace(ld=ld, ch=ch, chunks=[min(ch, Pp - c0) for c0 in range(0, Pp, ch)], Pp=Pp, mask_bytes=mb, lds_bytes=lds,
                                 pack_floats=off, fits=lds <= LDS_LIMIT and off < (1 << 30), occ=max(1, min(4, LDS_LIMIT // lds)))


def gxf_grid(n, n_cus, occ):
    """The gxf_bgm_hmc_kernel launch of bgm_bvn_hmc_run: workgroups."""
    return max(1, min((n + GX_ROWS - 1) // GX_ROWS, n_cus * occ))


def bgmf_grid(n, n_cus):
    """bgm_tile_grid (csrc/bgm_host.h) as bgmf_launch_chain calls it: workgroups of BGMF_WAVES 16-row tiles."""
    return max(1, min(((n + 15) // 16 + BGMF_WAVES - 1) // BGMF_WAVES, n_cus))


def bvn_rt(n, n_cus):
    """bvn_rt (csrc/bgmb_api.hip): rows of a workspace tile."""
    per_cu = (n + n_cus - 1) // n_cus
    return min(BGMB_RT, max(16, (per_cu + 15) // 16 * 16))


def workspace_grid(n, n_cus):
    """bgm_bvn_logpost and the workspace branch of bgm_bvn_hmc_run: (rt, row tiles, workgroups)."""
    rt = bvn_rt(n, n_cus)
    n_tiles = (n + rt - 1) // rt
    return rt, n_tiles, min(n_tiles, 8 * n_cus)


def decode_grid(n, n_draws, n_cus):
    """bgm_bvn_decode: (tiles, workgroups); a tile never spans two draws."""
    tiles = ((n + BGMB_RT - 1) // BGMB_RT) * n_draws
    return tiles, min(tiles, 4 * n_cus)


def decode_refused(n, n_draws, sign_stride, sign_off):
    """bgm_bvn_decode: the sign row ids must stay below 2^32."""
    return n_draws * sign_stride + sign_off + n >= (1 << 32)


def route(q, units, p, frozen, no_chains=False, no_tiles=False):
    """bgm_bvn_hmc_run: "chains" (bgmf_hmc_kernel) | "tiles" (gxf_bgm_hmc_kernel) | "workspace" (bgmb_hmc_kernel).  Frozen noise asks
    gxf_session first and the chains only when the tiles hold the generator; fresh noise asks the chains alone."""
    f = bgmf_plan(q, units, p, no_chains)
    chains = f is not None and f.fits
    if frozen and not no_tiles:
        g = gxf_plan(q, units, p)
        if g is not None and g.fits:
            return "chains" if chains else "tiles"
        return "workspace"
    if not frozen and chains:
        return "chains"
    return "workspace"


def first_p_declined(q, units, plan=bgmf_plan, lo=1, hi=1 << 16):
    """The smallest p in [lo, hi] at which plan(q, units, p) does not fit (its LDS need grows with p), by bisection."""
    assert plan(q, units, lo).fits and not plan(q, units, hi).fits
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(q, units, mid).fits else (lo, mid)
    return hi


def rt_rows(n_cus):
    """{rt: n}: the largest panel bvn_rt cuts into tiles of rt rows whose last tile holds one row."""
    return {rt: rt * n_cus - rt + 1 for rt in (16, 32, 48, 64)}


def rows_workspace_trips(n_cus):
    """Two full trips of the 8 n_cus workspace workgroups over 64-row tiles and a ragged third: one whole tile, then one row."""
    return 2 * 64 * 8 * n_cus + 65


def rows_tiles_trips(n_cus, occ):
    """Two full trips of the occ n_cus LDS-tile workgroups and a ragged third: one whole tile, then one row."""
    return 2 * 32 * occ * n_cus + 33


def sampled_tiles(n, rt, grid):
    """The tiles a multi-trip panel meets the oracle on: the first and last tile of every trip, and the last tile of the panel."""
    n_tiles = (n + rt - 1) // rt
    t = set()
    for lo in range(0, n_tiles, grid):
        t |= {lo, min(lo + grid, n_tiles) - 1}
    return sorted(t | {n_tiles - 1})


def tile_rows(tiles, rt, n):
    return np.concatenate([np.arange(t * rt, min(n, (t + 1) * rt)) for t in tiles])


# ---------------------------------------------------------------------------------------------------------------------------
# nets and panels
# ---------------------------------------------------------------------------------------------------------------------------
def make_net(q, units, p, seed=0):
    """A generator whose activations stay of order one at every width: posterior means of scale min(0.1, 1 / sqrt(fan-in)), posterior
    scales of half that, a variance-head bias around +0.5 (the raw head then stays well above -3: host file), BatchNorm parameters and
    moving statistics off their defaults."""
    rs = np.random.RandomState(seed)
    net = OV.init_vnet(rs, q, list(units), p)

    def layer(L, shift=0.0):
        loc, rho, bias = L
        s = min(0.1, 1.0 / np.sqrt(loc.shape[0]))
        sg = 0.5 * s * np.exp(rho + 3.0)          # rho of init_vnet is -3 + 0.1 N(0, 1): keep that spread around half the mean's scale
        return ((loc / 0.1 * s).astype(np.float32), np.log(np.expm1(sg)).astype(np.float32), (bias + shift).astype(np.float32))
    net["trunk"] = [layer(L) for L in net["trunk"]]
    net["mean"] = layer(net["mean"])
    net["var"] = layer(net["var"], 0.5)
    net["gamma"] = (1.0 + 0.2 * rs.standard_normal(q)).astype(np.float32)
    net["beta"] = (0.1 * rs.standard_normal(q)).astype(np.float32)
    net["mean_mv"] = (0.2 * rs.standard_normal(q)).astype(np.float32)
    net["var_mv"] = (0.7 + 0.5 * rs.uniform(size=q)).astype(np.float32)
    return net


ROW_MISSING, ROW_FULL = 3, 5      # rows of every panel: no observed cell (posterior = prior) | every cell observed


def make_panel(n, p, seed):
    """[n, p] float32 with about 25 % NaN cells, row ROW_MISSING all NaN and row ROW_FULL without one."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, p)).astype(np.float32)
    full = x[ROW_FULL].copy()
    x[rs.uniform(size=x.shape) < 0.25] = np.nan
    x[ROW_MISSING] = np.nan
    x[ROW_FULL] = full
    return x


def split_nan(x, dtype=np.float64):
    return np.where(np.isnan(x), 0.0, x).astype(dtype), (~np.isnan(x)).astype(dtype)


def logpost_rows(net, z, x, rows, seed, stream, row_base, dtype=np.float64):
    """OV.log_posterior_and_grad of rows `rows` of the call (z, x) in `dtype`: signs keyed row_base + row, the perturbation shared.
    -> (logp, grad, smallest raw variance head)."""
    rows = np.asarray(rows)
    nd = OV.cast_vnet(net, dtype)
    xc, mk = split_nan(x[rows], dtype)
    noise = OV.draw(nd, len(rows), seed, stream, dtype=dtype, rows=row_base + rows)
    lp, gr, s_min = _lpg(nd, np.asarray(z)[rows].astype(dtype), xc, mk, noise)
    return lp, gr, s_min


def _lpg(net, z, x, mk, noise):
    """OV.log_posterior_and_grad (restated line by line to also return the smallest raw variance head)."""
    mean, s2, c = OV.vforward(net, z, noise, training=False)
    d = x - mean
    logp = -((mk * (d ** 2 / (2 * s2) + 0.5 * np.log(s2))).sum(axis=1) + (z ** 2).sum(axis=1) / 2)
    dmu = mk * d / s2
    ds = mk * (d ** 2 / (2 * s2 * s2) - 0.5 / s2) * OV.sigmoid(c["s_raw"])
    _, dz = OV.vbackward(net, c, dmu, ds)
    return logp, dz - z, float(c["s_raw"].min())


# ---------------------------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------------------------
def chains64(net, x, rows, seed, row_base, step, n_leapfrog, n_iters, burn_in, frozen, dtype=np.float64):
    """oracle/bgm_bnn.py::hmc_sampler at a fixed step size, for rows `rows` of the panel x (NaN = missing) whose first row is the global
    row row_base: the perturbations are shared by the rows and the signs, momenta and uniforms keyed by the global row, so a subset of
    rows gives the chains those rows have in the whole panel.  Transitions 0 .. n_iters - 1 after the bootstrap evaluation (stream 0).
    -> draws [n_iters - burn_in, rows, q], state, logp, grad (after the last transition), acc [n_iters, rows] bool, margin [rows] (the
    smallest |log u - min(log ratio, 0)| of the row), flagged [rows]: at some transition that distance was below
    2 (1e-5 max(|lp|, |lp proposed|) + 1e-3) -- the rule and the constants of _gx_edges_ref.fragile_rows --, s_min: the smallest raw
    variance head met, lp_max: the largest |log posterior| met."""
    rows = np.asarray(rows)
    g = (row_base + rows).astype(np.int64)
    nd = OV.cast_vnet(net, dtype)
    q = len(net["gamma"])
    xc, mk = split_nan(x[rows], dtype)
    draw = lambda stream: OV.draw(nd, len(rows), seed, stream, dtype=dtype, rows=g)
    n0 = draw(0)
    z = R.normals(g, 0, q, R.TAG_INIT, seed).astype(dtype)
    lp, gr, s_min = _lpg(nd, z, xc, mk, n0)
    e = dtype(np.float32(step))
    flagged, margin = np.zeros(len(rows), bool), np.full(len(rows), np.inf)
    acc_hist, out, lp_max = np.zeros((n_iters, len(rows)), bool), [], np.abs(lp).max()
    for it in range(n_iters):
        mom = R.normals(g, it, q, R.TAG_MOM, seed).astype(dtype)
        u = R.uniforms(g, it, R.TAG_HACC, seed).astype(dtype)
        h0 = -lp + (mom ** 2).sum(axis=1) / 2
        zc, pc = z.copy(), mom + e / 2 * gr
        for l in range(n_leapfrog):
            zc = zc + e * pc
            lpc, grc, s = _lpg(nd, zc, xc, mk, n0 if frozen else draw(OV.hmc_stream(it, l, n_leapfrog)))
            s_min = min(s_min, s)
            pc = pc + (e if l < n_leapfrog - 1 else e / 2) * grc
        h1 = -lpc + (pc ** 2).sum(axis=1) / 2
        lr = -(h1 - h0)
        lr = np.where(np.isfinite(lr), lr, -np.inf)
        dist = np.abs(np.log(u) - np.minimum(lr, 0.0))
        flagged |= dist < 2.0 * (1e-5 * np.maximum(np.abs(lpc), np.abs(lp)) + 1e-3)
        margin = np.minimum(margin, dist)
        acc = np.log(u) < lr
        z = np.where(acc[:, None], zc, z)
        lp = np.where(acc, lpc, lp)
        gr = np.where(acc[:, None], grc, gr)
        lp_max = max(lp_max, np.abs(lpc).max())
        acc_hist[it] = acc
        if it >= burn_in:
            out.append(z.copy())
    return types.SimpleNamespace(draws=np.array(out).reshape(len(out), len(rows), q), state=z, logp=lp, grad=gr, acc=acc_hist, margin=margin,
                                 flagged=flagged, s_min=s_min, lp_max=float(lp_max))


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
A_ROWS, A_ROW_BASE, A_LEAP = 33, 7, 3
A_FIRST, A_MORE = 2, 3            # bootstrap + 2 transitions, then 3 more from the stored state with their draws kept
CAP_A, CAP_TRIPS = 0.15, 0.06     # largest flagged share of a panel (tests/_gx_edges_ref.py CAP_35, CAP_8): a condition on the inputs
H64 = lambda k: (64,) * k
P_DECLINE = first_p_declined(10, H64(5))          # the first p the chains decline at q = 10 with five hidden layers


def acase(name, q, units, p, frozen, want, step, seed=77, data_seed=22, **kw):
    """A chain case of part A: want = the route it is planned for; kw: what else the host file asserts of the plan (ktq, nh: the chains'
    instantiation; chunks, occ: the tiles' head chunks and workgroups per CU)."""
    return dict(name=name, q=q, units=tuple(units), p=p, frozen=frozen, want=want, step=step, seed=seed, data_seed=data_seed, n=A_ROWS,
                row_base=A_ROW_BASE, leap=A_LEAP, n_first=A_FIRST, n_more=A_MORE, net_seed=21, **kw)


# step: chosen per case in the float64 oracle alone so that every case both accepts and rejects proposals and at most CAP_A of the rows
# are flagged (test_bvn_edges_host.py asserts both)
A_CASES = []
for _fz in (True, False):          # one case per fp32 instantiation of bgmf_hmc_kernel<KTQ, NH, FRESH>
    _t = "frozen" if _fz else "fresh"
    A_CASES += [acase("chains-q16-nh3-p16-" + _t, 16, H64(3), 16, _fz, "chains", 0.7, ktq=1, nh=3),
                acase("chains-q17-nh3-p17-" + _t, 17, H64(3), 17, _fz, "chains", 0.7 if _fz else 0.45, ktq=2, nh=3),
                acase("chains-q1-nh5-p1-" + _t, 1, H64(5), 1, _fz, "chains", 0.7 if _fz else 0.45, ktq=1, nh=5),
                acase("chains-q32-nh5-p15-" + _t, 32, H64(5), 15, _fz, "chains", 0.7, ktq=2, nh=5)]
A_CASES += [          # one predicate of bgmf_session off the chains each: frozen noise lands on the tiles
    acase("off-q33", 33, H64(3), 20, True, "tiles", 0.7, off="q"),
    acase("off-nh4", 10, H64(4), 20, True, "tiles", 0.7, off="depth"),
    acase("off-w63", 10, (64, 64, 63, 64, 64), 20, True, "tiles", 0.45, off="width"),
    acase("off-w65", 10, (64, 65, 64), 20, True, "tiles", 0.45, off="width"),
    acase("lds-last-p%d" % (P_DECLINE - 1), 10, H64(5), P_DECLINE - 1, True, "chains", 0.45, ktq=1, nh=5),
    acase("lds-first-p%d" % P_DECLINE, 10, H64(5), P_DECLINE, True, "tiles", 0.3, off="lds"),
    # the tiles alone
    acase("tiles-24-40-p100", 5, (24, 40), 100, True, "tiles", 1.0, occ=3, n_chunks=2),
    acase("tiles-130-p300", 5, (130,), 300, True, "tiles", 0.3, occ=1, chunks=[192, 128], ld=200),
    acase("tiles-16-T1", 3, (16,), 9, True, "tiles", 0.3, occ=3, n_chunks=1),
    acase("tiles-32x6", 4, (32,) * 6, 12, True, "tiles", 0.7, n_chunks=1),
    acase("tiles-256x3-p100", 10, (256,) * 3, 100, True, "tiles", 0.12, occ=1, n_chunks=1),
    # off the tiles: the workspace kernel with frozen noise
    acase("ws-257-frozen", 5, (257,), 20, True, "workspace", 1.0),
    acase("ws-256x5-frozen", 10, (256,) * 5, 8, True, "workspace", 1.0),
    acase("ws-512-frozen", 5, (512,), 20, True, "workspace", 1.0),
    # the workspace kernel with fresh noise on widths that are no multiple of 64
    acase("ws-24-40-p37-fresh", 5, (24, 40), 37, False, "workspace", 0.3),
    acase("ws-257-fresh", 5, (257,), 20, False, "workspace", 0.3),
]
A_BY_NAME = {c["name"]: c for c in A_CASES}
assert len(A_BY_NAME) == len(A_CASES)

# parts B and C share one small net (its workspace slice is 0.17 MB: 8 n_cus slices stay far below 1 GiB)
SMALL = dict(q=5, units=(24, 40), p=37, net_seed=21)
B_SEED, B_STREAM, B_ROW_BASE, B_STEP, B_LEAP, B_ITERS = (5 << 32) | 1234567, 9, 11, 0.7, 3, 2
D_ROWS, D_SEED, D_BLOCK, D_BURN, D_ROW_BASE = 130, 77, 2, 11, 300
C_BATCHES = (2, 65, 4096)


def decode_draws(n_cus):
    """Draws of the decode panel: 3 tiles (64, 64, 2 rows) per draw, more than two trips of the 4 n_cus workgroups."""
    return (2 * 4 * n_cus) // 3 + 1


def case_net(c):
    return _net(c["q"], tuple(c["units"]), c["p"], c["net_seed"])


@functools.lru_cache(maxsize=None)
def _net(q, units, p, seed):
    net = make_net(q, units, p, seed)
    for a in [net[k] for k in ("gamma", "beta", "mean_mv", "var_mv")] + [a for L in OV.layers_of(net) for a in L]:
        a.setflags(write=False)
    return net


@functools.lru_cache(maxsize=None)
def panel(n, p, seed):
    x = make_panel(n, p, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref_chain(name):
    """chains64 of a part A case over all its transitions (the first n_first belong to the burn-in); shared, computed once."""
    c = A_BY_NAME[name]
    r = chains64(case_net(c), panel(c["n"], c["p"], c["data_seed"]), np.arange(c["n"]), c["seed"], c["row_base"], c["step"], c["leap"],
                 c["n_first"] + c["n_more"], c["n_first"], c["frozen"])
    for a in (r.draws, r.state, r.logp, r.grad, r.acc, r.flagged):
        a.setflags(write=False)
    return r


def sign_layout_oracle(q, units, p):
    return OB.sign_layout(flip_shapes(q, units, p))
