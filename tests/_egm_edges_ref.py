"""The host plan of the deterministic CausalBGM EGM warm start restated in plain Python, the case table of
tests/test_gpu_egm_edges.py, and the builders of the cases' inputs (TEST INFRASTRUCTURE; tests/test_egm_edges_host.py shows on the CPU
what every case reaches and keeps the restatement in step with the C++ text).

plan() restates egm_plan (csrc/egm_plan.h: chain_extent, chain_disc_ok, chain_trunk_ok, chain_head_ok, egm_arena), which
bgm_causal_egm_begin (csrc/egm_api.hip) evaluates once for the kernels of bgm_causal_egm_disc_step / _gen_step, together with the
LDS sizes of the register-chained kernels (ech_layout / ech_disc_lds_floats in csrc/egm_chain.h, ecg_lds_floats in csrc/egm_chain_gen.h).

Routes of the discriminator step           Routes of the generator step
  chain-t2         two latent tiles (q 17..32), B = 32        chain-t2       two latent tiles, masked 13-tile output of g
  chain-32-k13     B = 32, (p + 15) / 16 == 13                chain-pad      B = 32, p + 1 narrower than a compiled extent: 13 tiles, masked
  chain-32-k7      B = 32, (p + 15) / 16 == 7                 chain-32-n13   B = 32, (p + 16) / 16 == 13
  chain-32-stream  B = 32, any other p                        chain-32-n7    B = 32, (p + 16) / 16 == 7
  chain-16         B = 16                                     chain-16-n13   B = 16, 13 tiles
  lds              workgroup kernel, arena in LDS             chain-16-n7    B = 16, 7 tiles
  global           workgroup kernel, arena in the workspace   step           workgroup kernel

Fixed normalisation: the engine carries no moving statistics of its own; bgm_set_disc_norm(fixed) is BatchNormalization in inference
mode on its INITIAL moving averages (mean 0, variance 1), i.e. the constant scale 1 / sqrt(1 + 1e-3) per column (oracle/egm.py::_fixed).
The builders therefore have nothing to randomise there; gamma (1 +- 0.2) and beta (+- 0.1) and every bias are non-trivial, so a kernel
that drops a masked gamma, beta or bias column shows."""
import collections
import functools

import numpy as np

from oracle import egm as OE
from oracle import nets as N

# ---------------------------------------------------------------------------------------------------------------------------
# constants of the C++ text (tests/test_egm_edges_host.py parses them out of the sources and fails when they move)
# ---------------------------------------------------------------------------------------------------------------------------
LDS_LIMIT = 160 * 1024
B_MIN, B_MAX = 2, 4096
EGM_THREADS = 512
EGM_MAX_LAYERS = 8                 # layers of one network, the output layer included: at most 7 hidden layers
ECH_ROLE_WAVES = 6
CHAIN_T = (4, 2, 1)                # tiles of the three hidden layers of a chained discriminator: d1 49..64, d2 17..32, d3 1..16
CHAIN_BATCHES = (16, 32)
GEN_EXTENTS = (13, 7)              # compiled output-tile counts of g in the generator chains
DISC_EXTENTS = (13, 7)             # compiled first-layer tile counts of e in the B = 32 discriminator chain
HEAD_FIXED = (64, 32)              # first two hidden widths of f and h on the chains; the third 1..16, the input <= 16

DISC_ROUTES = ("chain-t2", "chain-32-k13", "chain-32-k7", "chain-32-stream", "chain-16", "lds", "global")
GEN_ROUTES = ("chain-t2", "chain-pad", "chain-32-n13", "chain-32-n7", "chain-16-n13", "chain-16-n7", "step")

Plan = collections.namedtuple("Plan", "arena_bytes disc_lds t0 disc gen chain_disc_bytes chain_gen_bytes")


def _tiles(n):
    return (n + 15) // 16


def _up4(n):
    return (n + 3) // 4 * 4


def ech_layout_floats(t0):
    """ech_layout<4, 2, 1, t0>(d).total: the zero-padded LDS parameter block of a chained discriminator."""
    T1, T2, T3 = CHAIN_T
    ld = (16 * T1 + 4, 16 * T2 + 4, 16 * T3 + 4)
    lt = (16 * t0 + 4, 16 * T1 + 4, 16 * T2 + 4)
    parts = [16 * t0 * ld[0], 16 * T1 * ld[1], 16 * T2 * ld[2], 16 * T1 * lt[0], 16 * T2 * lt[1], 16 * T3 * lt[2]]
    parts += [16 * T1, 16 * T2, 16 * T3] * 3 + [16 * T3, 1]
    return sum(_up4(n) for n in parts)


def ech_disc_lds_floats(B, t0):
    T1, T2, T3 = CHAIN_T
    xw, dw = 16 * (t0 + T1 + T2), 16 * (T1 + T2 + T3)
    sl = 16 * (T1 + T2 + T3)
    slot = 2 * sl + 16 * T3 + 16
    return 64 + ech_layout_floats(t0) + ECH_ROLE_WAVES * slot + 16 * t0 * B + (3 if t0 > 1 else 4) * B * (xw + dw)


def ecg_lds_floats(B, t0):
    return 64 + ech_layout_floats(t0) + 8 * 16 + 16 + 3 * 16 * t0 * B


def arena_floats(q, B, dz_units):
    """The working set of egm_disc_step_kernel: cache A | max(cache B + da + du, gradient-penalty scratch)."""
    dims = [q] + list(dz_units)
    dmax, dall, dsum = max(dims), sum(dims), sum(dz_units)
    cache = ((2 * B + 1) * dsum + B + 3) // 4 * 4
    gp = (B * dall + (5 * B + 1) * dsum + 3) // 4 * 4 + 3 * B * dmax
    return cache + max(cache + 2 * B * dmax, gp)


def plan(p, z_dims, B, dz_units, g_units, e_units, f_units, h_units, fixed_norm, no_chain=False, no_chain_gen=False):
    """egm_plan for a session bgm_causal_egm_begin accepts -> Plan(arena bytes incl. the 64 reduction words, disc_lds, t0, routes, chain LDS)."""
    q = sum(z_dims)
    assert B_MIN <= B <= B_MAX and 1 <= len(dz_units) <= EGM_MAX_LAYERS - 1
    for units in (g_units, e_units, f_units, h_units):
        assert 1 <= len(units) <= EGM_MAX_LAYERS - 1
    arena_bytes = 4 * (64 + arena_floats(q, B, dz_units))
    disc_lds = int(arena_bytes <= LDS_LIMIT)
    t0 = 1 if q <= 16 else 2
    T1, T2, T3 = CHAIN_T
    dz = list(dz_units)
    chain = (bool(fixed_norm) and len(dz) == 3 and q <= 32 and (t0 == 1 or B == 32) and _tiles(dz[0]) == T1 and _tiles(dz[1]) == T2
             and 1 <= dz[2] <= 16 * T3 and B in CHAIN_BATCHES and all(w == 64 for w in e_units))
    chain_disc_bytes = 4 * ech_disc_lds_floats(B, t0) if chain else 0
    if no_chain or chain_disc_bytes > LDS_LIMIT:
        chain_disc_bytes = 0
    # generator step
    ntl_need = _tiles(p + 1)
    ntl = ntl_need if (ntl_need in GEN_EXTENTS and t0 == 1) else 13
    gchain = chain_disc_bytes > 0 and ntl_need <= 13 and (ntl == ntl_need or B == 32) and all(w == 64 for w in g_units)
    for units, n_in in ((f_units, z_dims[0] + z_dims[1] + 1), (h_units, z_dims[0] + z_dims[2])):
        gchain = gchain and len(units) == 3 and n_in <= 16 and tuple(units[:2]) == HEAD_FIXED and 1 <= units[2] <= 16
    if no_chain_gen:
        gchain = False
    chain_gen_bytes = 4 * ecg_lds_floats(B, t0) if gchain else 0
    pad = ntl != ntl_need or t0 == 2
    # routes
    if chain_disc_bytes:
        kt0 = _tiles(p)
        disc = ("chain-t2" if t0 == 2 else "chain-16" if B == 16 else
                "chain-32-k%d" % kt0 if kt0 in DISC_EXTENTS else "chain-32-stream")
    else:
        disc = "lds" if disc_lds else "global"
    if gchain:
        gen = "chain-t2" if t0 == 2 else "chain-pad" if pad else "chain-%d-n%d" % (B, ntl)
    else:
        gen = "step"
    return Plan(arena_bytes, disc_lds, t0, disc, gen, chain_disc_bytes, chain_gen_bytes)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
N_ROWS = 200
LR = 2e-4
EPS_GRAD = 0.37
ROUNDS = 3
D_DEF, G_DEF, FH_DEF = (64, 32, 8), (64,) * 5, (64, 32, 8)
Z10, Z18, Z24 = (1, 1, 1, 7), (3, 3, 6, 6), (7, 8, 8, 1)


def _case(name, edge, want_disc, want_gen, p=23, z_dims=Z10, B=32, binary=False, fixed=True, dz=D_DEF, g=G_DEF, e=G_DEF, f=FH_DEF, h=FH_DEF,
          use_z_rec=True, ends=False, masked=False, split=False, seed=0):
    return dict(name=name, edge=edge, want_disc=want_disc, want_gen=want_gen, p=p, z_dims=tuple(z_dims), B=B, binary=binary, fixed=fixed,
                dz_units=tuple(dz), g_units=tuple(g), e_units=tuple(e), f_units=tuple(f), h_units=tuple(h), use_z_rec=use_z_rec, ends=ends,
                masked=masked, split=split, seed=seed, n=N_ROWS)


CASES = [
    # ---- where the workgroup kernels keep the discriminator's working set
    _case("ws-b39-lds", "the last batch whose arena fits LDS (162 560 B)", "lds", "step", B=39, fixed=False),
    _case("ws-b40-global", "the first batch whose arena leaves LDS (166 688 B); idx holds rows 0 and n - 1", "global", "step", B=40, fixed=False, ends=True),
    _case("ws-b40-fixed-binary", "the arena in the workspace with fixed statistics and a binary treatment", "global", "step", B=40, binary=True),
    _case("ws-b65", "a batch of four 16-row tiles and one row", "global", "step", B=65, fixed=False),
    _case("ws-b513-p20", "EGM_THREADS + 1 rows: every b += EGM_THREADS loop takes a second pass (rows drawn with replacement from n = 200)",
          "global", "step", p=20, B=EGM_THREADS + 1, fixed=False),
    _case("ws-b2", "the ABI minimum; fixed statistics (batch statistics of two rows cost the float32 ORACLE 8.5e-6 on the trained parameters, more\n"
          "than a quarter of the bar: no fair case)", "lds", "step", B=2),
    _case("ws-b3", "one above the minimum, an odd batch; fixed statistics (batch statistics of three rows cost the float32 ORACLE 9.6e-5 of the\n"
          "largest generator gradient, twice the bar: no fair case)", "lds", "step", B=3),
    _case("ws-dz256-b16", "a wide discriminator: the arena leaves LDS at a small batch", "global", "step", B=16, fixed=False, dz=(256, 64, 8)),
    # ---- masked widths of the chained discriminator (ech_ld, min(o, n_out - 1), o < n_out, the padded parameter block)
    _case("dz-49-17-1-b32", "the narrowest widths of every tile count, d3 = 1", "chain-32-stream", "chain-pad", dz=(49, 17, 1), masked=True),
    _case("dz-63-31-16-b32", "one short of whole tiles, d3 a whole tile", "chain-32-stream", "chain-pad", dz=(63, 31, 16), masked=True),
    _case("dz-64-32-16-b32", "whole tiles with d3 = 16", "chain-32-stream", "chain-pad", dz=(64, 32, 16)),
    _case("dz-50-20-3-b32", "widths that are no multiple of 4", "chain-32-stream", "chain-pad", dz=(50, 20, 3), masked=True),
    _case("dz-49-17-1-b16", "... one 16-row tile; the generator step has no padded variant at B = 16", "chain-16", "step", p=37, B=16, dz=(49, 17, 1), masked=True),
    _case("dz-63-31-16-b16", "... one 16-row tile", "chain-16", "step", p=37, B=16, dz=(63, 31, 16), masked=True),
    _case("dz-64-32-16-b16", "... one 16-row tile", "chain-16", "step", p=37, B=16, dz=(64, 32, 16)),
    _case("dz-50-20-3-b16", "... one 16-row tile", "chain-16", "step", p=37, B=16, dz=(50, 20, 3), masked=True),
    _case("dz-48-32-8-off", "d1 = 48 is three tiles: off the chains", "lds", "step", dz=(48, 32, 8)),
    _case("dz-64-33-8-off", "d2 = 33 is three tiles: off the chains", "lds", "step", dz=(64, 33, 8)),
    _case("dz-49-17-1-t2", "masked widths with two latent tiles (q = 18)", "chain-t2", "chain-t2", p=177, z_dims=Z18, binary=True, dz=(49, 17, 1), masked=True),
    _case("dz-63-31-16-t2", "... two latent tiles", "chain-t2", "chain-t2", p=60, z_dims=Z18, dz=(63, 31, 16), masked=True),
    _case("dz-64-32-16-t2", "... two latent tiles", "chain-t2", "chain-t2", p=60, z_dims=Z18, dz=(64, 32, 16)),
    _case("dz-50-20-3-t2", "... two latent tiles", "chain-t2", "chain-t2", p=177, z_dims=Z18, dz=(50, 20, 3), masked=True),
    # ---- heads and depth on the generator chains
    _case("fh-64-32-1", "third hidden width of f and h = 1", "chain-32-k7", "chain-32-n7", p=100, f=(64, 32, 1), h=(64, 32, 1), masked=True),
    _case("fh-64-32-16", "third hidden width = 16", "chain-32-k13", "chain-32-n13", p=200, f=(64, 32, 16), h=(64, 32, 16)),
    _case("fh-64-32-5", "third hidden width = 5, padded g", "chain-32-stream", "chain-pad", p=50, f=(64, 32, 5), h=(64, 32, 5), masked=True),
    _case("heads-in-16-15", "head inputs of 16 and 15 columns, q = 24", "chain-t2", "chain-t2", p=60, z_dims=Z24, masked=True),
    _case("heads-in-16-15-fh5", "... with a third hidden width of 5", "chain-t2", "chain-t2", p=60, z_dims=Z24, f=(64, 32, 5), h=(64, 32, 5), masked=True),
    _case("depth-1", "g and e with one hidden layer", "chain-32-k13", "chain-32-n13", p=200, g=(64,), e=(64,)),
    _case("depth-2-7", "g with two and e with seven hidden layers (EGM_MAX_LAYERS allows no more)", "chain-32-k7", "chain-32-n7", p=100, g=(64,) * 2, e=(64,) * 7),
    _case("fh-64-32-17-off", "third hidden width = 17: the generator step leaves the chains, the discriminator step stays", "chain-32-k7", "step",
          p=100, f=(64, 32, 17), h=(64, 32, 17)),
    # ---- compiled variants nobody compared with the oracle
    _case("b16-p100", "egm_gen_chain_kernel<4, 7, 4, 2, 1, 1>; idx holds rows 0 and n - 1", "chain-16", "chain-16-n7", p=100, B=16, ends=True, split=True),
    _case("b16-p200", "egm_gen_chain_kernel<4, 13, 4, 2, 1, 1>", "chain-16", "chain-16-n13", p=200, B=16, split=True),
    _case("b16-p100-binary", "... binary treatment", "chain-16", "chain-16-n7", p=100, B=16, binary=True),
    _case("b16-p200-binary", "... binary treatment", "chain-16", "chain-16-n13", p=200, B=16, binary=True),
    # ---- the edges of the compiled extents: the discriminator step keys on (p + 15) / 16, the generator step on (p + 16) / 16
    _case("p95", "six tiles for both", "chain-32-stream", "chain-pad", p=95),
    _case("p96", "g's output p + 1 = 97 opens the seventh tile, e's input does not", "chain-32-stream", "chain-32-n7", p=96),
    _case("p111", "seven tiles for both, the last one short", "chain-32-k7", "chain-32-n7", p=111, masked=True),
    _case("p112", "e's input fills seven tiles, g's output needs eight", "chain-32-k7", "chain-pad", p=112),
    _case("p191", "twelve tiles for both", "chain-32-stream", "chain-pad", p=191),
    _case("p192", "g's output opens the thirteenth tile", "chain-32-stream", "chain-32-n13", p=192),
    _case("p207", "thirteen tiles for both", "chain-32-k13", "chain-32-n13", p=207, masked=True),
    _case("p208", "a full thirteenth tile of e's input; g's output needs fourteen: off the generator chains", "chain-32-k13", "step", p=208),
    # ---- use_z_rec = 0
    _case("zrec0-n13", "no z reconstruction term on a compiled extent", "chain-32-k13", "chain-32-n13", p=200, use_z_rec=False),
    _case("zrec0-pad", "... on the padded variant", "chain-32-stream", "chain-pad", p=50, use_z_rec=False),
    _case("zrec0-step", "... in the workgroup kernel", "lds", "step", fixed=False, use_z_rec=False),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# p -> (discriminator route, generator route) at B = 32, fixed normalisation, q = 10, default widths: the claim test_egm_edges_host.py sweeps
EXTENT_PAIRS = {95: ("chain-32-stream", "chain-pad"), 96: ("chain-32-stream", "chain-32-n7"), 111: ("chain-32-k7", "chain-32-n7"),
                112: ("chain-32-k7", "chain-pad"), 191: ("chain-32-stream", "chain-pad"), 192: ("chain-32-stream", "chain-32-n13"),
                207: ("chain-32-k13", "chain-32-n13"), 208: ("chain-32-k13", "step")}


def case_plan(c, **switches):
    return plan(c["p"], c["z_dims"], c["B"], c["dz_units"], c["g_units"], c["e_units"], c["f_units"], c["h_units"], c["fixed"], **switches)


def is_chain(c):
    return c["want_disc"].startswith("chain") or c["want_gen"].startswith("chain")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and float64 references (computed once per case and never modified by their readers)
# ---------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "nets dz params v x y grad_batch rounds")


def _batch(rs, c, with_eps):
    n, B, q = c["n"], c["B"], sum(c["z_dims"])
    z = rs.randn(B, q).astype(np.float32)
    if B > n:
        idx = rs.randint(0, n, B)
    elif c["ends"]:          # the gather reads the first and the last row of the panel, neither at the edge of the batch
        idx = 1 + rs.choice(n - 2, B, replace=False)
        idx[B // 2], idx[B - 2] = 0, n - 1
    else:
        idx = rs.choice(n, B, replace=False)
    return z, idx.astype(np.int32), (float(rs.rand()) if with_eps else None)


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = BY_NAME[name]
    rs = np.random.RandomState(1000 + c["seed"])
    p, zd = c["p"], c["z_dims"]
    q = sum(zd)
    nets = {"g": N.init_mlp(rs, [q] + list(c["g_units"]) + [p + 1]), "e": N.init_mlp(rs, [p] + list(c["e_units"]) + [q]),
            "f": N.init_mlp(rs, [zd[0] + zd[1] + 1] + list(c["f_units"]) + [2]), "h": N.init_mlp(rs, [zd[0] + zd[2]] + list(c["h_units"]) + [2])}
    for k in nets:
        nets[k] = [(W, (0.1 * rs.randn(*b.shape)).astype(np.float32)) for W, b in nets[k]]
    dz = OE.init_disc(rs, q, list(c["dz_units"]))
    dz["b"] = [(0.1 * rs.randn(*b.shape)).astype(np.float32) for b in dz["b"]]
    dz["gamma"] = [(1 + 0.2 * rs.randn(*b.shape)).astype(np.float32) for b in dz["gamma"]]
    dz["beta"] = [(0.1 * rs.randn(*b.shape)).astype(np.float32) for b in dz["beta"]]
    if c["fixed"]:
        dz["fixed_norm"] = True
    n = c["n"]
    v = rs.randn(n, p).astype(np.float32)
    x = (rs.rand(n) > 0.5).astype(np.float32) if c["binary"] else rs.rand(n).astype(np.float32)
    y = rs.randn(n).astype(np.float32)
    params = dict(v_dim=p, z_dims=list(zd), binary_treatment=c["binary"], use_z_rec=c["use_z_rec"], lr=LR)
    grad_batch = _batch(rs, c, False)
    rounds = [(_batch(rs, c, True), _batch(rs, c, True), _batch(rs, c, False)) for _ in range(ROUNDS)]
    return Inputs(nets, dz, params, v, x, y, grad_batch, rounds)


def flat_gen(nets):
    return np.concatenate([a.ravel() for a in OE.gen_param_list(nets)])


def flat_disc(dz):
    return np.concatenate([a.ravel() for a in OE.disc_param_list(dz)])


GradRef = collections.namedtuple("GradRef", "d_losses d_grads g_losses g_grads d_tree g_tree")


def step_grads(name, dtype=np.float64):
    """One discriminator and one generator step of the oracle on the case's gradient batch, in `dtype`."""
    c, I = BY_NAME[name], inputs(name)
    nets = {k: N.cast_net(I.nets[k], dtype) for k in I.nets}
    dz = OE.cast_disc(I.dz, dtype)
    z, idx, _ = I.grad_batch
    zb, vb = z.astype(dtype), I.v[idx].astype(dtype)
    l1, l2, gd = OE.disc_step_grads(nets, dz, zb, vb, dtype(EPS_GRAD))
    lg, gg = OE.gen_step_grads(nets, dz, I.params, zb, vb, I.x[idx].astype(dtype).reshape(-1, 1), I.y[idx].astype(dtype).reshape(-1, 1))
    return GradRef(np.array([l1, l2]), flat_disc(gd), np.asarray(lg), flat_gen(gg), gd, gg)


@functools.lru_cache(maxsize=None)
def grads64(name):
    return step_grads(name, np.float64)


TrainRef = collections.namedtuple("TrainRef", "theta_g theta_d g_first")


def trained(name, dtype=np.float64):
    """ROUNDS alternating rounds (two discriminator steps, one generator step) of oracle.egm.EgmState in `dtype`."""
    I = inputs(name)
    st = OE.EgmState({k: N.cast_net(I.nets[k], dtype) for k in I.nets}, OE.cast_disc(I.dz, dtype), I.params)
    f = lambda a: a.astype(dtype)
    for d1, d2, g in I.rounds:
        for z, idx, eps in (d1, d2):
            st.disc_step(f(z), f(I.v[idx]), dtype(eps))
        z, idx, _ = g
        st.gen_step(f(z), f(I.v[idx]), f(I.x[idx]).reshape(-1, 1), f(I.y[idx]).reshape(-1, 1))
    return TrainRef(flat_gen(st.nets), flat_disc(st.dz), st.nets["g"][0][0].copy())


@functools.lru_cache(maxsize=None)
def trained64(name):
    return trained(name, np.float64)


def inert_disc_mask(name):
    """Hidden-layer biases of a batch-normalised discriminator: zero exact gradient, rounding noise amplified by Adam (tests/test_gpu_egm.py)."""
    c, I = BY_NAME[name], inputs(name)
    m = np.zeros(flat_disc(I.dz).size, bool)
    if not c["fixed"]:
        n_w = sum(a.size for a in I.dz["W"])
        m[n_w:n_w + sum(a.size for a in I.dz["b"][:-1])] = True
    return m


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-30))
