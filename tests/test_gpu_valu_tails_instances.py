"""The vector-ALU tails of the keep kernel's dose passes (csrc/causal_kernels.h causal_dose_passes_valu) at every compiled shape and
route.  tests/test_gpu_effect_valu_tails.py runs z_dims [1, 1, 1, 7] at p = 20 and p = 50; which template instance gets the new path
is decided per instance (causal_valu_tails, and a second time for the event form in bgm_causal_event_finish), so this module runs
every instance of the table below and asserts the table itself.

TABLE is a literal, written from DESIGN.md ("The tails of the dose passes on the vector ALU": its table and resource bullet), not
computed from the C++ rule.  How it is asserted: the dose passes do not feed back into the chains, so state, cached log posterior,
acceptance counts and draws are np.array_equal between the default engine and the BGM_MH_MFMA_TAILS=1 engine in every cell; where
the table says 'mfma' both engines ran the same instance and the ADRF is np.array_equal too; where it says 'valu' the two summation
orders must show in at least one of the 20 x 7 ADRF values (otherwise the switch or the rule did nothing).

The panels are the smallest that reach each shape (KT1, KSL1, NTL): q + 1 <= 12 gives KT1 = 1, 13 .. 20 gives KT1 = 2; p + 1 outputs
in 16-wide tiles, rounded up to 2, 7 or 13 / 10 tiles.  The shapes with NTL > 2 run the Gram form of g's likelihood by default and
the direct form under BGM_MH_DIRECT_LIKELIHOOD=1; the NTL the panel reached is checked through mh_info (the two forms differ by
16 NTL - 64 matrix instructions per transition).

Doses are rounded to fp32 before they go to the engine and to the float64 oracle, so the oracle sees the engine's inputs exactly.

Per-row accuracy (test_per_row_accuracy): at n = 1 an ADRF entry is one chain's value, nothing is averaged.  Measured on an MI355X
over the n = 1 cases (20 doses x 7 draws, sample_y on and off, shapes (1,3,13) Gram and (2,1,2)):
    worst |ADRF - oracle64|, matrix-pipe tails (the arithmetic before the vector-ALU tails):  5.70e-7
    worst |ADRF - oracle64|, vector-ALU tails:                                               4.43e-7
PER_ROW_BOUND = 8 x the matrix-pipe figure = 4.56e-6 (cap 2e-4): the two summation orders legitimately differ by a few ulp of a sum
of O(1) terms, and a maximum over a few hundred values fluctuates.  (Two outputs of layer 3 swapped in the vector-ALU weights, tried
once on a scratch build: 1e-2 .. 1.4e-1 in every oracle check of this module.)

test_second_tile_of_a_slot leaves nothing out: the float64 oracle on its 32 792-row panel is 35 small forward passes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import causal as OC            # noqa: E402
from oracle import identifiable as OI      # noqa: E402
from tests.test_gpu_causal import _model, _data, _engine  # noqa: E402
from tests.test_gpu_effect_valu_tails import BURN, KEEP, CHUNK, SEED, Q_SD, TOL, _check, _sample  # noqa: E402

MFMA, DIRECT = "BGM_MH_MFMA_TAILS", "BGM_MH_DIRECT_LIKELIHOOD"
PER_ROW_BOUND = min(8 * 5.70e-7, 2e-4)      # 4.56e-6: 8 x the matrix-pipe engine's worst per-row error (module docstring)
CHAIN = ("state", "logp", "acc_count", "draws")

# name -> (z_dims, p, NTL).  q + 1 = 11, 19, 13, 20; p + 1 = 21 (2 tiles), 51 (4 -> 7), 121 (8 -> 13 / 10)
SHAPES = {"1-3-2": ([1, 1, 1, 7], 20, 2), "1-3-7": ([1, 1, 1, 7], 50, 7), "1-3-13": ([1, 1, 1, 7], 120, 13),
          "2-1-2": ([3, 3, 6, 6], 20, 2), "2-1-2-q19": ([3, 3, 6, 7], 20, 2),      # q + 1 = 20: the widest first layer
          "2-1-7": ([3, 3, 6, 6], 50, 7), "2-1-10": ([2, 2, 2, 6], 120, 10)}       # q + 1 = 13: the treatment alone in the second K tile

# (shape, form of g's likelihood, tails with the fixed scale, tails with the per-chain scale).  form: 'default' = no environment
# (direct at NTL = 2, Gram above), 'direct' = BGM_MH_DIRECT_LIKELIHOOD=1 (at NTL = 2 the same instance as 'default')
TABLE = [("1-3-2", "default", "valu", "valu"),
         ("1-3-2", "direct", "valu", "valu"),
         ("1-3-7", "default", "valu", "valu"),
         ("1-3-7", "direct", "mfma", "mfma"),
         ("1-3-13", "default", "valu", "valu"),
         ("1-3-13", "direct", "valu", "valu"),
         ("2-1-2", "default", "valu", "mfma"),
         ("2-1-2", "direct", "valu", "mfma"),
         ("2-1-2-q19", "default", "valu", "mfma"),
         ("2-1-2-q19", "direct", "valu", "mfma"),
         ("2-1-7", "default", "mfma", "mfma"),
         ("2-1-7", "direct", "mfma", "mfma"),
         ("2-1-10", "default", "mfma", "mfma"),
         ("2-1-10", "direct", "valu", "valu")]
CELLS = [(s, f, sc, t) for s, f, fixed, row in TABLE for sc, t in (("fixed", fixed), ("row", row))]
# the distinct template instances with the vector-ALU tails (at NTL = 2 'direct' is 'default' again)
VALU = [(s, f, sc) for s, f, sc, t in CELLS if t == "valu" and not (SHAPES[s][2] == 2 and f == "direct")]
_ids = lambda cases: ["-".join(str(c) for c in case) for case in cases]      # noqa: E731

_models, _engines = {}, {}


def _doses(k):
    return np.linspace(0.0, 3.0, k).astype(np.float32).astype(np.float64)


def _mod(shape, **kw):
    key = (shape,) + tuple(sorted(kw.items()))
    if key not in _models:
        z_dims, p, _ = SHAPES[shape]
        _models[key] = _model(131 + p + sum(z_dims), z_dims, p, **kw)
    return _models[key]


def _build(m, **env):
    """an engine created with `env` in the environment, which is read at handle creation only and restored here"""
    for k in env:
        assert k not in os.environ, k
    os.environ.update(env)
    try:
        return _engine(m)
    finally:
        for k in env:
            del os.environ[k]


def _eng(shape, form="default", tails=None, **kw):
    """cached engine; tails: None = the default, '1' / '0' = BGM_MH_MFMA_TAILS"""
    key = (shape, form, tails) + tuple(sorted(kw.items()))
    if key not in _engines:
        env = {DIRECT: "1"} if form == "direct" else {}
        if tails is not None:
            env[MFMA] = tails
        _engines[key] = _build(_mod(shape, **kw), **env)
    return _engines[key]


def _scale_kw(scale):
    return dict(row_adapt=0.25) if scale == "row" else {}


def _keys(scale):
    return CHAIN + (("row_scale",) if scale == "row" else ())


def _assert_same(a, b, keys):
    for k in keys:
        ka, kb = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert np.isfinite(ka).all(), k
        assert np.array_equal(ka, kb), k


@pytest.mark.parametrize("shape,form,scale,tails", CELLS, ids=_ids(CELLS))
def test_instance_table(shape, form, scale, tails):
    """every cell of the table: which engine pair shares an instance, which does not"""
    z_dims, p, ntl = SHAPES[shape]
    new, old = _eng(shape, form), _eng(shape, form, "1")
    n = 40
    if form == "direct" and ntl > 2:     # the panel reached the shape it is listed under
        assert new.mh_info(n).mfma_per_transition_per_wave - _eng(shape).mh_info(n).mfma_per_transition_per_wave == 16 * ntl - 64
    x, y, v = _data(n, p, 140)
    xs = _doses(20)
    out_n = _sample(new, x, y, v, xs, True, False, **_scale_kw(scale))
    out_o = _sample(old, x, y, v, xs, True, False, **_scale_kw(scale))
    _assert_same(out_n, out_o, _keys(scale))
    assert out_n["acc_count"].sum().item() > 0
    a_n, a_o = out_n["adrf"].cpu().numpy(), out_o["adrf"].cpu().numpy()
    assert a_n.shape == (20, KEEP) and np.isfinite(a_n).all()
    diff = np.abs(a_n - a_o).max()
    print("%s %s %s: expected %s, worst ADRF difference between the engines %.3e" % (shape, form, scale, tails, diff))
    if tails == "mfma":
        assert np.array_equal(a_n, a_o), diff
    else:
        assert not np.array_equal(a_n, a_o)
        assert diff <= 2 * TOL, diff      # each within TOL of the oracle (test_oracle_and_wave_cache_at_every_valu_instance)
    if scale == "fixed":                 # BGM_MH_MFMA_TAILS=0 is the default engine
        zero = _sample(_eng(shape, form, "0"), x, y, v, xs, True, False)
        _assert_same(zero, out_n, CHAIN + ("adrf",))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_conditional_prior_keeps_the_matrix_pipe(shape):
    """test_valu_tails_with_the_conditional_prior at every shape, with the ADRF equal to the last bit: every conditional-prior instance
    keeps the matrix-pipe tails, so the two engines run the same kernel"""
    import torch
    z_dims, p, _ = SHAPES[shape]
    m, n = _mod(shape), 40
    x, y, v = _data(n, p, 141)
    rs = np.random.RandomState(142)
    pn = OI.init_prior_net(rs, 5, sum(z_dims))
    pn = [(W, (0.3 * rs.randn(*b.shape)).astype(np.float32)) for W, b in pn]
    seg, tab = rs.randint(0, 5, n).astype(np.int32), OI.prior_table(pn, sum(z_dims))
    new, old = _build(m), _build(m, **{MFMA: "1"})
    for eng in (new, old):
        eng.set_prior(torch.from_numpy(seg).cuda(), torch.from_numpy(tab).cuda())
    _check(m, new, old, x, y, v, 20, xs=_doses(20), expect="mfma")


@pytest.mark.parametrize("n", [40, 16])
@pytest.mark.parametrize("shape,form,scale", VALU, ids=_ids(VALU))
def test_oracle_and_wave_cache_at_every_valu_instance(shape, form, scale, n):
    """both engines against the float64 oracle on their own draws, sample_y on and off, ragged and full tile; the per-wave cache
    against no cache on the new engine to the last bit (all of it in _check)"""
    p = SHAPES[shape][1]
    x, y, v = _data(n, p, 143)
    _check(_mod(shape), _eng(shape, form), _eng(shape, form, "1"), x, y, v, 20, keys=_keys(scale), xs=_doses(20), expect="valu",
           **_scale_kw(scale))


PER_ROW = [("1-3-13", "default"), ("2-1-2", "default")]


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("shape,form", PER_ROW, ids=_ids(PER_ROW))
def test_per_row_accuracy(shape, form, n):
    """20 doses: every (lane group, pass) pair finishes a dose.  n = 1: one valid lane of 16 in the row reduction, and every ADRF
    entry is a single chain's value.  Figures and the bound: module docstring."""
    p = SHAPES[shape][1]
    x, y, v = _data(n, p, 144)
    e_n, e_o, e_b = _check(_mod(shape), _eng(shape, form), _eng(shape, form, "1"), x, y, v, 20, xs=_doses(20), expect="valu")
    print("per row, %s n=%d: worst |adrf - oracle64| vector-ALU tails %.3e, matrix-pipe tails %.3e, between the two %.3e"
          % (shape, n, e_n, e_o, e_b))
    assert e_n <= PER_ROW_BOUND, (e_n, e_o)


@pytest.mark.parametrize("n_doses", [29, 32, 33])
@pytest.mark.parametrize("shape,form", PER_ROW, ids=_ids(PER_ROW))
def test_two_owned_call_groups(shape, form, n_doses):
    """8 Philox calls in two owned groups, so a lane group renews its own noise call at pass 4: 29 doses (the last call partial: dose
    indices 29 .. 31 of the second group are masked), 32 (no remainder), 33 (a ninth, shared call in a remainder pass)"""
    p = SHAPES[shape][1]
    x, y, v = _data(40, p, 145)
    _check(_mod(shape), _eng(shape, form), _eng(shape, form, "1"), x, y, v, n_doses, xs=_doses(n_doses), expect="valu")


def test_fixed_outcome_variance():
    """sigma_y fixed, the other variances free: the sig2_y > 0 branch of the finish, at the (1,3,7) Gram instance"""
    shape = "1-3-7"
    p = SHAPES[shape][1]
    x, y, v = _data(40, p, 146)
    m = _mod(shape, sigma_y=0.5)
    assert "sigma_y" in m and "sigma_v" not in m and "sigma_x" not in m
    _check(m, _eng(shape, sigma_y=0.5), _eng(shape, tails="1", sigma_y=0.5), x, y, v, 20, xs=_doses(20), expect="valu")


# (shape, form, scale, BGM_MH_MFMA_TAILS): the event twin of every cell's fused instance, the per-chain scale where the fused kernel
# falls back ((2,1,2)) and at a two-tile Gram shape, and once the matrix-pipe engine
EVENT = [("2-1-2", "default", "fixed", None), ("1-3-7", "default", "fixed", None), ("2-1-10", "default", "fixed", None),
         ("2-1-10", "direct", "fixed", None), ("1-3-13", "direct", "fixed", None), ("1-3-7", "direct", "fixed", None),
         ("2-1-2", "default", "row", None), ("2-1-7", "default", "row", None), ("1-3-13", "default", "fixed", "1"),
         ("1-3-2", "default", "fixed", None), ("1-3-13", "default", "fixed", None), ("2-1-7", "default", "fixed", None),
         ("2-1-2-q19", "default", "fixed", None), ("1-3-2", "default", "row", None), ("2-1-10", "direct", "row", None)]


@pytest.mark.parametrize("shape,form,scale,tails", EVENT, ids=_ids(EVENT))
def test_event_form_picks_the_fused_kernels_tails(shape, form, scale, tails):
    """outcome cache mode 2 (the event form: causal_event_f_kernel chosen by bgm_causal_event_finish) against mode 0 (the fused keep
    kernel chosen by launch_mh / causal_rowadapt_api.hip) on one engine: bit-identical only if both picked the same tails.  The
    retained phase is cut by the chunks (iterations 12 and 16 ... of 10 + 7) and by an event budget of two iterations per segment."""
    from bayesgm_amd import _lib
    z_dims, p, _ = SHAPES[shape]
    n, n_doses = 100, 20
    eng = _eng(shape, form, tails)
    x, y, v = _data(n, p, 147)
    kw = dict(want_draws=True, effect=_lib.EFFECT_ADRF, x_values=_doses(n_doses), sample_y=True, **_scale_kw(scale))
    keys = _keys(scale) + ("adrf_partial", "adrf")
    try:
        eng.set_outcome_cache(False)
        ref = eng.mh_sample(x, y, v, BURN, KEEP, Q_SD, SEED, chunk=CHUNK, **kw)
        eng.set_outcome_cache(True)
        eng.outcome_cache_stats(reset=True)
        one = eng.mh_sample(x, y, v, BURN, KEEP, Q_SD, SEED, **kw)                  # one call, one segment
        assert eng.outcome_cache_stats()[1] == n * KEEP                             # chain-iterations: the event form ran
        n_slots, tiles, n_calls = eng.mh_slots(n), (n + 15) // 16, (n_doses + 3) // 4
        per_iter = n_slots * ((tiles + n_slots - 1) // n_slots) * 16 * (4 * sum(z_dims) + 4 + 32 * n_calls)
        fixed = 2 * tiles * n_calls * 64 * 2 * 4 + tiles * 8 + n_slots * 4
        eng.set_event_budget(fixed + 2 * per_iter + 100)
        got = eng.mh_sample(x, y, v, BURN, KEEP, Q_SD, SEED, chunk=CHUNK, **kw)     # three calls, segments of two iterations
        assert eng.outcome_cache_stats()[1] == n * KEEP
    finally:
        eng.set_event_budget(0)
        eng.set_outcome_cache(True)
    assert ref["acc_count"].sum().item() > 0
    _assert_same(one, ref, keys)
    _assert_same(got, ref, keys)


@pytest.mark.parametrize("shape", ["1-3-2", "2-1-2"])
def test_second_tile_of_a_slot(shape):
    """n = 16 x slots + 24: the first two slots visit a second tile, the last tile has 8 rows; 5 doses at p = 20"""
    z_dims, p, _ = SHAPES[shape]
    new, old = _eng(shape), _eng(shape, tails="1")
    slots = new.mh_slots(1 << 22)
    n = 16 * slots + 24
    assert new.mh_slots(n) == slots and n < 1 << 17
    x, y, v = _data(n, p, 148)
    xs = _doses(5)
    out_n = _sample(new, x, y, v, xs, True, False)
    out_o = _sample(old, x, y, v, xs, True, False)
    _assert_same(out_n, out_o, CHAIN)
    cached = _sample(new, x, y, v, xs, True, True)
    _assert_same(cached, out_n, CHAIN + ("adrf",))
    a_n, a_o = out_n["adrf"].cpu().numpy(), out_o["adrf"].cpu().numpy()
    assert not np.array_equal(a_n, a_o)
    assert np.abs(a_n - a_o).max() <= PER_ROW_BOUND, np.abs(a_n - a_o).max()
    ref = OC.infer_from_latent_posterior(OC.cast_model(_mod(shape), np.float64), out_n["draws"].cpu().numpy().astype(np.float64), xs,
                                         True, SEED, burn_in=BURN)
    e_n, e_o = np.abs(a_n - ref).max(), np.abs(a_o - ref).max()
    print("second tile, %s n=%d: worst |adrf - oracle64| vector-ALU tails %.3e, matrix-pipe tails %.3e" % (shape, n, e_n, e_o))
    assert e_n <= TOL and e_o <= TOL
