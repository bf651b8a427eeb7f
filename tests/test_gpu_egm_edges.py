"""The deterministic CausalBGM EGM warm start (csrc/egm_api.hip: egm_kernels.h, egm_chain.h, egm_chain_gen.h) at the edges of its kernel
routing, against oracle/egm.py in float64.  tests/_egm_edges_ref.py restates the host plan and holds the cases and their inputs;
tests/test_egm_edges_host.py shows on the CPU which of the seven discriminator-step and seven generator-step kernels every case reaches,
and that the oracle alone (in float64, and in float32 for the long and the shortest batches) meets the conditions put on the inputs.

What the cases are there for: the discriminator working set in LDS and in the workspace (B = 39 / 40, 65, 513 = EGM_THREADS + 1, 2, 3, a
wide discriminator at B = 16); the masked widths of the chained discriminator (49-17-1, 63-31-16, 64-32-16, 50-20-3 at one and two row
tiles and with two latent tiles; 48-32-8 and 64-33-8 just outside); heads with a third hidden width of 1, 5, 16 (17 just outside) and
inputs of 16 and 15 columns; g and e of depth 1 and 2 / 7; the one-row-tile generator chains at p = 100 and p = 200; the extent edges
p = 95, 96, 111, 112, 191, 192, 207, 208 where the two steps key on different tile counts; use_z_rec = 0; idx with rows 0 and n - 1.

Bars (tests/test_gpu_egm.py): losses 2e-5 relative plus its absolute floors, gradients 5e-5 of the largest entry of the same step,
parameters after three alternating rounds (two discriminator steps, one generator step; lr 2e-4) 2e-5 absolute over all of g | e | f | h
and the discriminator -- with batch statistics the hidden-layer discriminator biases (zero exact gradient) are held to 12 lr instead,
nothing else is excluded.  Chain cases run a second time with BGM_EGM_NO_CHAIN and BGM_EGM_NO_CHAIN_GEN set: same bars, and the two
forms' gradients within 1e-4 of the largest entry.  No case has a bound of its own: the float32 oracle stays inside the bars on every
batch of 40 rows and more (tests/test_egm_edges_host.py).  Every check prints an EGM-EDGE line (pytest -s) before it asserts.

Measured on an MI355X: 126 tests in 3.3 s.  Worst error / bar: gradients 0.08 (ws-b65), losses 0.06, trained parameters 0.57 at
ws-b40-global (1.12e-5 / 1.14e-5; the float32 ORACLE deviates by 1.36e-5 / 1.54e-5 there) and below 0.1 everywhere else, chains against
workgroup kernels 0.007, fused against split 3.0e-8.  ws-b2 and ws-b3 use fixed statistics: batch statistics of two and three rows cost
the float32 oracle more than a quarter of the bars (the kernels missed the parameter bar at B = 2 with them, 2.38e-5).  DESIGN.md 4ae."""
import numpy as np
import pytest

import _egm_edges_ref as E

pytestmark = pytest.mark.gpu

BAR_LOSS, BAR_GRAD, BAR_PARAM, BAR_FORMS, BAR_SPLIT = 2e-5, 5e-5, 2e-5, 1e-4, 1e-7
ids = [c["name"] for c in E.CASES]
CHAIN_CASES = [c for c in E.CASES if E.is_chain(c)]
SPLIT_CASES = [c for c in E.CASES if c["split"]]
SWITCHES = ("BGM_EGM_NO_CHAIN", "BGM_EGM_NO_CHAIN_GEN")


def _setup(c):
    """Engine with the case's networks installed and an open session (dz_units, g_units, e_units, f_units, h_units, use_z_rec and the
    normalisation mode from the case; the switches are read by egm_begin from the environment of the moment)."""
    import torch
    from bayesgm_amd.engine import CausalEngine
    I = E.inputs(c["name"])
    eng = CausalEngine(c["p"], list(c["z_dims"]), binary_treatment=c["binary"], g_units=list(c["g_units"]), f_units=list(c["f_units"]),
                       h_units=list(c["h_units"]), e_units=list(c["e_units"]))
    eng.set_model(g=I.nets["g"], f=I.nets["f"], h=I.nets["h"], e=I.nets["e"])
    if c["fixed"]:
        eng.set_disc_norm("fixed")
    eng.egm_begin(c["B"], list(c["dz_units"]), E.LR, c["use_z_rec"], I.dz)
    dev = {k: torch.from_numpy(getattr(I, k)).cuda() for k in ("v", "x", "y")}
    return eng, I, dev


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_GRADS, _TRAINED = {}, {}


def _grads(c, switched):
    """One discriminator and one generator step with apply = False -> losses, gradients and the parameters read back (cached per form)."""
    key = (c["name"], switched)
    if key not in _GRADS:
        import torch
        eng, I, dev = _setup(c)
        n_gen, n_dz = eng.egm_sizes()
        z, idx, _ = I.grad_batch
        zd, idd = _cu(z), _cu(idx)
        out_d, out_g = torch.zeros(2, device="cuda"), torch.zeros(6, device="cuda")
        eng.egm_disc_step(zd, idd, dev["v"], E.EPS_GRAD, apply=False, out=out_d)
        gd = eng.egm_read(3, n_dz)
        eng.egm_gen_step(zd, idd, dev["v"], dev["x"], dev["y"], apply=False, out=out_g)
        gg = eng.egm_read(2, n_gen)
        _GRADS[key] = dict(d_losses=out_d.cpu().numpy().astype(np.float64), g_losses=out_g.cpu().numpy().astype(np.float64), d_grads=gd, g_grads=gg,
                           theta_g=eng.egm_read(0, n_gen), theta_d=eng.egm_read(1, n_dz))
        eng.egm_end()
    return _GRADS[key]


def _train(c, switched, split=False):
    """ROUNDS alternating rounds with Adam -> parameters read from the session, and g's first layer as get_weights returns it after egm_end."""
    key = (c["name"], switched, split)
    if key not in _TRAINED:
        import torch
        eng, I, dev = _setup(c)
        n_gen, n_dz = eng.egm_sizes()
        bg, bd = torch.empty(n_gen, device="cuda"), torch.empty(n_dz, device="cuda")
        for d1, d2, g in I.rounds:
            for z, idx, eps in (d1, d2):
                eng.egm_disc_step(_cu(z), _cu(idx), dev["v"], eps, apply=not split)
                if split:
                    eng.egm_grad(1, 1.0, bd)
                    eng.egm_apply(1, bd)
            z, idx, _ = g
            eng.egm_gen_step(_cu(z), _cu(idx), dev["v"], dev["x"], dev["y"], apply=not split)
            if split:
                eng.egm_grad(0, 1.0, bg)
                eng.egm_apply(0, bg)
        tg, td = eng.egm_read(0, n_gen), eng.egm_read(1, n_dz)
        eng.egm_end()
        g_tr = eng.get_weights(0, [sum(c["z_dims"])] + list(c["g_units"]) + [c["p"] + 1])
        _TRAINED[key] = dict(theta_g=tg, theta_d=td, g_first=g_tr[0][0])
    return _TRAINED[key]


def _check_grads(c, got, form):
    I, r = E.inputs(c["name"]), E.grads64(c["name"])
    dl = np.abs(got["d_losses"] - r.d_losses) / (BAR_LOSS * np.abs(r.d_losses) + np.array([1e-6, 1e-5]))
    gl = np.abs(got["g_losses"] - r.g_losses) / (BAR_LOSS * np.abs(r.g_losses) + 1e-6)
    ed, eg = E.rel(got["d_grads"], r.d_grads), E.rel(got["g_grads"], r.g_grads)
    print("EGM-EDGE case=%s form=%s routes=%s/%s disc grads %.2e gen grads %.2e (bar %.0e) loss ratios %.3f %.3f"
          % (c["name"], form, c["want_disc"], c["want_gen"], ed, eg, BAR_GRAD, dl.max(), gl.max()))
    assert np.isfinite(got["d_grads"]).all() and np.isfinite(got["g_grads"]).all()
    assert dl.max() <= 1, (got["d_losses"], r.d_losses)
    assert gl.max() <= 1, (got["g_losses"], r.g_losses)
    assert ed <= BAR_GRAD, (ed, int(np.abs(got["d_grads"] - r.d_grads).argmax()))
    assert eg <= BAR_GRAD, (eg, int(np.abs(got["g_grads"] - r.g_grads).argmax()))
    # apply = False left both parameter sets exactly as installed
    assert np.array_equal(got["theta_g"], E.flat_gen(I.nets)) and np.array_equal(got["theta_d"], E.flat_disc(I.dz))


def _check_trained(c, got, form):
    I, r = E.inputs(c["name"]), E.trained64(c["name"])
    inert = E.inert_disc_mask(c["name"])
    eg = float(np.abs(got["theta_g"] - r.theta_g).max())
    ed = float(np.abs(got["theta_d"] - r.theta_d)[~inert].max())
    ei = float(np.abs(got["theta_d"] - r.theta_d)[inert].max()) if inert.any() else 0.0
    moved = float(np.abs(got["theta_g"] - E.flat_gen(I.nets)).max())
    print("EGM-EDGE case=%s form=%s rounds=%d |dtheta| g|e|f|h %.2e discriminator %.2e (bar %.0e) inert biases %.2e (bar %.1e) moved %.1e"
          % (c["name"], form, E.ROUNDS, eg, ed, BAR_PARAM, ei, 12 * E.LR, moved))
    assert eg <= BAR_PARAM, (eg, int(np.abs(got["theta_g"] - r.theta_g).argmax()))
    assert ed <= BAR_PARAM, ed
    assert ei <= 12 * E.LR
    assert moved > 2e-4          # Adam's first steps are ~lr each
    assert np.abs(got["g_first"] - r.g_first).max() <= BAR_PARAM          # after egm_end the handle holds the trained g


@pytest.mark.parametrize("c", E.CASES, ids=ids)
def test_step_gradients_match_oracle(c):
    _check_grads(c, _grads(c, False), "default")


@pytest.mark.parametrize("c", E.CASES, ids=ids)
def test_alternating_adam_rounds_track_oracle(c):
    """The second and third round run on what the first one's Adam wrote: the masked Adam of the chains and the transposed mirror their
    backward passes read."""
    _check_trained(c, _train(c, False), "default")


@pytest.mark.parametrize("c", CHAIN_CASES, ids=[c["name"] for c in CHAIN_CASES])
def test_chains_switched_off_meet_the_same_bars(c, monkeypatch):
    for s in SWITCHES:
        monkeypatch.setenv(s, "1")
    off = _grads(c, True)
    _check_grads(c, off, "workgroup")
    _check_trained(c, _train(c, True), "workgroup")
    for s in SWITCHES:
        monkeypatch.delenv(s)
    on = _grads(c, False)
    for k in ("d_grads", "g_grads"):
        e = E.rel(on[k], off[k].astype(np.float64))
        print("EGM-EDGE case=%s chains vs workgroup kernels %s %.2e (bar %.0e)" % (c["name"], k, e, BAR_FORMS))
        assert e <= BAR_FORMS, (k, e)


@pytest.mark.parametrize("c", SPLIT_CASES, ids=[c["name"] for c in SPLIT_CASES])
def test_split_step_equals_fused_step_on_one_row_tile(c):
    """step with apply = 0, egm_grad, egm_apply takes the Adam steps the fused step takes: the one-row-tile generator chains, whose
    transposed mirror the apply kernel maintains."""
    a, b = _train(c, False), _train(c, False, split=True)
    eg, ed = float(np.abs(a["theta_g"] - b["theta_g"]).max()), float(np.abs(a["theta_d"] - b["theta_d"]).max())
    print("EGM-EDGE case=%s fused vs split g|e|f|h %.2e discriminator %.2e (bar %.0e)" % (c["name"], eg, ed, BAR_SPLIT))
    assert eg <= BAR_SPLIT and ed <= BAR_SPLIT
