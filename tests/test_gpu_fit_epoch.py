"""bgm_causal_fit_epoch (csrc/fit_api.hip fit_epoch_impl: two streams, a ring of four parameter buffers, the Adam step fused into the
gradient-tile kernel, rider workgroups that replay a later minibatch's rows, ordering through device counters) against the sequential
order it promises "bit for bit": the per-minibatch calls fit_z_sync / fit_theta_grad / fit_theta_apply / fit_z_step of CausalBGM.fit's
host loop, at engine level, on every case of tests/_fit_epoch_cases.py (every chain family, minibatch instantiation and ring edge;
tests/test_fit_epoch_host.py proves the coverage from the table).

Every comparison with the host loop is np.array_equal: latent table, its Adam slots, the three networks, both moment vectors, the step
counters.  Two tolerances only, both taken from existing tests: the loss vectors are fp64 atomic sums in another order, 1e-6 * max(1, |a|)
(tests/test_gpu_class_level.py); the float64 oracle at 4 steps and lr = 1e-3, 3e-4 absolute on weights and latents
(tests/test_gpu_fit.py, derived in its docstring).  Observed against the oracle (MI355X): see DESIGN.md section 4c."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import causal as OC  # noqa: E402
from oracle import fit as OF      # noqa: E402
from tests import _fit_epoch_cases as FE  # noqa: E402
from tests.test_gpu_causal import _model, _data, _engine  # noqa: E402

LR = FE.LR
EXACT = ("data_z", "zm", "zv", "g", "f", "h", "m", "v", "steps")
PATHS = {"chain": "fit=fit_chain_kernel", "gx": "fit=gx_causal_fit_kernel", "blob": "fit=fit_fwd_kernel"}


@functools.lru_cache(maxsize=None)
def _panel(p, z_dims, binary, n, g_units, f_units, h_units):
    m = _model(31, list(z_dims), p, binary, g_units=g_units, f_units=f_units, h_units=h_units)
    x, y, v = _data(n, p, 32, binary)
    z0 = np.random.RandomState(33).randn(n, sum(z_dims)).astype(np.float32)
    return m, x, y, v, z0


def _panel_of(case):
    return _panel(*(case[k] for k in ("p", "z_dims", "binary", "n", "g_units", "f_units", "h_units")))


def _flat(net):
    return np.concatenate([np.concatenate([np.asarray(W).ravel(), np.asarray(b).ravel()]) for W, b in net])


def _new_engine(case):
    m = _panel_of(case)[0]
    return _engine(m, g_units=list(case["g_units"]), f_units=list(case["f_units"]), h_units=list(case["h_units"]))


def _perm(case, seed=0, n_use=None):
    """a fixed list of distinct rows: the minibatches are its consecutive slices of B"""
    return np.random.RandomState(100 + seed).permutation(case["n"])[:n_use or case["n_use"]].astype(np.int32)


def _session(case, ops, epoch, eng=None, first=None):
    """One fit session from the case's initial state.  ops: ("epoch", rows[, with_loss]) -- one eng.fit_epoch call (epoch=True) or the
    host loop over the same minibatches (epoch=False); ("host", rows) -- the host loop in both; ("flush",) -- fit_z_sync(None) in replay
    mode.  first(eng, state): called once the session is open (the refusals).  Returns the whole state as host arrays."""
    import torch
    from bayesgm_amd import _lib
    m, x, y, v, z0 = _panel_of(case)
    if eng is None:
        eng = _new_engine(case)
    else:
        eng.set_model(g=m["g"], f=m["f"], h=m["h"])          # (an earlier session's fit_end left the trained weights behind)
    dev, B, lazy = eng.device, case["B"], case["lazy"]
    xd, yd, vd, zd = (torch.from_numpy(a).to(dev) for a in (x.ravel(), y.ravel(), v, z0.copy()))
    zm, zv = torch.zeros_like(zd), torch.zeros_like(zd)
    loss, loss_z = (torch.zeros(8, device=dev, dtype=torch.float64) for _ in range(2))
    npar = eng.fit_begin(case["n"], B)
    grad = torch.empty(npar, device=dev)

    def host_loop(rows, ls, lz):
        for i in range(0, rows.numel(), B):
            idx = rows[i:i + B]
            if lazy == 2:
                eng.fit_z_sync(zd, zm, zv, idx, LR)
            eng.fit_theta_grad(xd, yd, vd, zd, idx, int(idx.numel()), grad, ls)
            eng.fit_theta_apply(grad, LR)
            eng.fit_z_step(xd, yd, vd, zd, zm, zv, idx, int(idx.numel()), LR, lazy, lz)

    if first is not None:
        first(eng, dict(x=xd, y=yd, v=vd, z=zd, zm=zm, zv=zv))
    for op in ops:
        if op[0] == "call":
            if epoch:
                op[1](dev)
            continue
        if op[0] == "flush":
            if lazy == 2:
                eng.fit_z_sync(zd, zm, zv, None, LR)
            continue
        rows = torch.from_numpy(op[1]).to(dev)
        with_loss = len(op) < 3 or op[2]
        ls, lz = (loss, loss_z) if with_loss else (None, None)
        if op[0] == "epoch" and epoch:
            eng.fit_epoch(xd, yd, vd, zd, zm, zv, rows, B, LR, LR, lazy, ls, lz)
        else:
            host_loop(rows, ls, lz)
    if lazy == 2:
        eng.fit_z_sync(zd, zm, zv, None, LR)
    st = eng.fit_state()
    out = dict(data_z=zd.cpu().numpy(), zm=zm.cpu().numpy(), zv=zv.cpu().numpy(), m=st["m"], v=st["v"],
               steps=np.array([st["t_theta"], st["t_z"]], np.int64), loss=loss.cpu().numpy(), loss_z=loss_z.cpu().numpy(),
               path=eng.describe(B))
    for nid, key in ((_lib.NET_G, "g"), (_lib.NET_F, "f"), (_lib.NET_H, "h")):
        dims = [m[key][0][0].shape[0]] + [W.shape[1] for W, _ in m[key]]
        out[key] = _flat(eng.get_weights(nid, dims))
    eng.fit_end()
    return out


def _run(case, epoch):
    return _session(case, [("epoch", _perm(case))], epoch)


@functools.lru_cache(maxsize=None)
def _epoch_result(name):
    return _run(FE.BY_NAME[name], True)


@functools.lru_cache(maxsize=None)
def _host_result(name):
    return _run(FE.BY_NAME[name], False)


def digest(out):
    h = hashlib.sha256()
    for k in EXACT:
        h.update(np.ascontiguousarray(out[k]).tobytes())
    return h.hexdigest()


def _assert_same(a, b, what):
    for k in EXACT:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))
    for k in ("loss", "loss_z"):                       # fp64 atomics: summation order
        assert np.all(np.abs(a[k] - b[k]) <= 1e-6 * np.maximum(1.0, np.abs(a[k]))), (what, k, a[k], b[k])


def _assert_moved(case, out, n_steps):
    m, _, _, _, z0 = _panel_of(case)
    assert np.abs(out["data_z"] - z0).max() > 0
    for k in "gfh":
        assert out[k].shape == _flat(m[k]).shape and not np.array_equal(out[k], _flat(m[k])), k
    assert list(out["steps"]) == [n_steps, n_steps]
    assert np.isfinite(out["data_z"]).all() and all(np.isfinite(out[k]).all() for k in "gfh")


# ---- a. equality with the sequential order ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in FE.CASES])
def test_epoch_call_equals_the_host_loop(name):
    case, pl = FE.BY_NAME[name], FE.plan_of(FE.BY_NAME[name])
    a, b = _epoch_result(name), _host_result(name)
    _assert_same(a, b, name)
    _assert_moved(case, a, pl["n_mb"])
    assert a["loss"][0] != 0 and a["loss_z"][6] != 0
    for r in (a, b):                                   # the step kernels of the open session are the restatement's family
        assert PATHS[pl["family"]] in r["path"], (pl["family"], r["path"])
        assert sum(s in r["path"] for s in PATHS.values()) == 1


# ---- b. sessions, not single calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p200-z2-mb9", "t2-z2-mb9", "p200-z1-mb9"])
def test_successive_calls_and_mixed_use_in_one_session(name):
    """Three epoch calls of 5, 3 and 9 minibatches (short last ones of 17, 26 and 1 rows) on the counters, ring and replay stamps the call
    before left behind, the first without loss accumulators, a flush between two of them, then two host-loop minibatches and another
    epoch call."""
    case = FE.BY_NAME[name]
    ops = [("epoch", _perm(case, 1, 145), False), ("epoch", _perm(case, 2, 90)), ("flush",), ("epoch", _perm(case, 3, 257)),
           ("host", _perm(case, 4, 49)), ("epoch", _perm(case, 5, 129))]
    a, b = _session(case, ops, True), _session(case, ops, False)
    _assert_same(a, b, name)
    _assert_moved(case, a, 5 + 3 + 9 + 2 + 5)


# ---- the same with the device busy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t2-z2-mb9", "p20-z2-mb9", "p200-z2-mb9"])
def test_epoch_calls_beside_other_work_on_the_device(name):
    """On an idle device the latent stream never falls four minibatches behind the parameter stream, so the wait of theta phase k on the
    latent phase k - D (whose parameter buffer step k overwrites, and whose riders replayed minibatch k's rows) never has to hold anything
    up, and a library without it computes the same bits.  Eight other streams each running eight passes over a 512 MB tensor share the
    hardware queues and the compute units with the two streams of the call and delay them unevenly: epoch calls of nine minibatches,
    each issued right after such a load, must still give the host loop's bits.  Six sessions of two such calls, each on an engine of
    its own: which hardware queue the library's second stream shares with the load is settled when the stream is created.  (The
    first call of a session runs on the idle device: the handle probes there whether its two streams run side by side.)"""
    import torch
    case = FE.BY_NAME[name]
    dev = torch.device("cuda", 0)
    big = torch.ones(1 << 27, device=dev)
    others = [torch.cuda.Stream() for _ in range(8)]

    def load(_):
        torch.cuda.synchronize()                      # (the load of the call before has drained: a wait never outlasts its 2 s bound)
        for s in others:
            with torch.cuda.stream(s):
                for _ in range(8):
                    big.sin_()

    ops = [("epoch", _perm(case, 1, 96)), ("call", load), ("epoch", _perm(case, 2, 272)), ("call", load), ("epoch", _perm(case, 3, 272))]
    want = _session(case, ops, False)
    _assert_moved(case, want, 3 + 9 + 9)
    try:
        for r in range(6):
            _assert_same(_session(case, ops, True), want, "%s, session %d" % (name, r))
    finally:
        torch.cuda.synchronize()


# ---- c. caller stream --------------------------------------------------------------------------------------------------------
def test_another_caller_stream_then_the_default_stream_on_one_handle():
    """(the second session makes the handle probe its two streams again: epoch_probe_stream)"""
    import torch
    name = "p200-z2-mb9"
    case = FE.BY_NAME[name]
    ops = [("epoch", _perm(case))]
    eng = _new_engine(case)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = _session(case, ops, True, eng=eng)
    torch.cuda.synchronize()
    b = _session(case, ops, True, eng=eng)
    _assert_same(_epoch_result(name), a, "side stream")
    _assert_same(_epoch_result(name), b, "default stream after it")


# ---- d. rows outside the permutation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FE.OUTSIDE_CASES)
def test_rows_outside_the_permutation(name):
    case = FE.BY_NAME[name]
    a = _epoch_result(name)
    _assert_same(a, _host_result(name), name)
    out = np.setdiff1d(np.arange(case["n"]), _perm(case))
    assert len(out) == case["n"] - case["n_use"] > 0
    if case["lazy"] == 1:
        z0 = _panel_of(case)[4]
        assert np.array_equal(a["data_z"][out], z0[out])
        assert not a["zm"][out].any() and not a["zv"][out].any()
        assert np.abs(a["data_z"][_perm(case)] - z0[_perm(case)]).max(axis=1).min() > 0      # ... and every row inside it moved


# ---- e. event ordering -------------------------------------------------------------------------------------------------------
def test_event_ordering_gives_the_same_bits():
    """BGM_FIT_NO_FLAGS=1 (read once per process): the ordering the library falls back to by itself when its two streams do not run side
    by side, HIP events instead of device counters -- one child process, the digests of its results against this process's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_fit_epoch_cases.py")] + FE.EVENT_CASES, cwd=root,
                       env=dict(os.environ, BGM_FIT_NO_FLAGS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = dict(line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0] in FE.BY_NAME)
    assert sorted(got) == sorted(FE.EVENT_CASES), r.stdout[-2000:]
    for name in FE.EVENT_CASES:
        assert got[name] == digest(_epoch_result(name)), name
        assert got[name] == digest(_host_result(name)), name


@pytest.mark.parametrize("setting", FE.EPOCH_SWITCHES + FE.VARIANT_SWITCHES)
def test_debug_switch_keeps_the_sequential_order(setting):
    """Every BGM_FIT_* development switch (read once per process, so one fresh child per setting): under the switch the epoch call still
    gives the bits of the host loop run in the same process.  The switches that only reorder the epoch call's launches (no overlap, Adam
    and replay as launches of their own, a shorter ring) must also give the bits of this process, which runs with none of them set: every
    mode is "the sequential order bit for bit".  The switches that select another kernel variant or family change both sides alike and
    promise nothing against the default."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    key, value = setting.split("=")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_fit_epoch_cases.py"), "--host"] + FE.SWITCH_CASES, cwd=root,
                       env=dict(os.environ, **{key: value}), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = {w[0]: w[1:] for w in (line.split() for line in r.stdout.splitlines()) if w and w[0] in FE.BY_NAME}
    assert sorted(got) == sorted(FE.SWITCH_CASES) and all(len(d) == 2 for d in got.values()), r.stdout[-2000:]
    for name in FE.SWITCH_CASES:
        print(setting, name, "epoch", got[name][0][:12], "host loop", got[name][1][:12], "default", digest(_epoch_result(name))[:12])
    for name in FE.SWITCH_CASES:
        assert got[name][0] == got[name][1], (setting, name)
        if setting in FE.EPOCH_SWITCHES:
            assert got[name][0] == digest(_epoch_result(name)), (setting, name)


# ---- f. one anchor outside the project's kernels --------------------------------------------------------------------------
@pytest.mark.parametrize("name", FE.ORACLE_CASES)
def test_epoch_call_matches_the_float64_oracle(name):
    """oracle.fit.fit_step in float64 on the same four minibatches (32, 32, 32, 17 rows; lr = 1e-3); lazy = 0 and 2 against the dense
    recursion, lazy = 1 against lazy_z=True.  3e-4 absolute on weights and latents: the bar tests/test_gpu_fit.py derives for this
    setting.  Observed on an MI355X over the nine cases: at most 2.7e-7 on the latents (which moved 1.0e-3 .. 2.6e-3) and 7.7e-6 on the
    weights (g of the two-latent-tile case; 1.9e-6 at p = 200, 8.4e-7 at p = 20; f and h below 1.1e-7)."""
    case = FE.BY_NAME[name]
    m, x, y, v, z0 = _panel_of(case)
    a = _epoch_result(name)
    st = OF.FitState(OC.cast_model(m, np.float64), z0.astype(np.float64), LR, LR)
    x64, y64, v64 = (t.astype(np.float64) for t in (x, y, v))
    rows = _perm(case)
    assert len(rows) == 113 and case["B"] == 32
    for i in range(0, len(rows), 32):
        OF.fit_step(st, x64, y64, v64, rows[i:i + 32], lazy_z=(case["lazy"] == 1))
    dz = np.abs(a["data_z"] - st.data_z).max()
    dw = {k: np.abs(a[k] - _flat(st.m[k])).max() for k in "gfh"}
    print("fit_epoch vs float64 oracle %s: latents %.3e, g %.3e, f %.3e, h %.3e (latents moved %.3e)" % (
        name, dz, dw["g"], dw["f"], dw["h"], np.abs(st.data_z - z0).max()))
    assert dz <= 3e-4, dz
    for k in "gfh":
        assert dw[k] <= 3e-4, (k, dw[k])


# ---- g. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable():
    import torch
    name = "p200-z2-mb9"
    case = FE.BY_NAME[name]
    ops = [("epoch", _perm(case))]
    eng = _new_engine(case)
    dev = eng.device
    m, x, y, v, z0 = _panel_of(case)
    xd, yd, vd, zd = (torch.from_numpy(t).to(dev) for t in (x.ravel(), y.ravel(), v, z0.copy()))
    zm, zv = torch.zeros_like(zd), torch.zeros_like(zd)
    rows = torch.from_numpy(_perm(case)).to(dev)
    with pytest.raises(RuntimeError, match="fit_begin first"):                    # no session open
        eng.fit_epoch(xd, yd, vd, zd, zm, zv, rows, 32, LR, LR, 2)
    assert torch.equal(zd.cpu(), torch.from_numpy(z0))
    _assert_same(_epoch_result(name), _session(case, ops, True, eng=eng), "after the call without a session")

    def empty_list(e, s):
        with pytest.raises(RuntimeError, match="bad minibatch list"):
            e.fit_epoch(s["x"], s["y"], s["v"], s["z"], s["zm"], s["zv"], torch.empty(0, dtype=torch.int32, device=dev), 32, LR, LR, 2)

    def batch_too_large(e, s):
        with pytest.raises(RuntimeError, match="batch out of range"):
            e.fit_epoch(s["x"], s["y"], s["v"], s["z"], s["zm"], s["zv"], rows, 33, LR, LR, 2)

    for first in (empty_list, batch_too_large):        # refused inside the session that then runs the valid call
        _assert_same(_epoch_result(name), _session(case, ops, True, eng=eng, first=first), first.__name__)
