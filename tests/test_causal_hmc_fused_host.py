"""predict(sampler='hmc', fused_effects=True) on the CPU: the option checks of the class surface, the row blocks and the declaration
of the entry point.  No device is touched."""
import os

import numpy as np
import pytest

from bayesgm_amd import causal_hmc as HM

DATA = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))


def _bare(cls, **params):
    obj = object.__new__(cls)
    obj._p = dict(use_bnn=False, mh_precision="fp32", binary_treatment=False, **params)
    obj.params = obj._p
    return obj


def _error(call, **kw):
    with pytest.raises(ValueError) as e:
        call(DATA, x_values=[0.0], **kw)
    return str(e.value)


def test_fused_effects_belongs_to_hmc_and_has_no_draw_budget():
    from bayesgm_amd.models.causalbgm import CausalBGM
    ok = _bare(CausalBGM)
    assert "fused_effects=True belongs to sampler='hmc'" in _error(ok.predict, fused_effects=True)
    assert "fused_effects=True belongs to sampler='hmc'" in _error(ok.predict, sampler="mh", fused_effects=True)
    msg = _error(ok.predict, sampler="hmc", fused_effects=True, draw_budget_bytes=1 << 20)
    assert "fused_effects=True" in msg and "draw_budget_bytes" in msg
    # the options of the sampler are checked first, as without the argument
    for kw, word in ((dict(n_leapfrog=0), "n_leapfrog"), (dict(step_size=0.0), "step_size"), (dict(row_adapt=True), "row_adapt"),
                     (dict(q_sd=None), "q_sd"), (dict(mass="dense"), "mass must be")):
        assert word in _error(ok.predict, sampler="hmc", fused_effects=True, **kw)
        assert _error(ok.predict, sampler="hmc", fused_effects=True, **kw) == _error(ok.predict, sampler="hmc", **kw)
    with pytest.raises(ValueError, match="x_values"):          # good options go on to the next argument check, still without a device
        ok.predict(DATA, sampler="hmc", fused_effects=True)
    # the checks themselves
    HM.check_fused(False, False, 1 << 20)
    HM.check_fused(True, True, None)
    with pytest.raises(ValueError, match="sampler='hmc'"):
        HM.check_fused(True, False, None)
    with pytest.raises(ValueError, match="draw_budget_bytes"):
        HM.check_fused(True, True, 1)


def test_subclasses_refuse_hmc_as_before():
    from bayesgm_amd.models.causalbgm_bnn import CausalBGMBayes
    from bayesgm_amd.models.identifiable import IdentifiableCausalBGM
    from bayesgm_amd.models.identifiable_bnn import IdentifiableCausalBGMBayes
    for cls, params, word in ((IdentifiableCausalBGM, dict(n_segments=3), "IdentifiableCausalBGM"),
                              (IdentifiableCausalBGMBayes, dict(n_segments=3), "IdentifiableCausalBGM"),
                              (CausalBGMBayes, dict(), "not available for CausalBGMBayes")):
        m = _bare(cls, **params)
        before = _error(m.predict, sampler="hmc")
        assert word in before
        assert _error(m.predict, sampler="hmc", fused_effects=True) == before
        assert _error(m.predict, sampler="hmc", fused_effects=False) == before
        assert _error(m.predict, sampler="hmc", fused_effects=True, mass="diag") == _error(m.predict, sampler="hmc", mass="diag")
        assert "fused_effects=True belongs to sampler='hmc'" in _error(m.predict, fused_effects=True)
        assert _error(m.predict, mass="diag", fused_effects=True) == _error(m.predict, mass="diag")
    m = _bare(CausalBGMBayes)
    m._p["use_bnn"] = True
    assert "use_bnn" in _error(m.predict, sampler="hmc", fused_effects=True)
    assert _error(m.predict, sampler="hmc", fused_effects=True) == _error(m.predict, sampler="hmc")


def test_row_blocks():
    """fused_effects=False leaves the block list as block_rows makes it; True keeps a rank's blocks whole"""
    shard = [(100, 1000)]
    for n_keep, q, budget in ((20, 10, 4 * 20 * 10 * 48), (3000, 10, None), (100, 10, 1), (5, 19, 4 * 5 * 19 * 900)):
        rows = HM.block_rows(n_keep, q, budget)
        want = [(s0, min(s0 + rows, e0)) for (b0, e0) in shard for s0 in range(b0, e0, rows)]
        assert HM.predict_blocks(shard, n_keep, q, budget) == want == HM.predict_blocks(shard, n_keep, q, budget, False)
        assert want[0][0] == 100 and want[-1][1] == 1000 and all(b[1] - b[0] <= rows for b in want)
    assert len(HM.predict_blocks(shard, 20, 10, 4 * 20 * 10 * 48)) == 19
    assert HM.predict_blocks(shard, 20, 10, None, True) == shard
    ite_cut = [(0, 64), (64, 100)]                               # the binary cap's blocks pass through
    assert HM.predict_blocks(ite_cut, 20, 10, None, True) == ite_cut and HM.predict_blocks([], 20, 10) == []
    with pytest.raises(ValueError, match="draw_budget_bytes"):
        HM.predict_blocks(shard, 20, 10, 0)


def test_abi_declares_the_entry_point():
    from bayesgm_amd import _lib
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "bgm_hip.h")).read()
    name = "bgm_causal_hmc_run_effects"
    assert "BGM_API int %s(bgm_handle *h," % name in header and name in _lib.SYMBOLS
    run, fx, eff = (_lib.SYMBOLS[k][1] for k in ("bgm_causal_hmc_run", name, "bgm_causal_effects"))
    assert len(fx) == 30 and fx[:24] == run[:24] and fx[24:] == eff[8:]      # hmc_run's arguments, then those of the effects, then the stream
    src = open(os.path.join(root, "bayesgm_amd", "csrc", "build.py")).read()
    assert '"causal_hmc_fx_api.hip"' in src
