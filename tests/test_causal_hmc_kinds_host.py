"""The table of what the HMC sampler computes with what (causal_hmc.RESULT_KINDS) against engine.hmc_sample on an engine without a
handle or a device, and the declarations of the seven bgm_causal_hmc_run* entry points against a literal copy.  No device is touched:
a call that gets past the option checks ends in AttributeError (the bare engine has no device), a refused one in ValueError."""
import ctypes as C

import numpy as np
import pytest

from bayesgm_amd import _lib
from bayesgm_amd import causal_hmc as HM

DATA = (np.zeros((4, 1), np.float32), np.zeros((4, 1), np.float32), np.zeros((4, 5), np.float32))
RUN = DATA + (40, 5, 0.1, 2, 7)      # burn_in (long enough for mass='diag'), n_keep, step_size, n_leapfrog, seed
KINDS = list(HM.RESULT_KINDS.values())
# an option of hmc_sample -> (the keywords that turn it on, the field of a kind's record that says whether the combination exists)
OPTIONS = {
    "trajectory": (dict(max_trajectory=0.5), "traj"),
    "jitter": (dict(jitter=True), "traj"),
    "partial": (dict(partial=True), "obs"),
    "draws": (dict(row_draws=True), "draws"),
    "tails": (dict(row_tails=2), "tails"),
    "binary": (dict(), "treatment"),
    "continuous": (dict(), "treatment"),
    "metric_partial_wide": (dict(mass="diag", partial=True), "hole"),
    "metric_partial_narrow": (dict(mass="diag", partial=True), "hole"),
}
# the words the refusals carry today (asserted by tests/test_causal_hmc_*_host.py and tests/test_gpu_causal_hmc_*.py)
WORDS = {
    ("tails", "traj"): "max_trajectory / jitter are not available with row_tails: the tail-buffer kernels (hmc_run_rows_tails) have no variant with a trajectory length per chain",
    ("contrasts", "traj"): "max_trajectory / jitter are not available with row_contrasts: the dose-contrast kernels (hmc_run_rows_contrasts) have no variant with a trajectory length per chain",
    ("choice", "traj"): "max_trajectory / jitter are not available with row_choice: the dose-choice kernels (hmc_run_rows_choice) have no variant with a trajectory length per chain",
    ("group_ite", "traj"): "max_trajectory / jitter are not available with effect=EFFECT_GROUP_ITE: the label-sum kernels (hmc_run_group_effects) have no variant with a trajectory length per chain",
    ("adrf", "draws"): "row_draws belongs to row_effects=True", ("ite", "draws"): "row_draws belongs to row_effects=True",
    ("group_ite", "draws"): "row_draws belongs to row_effects=True",
    ("adrf", "tails"): "row_tails belongs to row_effects=True", ("ite", "tails"): "row_tails belongs to row_effects=True",
    ("group_ite", "tails"): "row_tails belongs to row_effects=True",
    ("choice", "tails"): "row_choice is not available with row_contrasts or row_tails: the dose-choice kernels (hmc_run_rows_choice) have no variant with contrasts or tail buffers",
    ("contrasts", "treatment"): "row_contrasts is the contrast between two doses of a continuous treatment; a binary treatment has its per-row effect already (effect=EFFECT_ITE)",
    ("choice", "treatment"): "row_choice is the choice among the doses of a continuous treatment; a binary treatment has its per-row effect already (effect=EFFECT_ITE)",
    ("group_ite", "treatment"): "effect=EFFECT_GROUP_ITE sums the treatment effect of a binary treatment; a continuous treatment has its dose-response (effect=EFFECT_ADRF)",
    ("choice", "hole"): "more than 11 latent features (here 12)",
}


def _engine(binary, q=10):
    from bayesgm_amd.engine import CausalEngine
    eng = object.__new__(CausalEngine)
    eng.binary, eng.q = binary, q
    return eng


def _request(kind):
    kw = dict(kind.request)
    if kw.get("row_effects") or kind.name == "adrf":
        kw["x_values"] = [0.0, 1.0]
    if kind.name == "group_ite":
        kw.update(labels=np.zeros(4, np.int32), n_labels=1)
    if kind.name == "tails":
        kw["row_tails"] = 2
    return kw


def _exists(kind, option):
    """(the combination exists, hmc_sample itself refuses it where it does not) by the kind's record"""
    field = OPTIONS[option][1]
    if field == "treatment":
        return kind.treatment == option, "treatment" not in kind.late
    if field == "hole":
        return kind.hole is None or option == "metric_partial_narrow", True
    return bool(getattr(kind, field)), field not in kind.late


PAIRS = [(k, o) for k in KINDS for o in OPTIONS if (k.name, o) != ("tails", "tails")]      # (there the kind is the option)


@pytest.mark.parametrize("kind, option", PAIRS, ids=["%s-%s" % (k.name, o) for k, o in PAIRS])
def test_hmc_sample_refuses_exactly_what_the_table_says_does_not_exist(kind, option):
    kw, field = dict(_request(kind), **OPTIONS[option][0]), OPTIONS[option][1]
    binary = option == "binary" if field == "treatment" else kind.treatment == "binary"
    eng = _engine(binary, q=12 if option == "metric_partial_wide" else 11 if option == "metric_partial_narrow" else 10)
    exists, refused_here = _exists(kind, option)
    if exists or not refused_here:      # past the option checks: the bare engine has no device
        with pytest.raises(AttributeError):
            eng.hmc_sample(*RUN, **kw)
        return
    with pytest.raises(ValueError) as e:
        eng.hmc_sample(*RUN, **kw)
    assert WORDS[(kind.name, field)] in str(e.value)


def test_the_table_covers_the_kinds_and_names_their_kernels():
    assert list(HM.RESULT_KINDS) == ["adrf", "ite", "group_ite", "rows", "tails", "contrasts", "choice"]
    from bayesgm_amd.engine import CausalEngine
    for kind in KINDS:
        assert callable(getattr(CausalEngine, kind.method)), kind.name
        assert HM.result_kind(kind.request.get("effect", _lib.EFFECT_NONE), kind.request.get("row_effects", False),
                              2 if kind.name == "tails" else None, kind.request.get("row_contrasts", False),
                              kind.request.get("row_choice", False)) is kind
    assert HM.result_kind(_lib.EFFECT_NONE) is None
    assert sorted(_engine(False)._row_routes()) == sorted(k.name for k in KINDS if k.request.get("row_effects"))
    # what is refused only after the device is touched keeps the error it has always had (tests/test_gpu_causal_hmc_partial.py: the
    # library's BGM_E_UNSUPPORTED for the pattern; tests/test_causal_hmc_contrast_host.py: the plain per-row route on a binary engine)
    assert {k.name: k.late for k in KINDS} == dict(adrf=("treatment", "obs"), ite=("treatment",), group_ite=("obs",), rows=("treatment",),
                                                   tails=("treatment",), contrasts=(), choice=())
    with pytest.raises(ValueError, match="effect must be EFFECT_NONE, EFFECT_ADRF, EFFECT_ITE or EFFECT_GROUP_ITE"):
        _engine(False).hmc_sample(*RUN, effect=3)
    with pytest.raises(ValueError, match="row_effects and effect exclude each other"):
        _engine(False).hmc_sample(*RUN, effect=_lib.EFFECT_ADRF, row_effects=True, x_values=[0.0])
    # predict_individual's clause reads the same record
    with pytest.raises(ValueError, match="interval='tails': the tail-buffer kernels have no variant with a trajectory length per chain"):
        HM.check_trajectory(0.5, False, True, "tails")
    assert HM.check_trajectory(0.5, True, True, "quantile") == (0.5, 1)


def test_a_segment_method_binds_like_a_written_out_parameter_list():
    eng = _engine(False)
    with pytest.raises(TypeError, match="unexpected keyword argument 'row_tail'"):
        eng.hmc_run_rows_tails(*([None] * 12), row_tail=None)
    with pytest.raises(TypeError, match="missing a required argument: 'seed'"):
        eng.hmc_run_rows_effects(*([None] * 11))
    with pytest.raises(TypeError, match="too many positional arguments"):
        eng.hmc_run(*([None] * 40))
    with pytest.raises(TypeError, match="multiple values for argument 'x'"):
        eng.hmc_run_rows_choice(*([None] * 12), x=None)


# today's declarations, written out: the handle and the 23 common arguments, then each entry point's own, then the stream
P, I64, I32, F32, U64 = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_uint64
PREFIX = [P, P, P, P, I64, I64, P, P, P, P, P, P, I32, F32, F32, I32, I32, I32, I32, I32, U64, P, P, I32]
ARGTYPES = {
    "bgm_causal_hmc_run": PREFIX + [P],
    "bgm_causal_hmc_run_effects": PREFIX + [I32, P, I32, P, P, P],
    "bgm_causal_hmc_run_row_effects": PREFIX + [I32, P, I32, P, P, P],
    "bgm_causal_hmc_run_row_tails": PREFIX + [I32, P, I32, P, P, P, I32, P],
    "bgm_causal_hmc_run_row_contrasts": PREFIX + [I32, P, I32, P, P, P, P, I32, P],
    "bgm_causal_hmc_run_row_choice": PREFIX + [I32, P, I32, P, P, P, P, P, F32, I32, P],
    "bgm_causal_hmc_run_group_effects": PREFIX + [I32, P, I32, P, P],
}


def test_the_argtypes_of_the_seven_entry_points_are_todays():
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("bgm_causal_hmc_run")) == sorted(ARGTYPES)
    for name, want in ARGTYPES.items():
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args == want, name
        assert args is not _lib.SYMBOLS["bgm_causal_hmc_run"][1] or name == "bgm_causal_hmc_run"      # no list shared between two
