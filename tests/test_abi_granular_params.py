"""The entry points that change a granular voice's parameters and loop range while it plays (include/phonic_gpu.h): exported on both handles, the
descriptor query equal to Sampler::granular_parameters() (tests/golden/granular_params.json, hand-copied from the reference's
src/generator/sampler.rs:219-280), every argument error that needs no device, the layout of pg_grain_state unchanged, and the header and
INTEGRATION.md in step."""
import ctypes as C
import json
import math
import os
import re

from phonic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["set_voice_granular_parameter", "set_voice_grain_loop_range", "voice_granular_params"]
SYMBOLS = ["pg_granular_param_count", "pg_granular_param"] + ["pg_graph_" + c for c in CALLS] + ["pg_sharded_" + c for c in CALLS]
SCALINGS = {"linear": 0, "exponential": 1}


def test_symbols_are_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_descriptor_query_equals_the_fixture():
    lib = _capi.load()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "granular_params.json")))
    assert lib.pg_granular_param_count() == len(golden) == 10
    descs = _capi.granular_param_descs()
    assert tuple(d["id"] for d in descs) == _capi.GRANULAR_PARAM_IDS == tuple(g["id"] for g in golden)
    for g, d in zip(golden, descs):
        assert d["name"] == g["name"]
        if g["type"] == "enum":
            assert (d["type"], d["n_values"], d["min"], d["max"], d["default"], d["scaling"]) == (1, len(g["values"]), 0.0, float(len(g["values"]) - 1), float(g["default"]), 0)
        else:
            assert (d["type"], d["n_values"], d["min"], d["max"], d["default"]) == (0, 0, g["min"], g["max"], g["default"])
            assert d["scaling"] == SCALINGS[g["scaling"]] and (g["scaling"] == "linear" or d["scaling_arg0"] == g["factor"])
    d = _capi.ParamDesc()
    assert lib.pg_granular_param(10, C.byref(d)) == _capi.PG_ERR_NOT_FOUND and lib.pg_granular_param(-1, C.byref(d)) == _capi.PG_ERR_NOT_FOUND
    assert lib.pg_granular_param(0, None) == _capi.PG_ERR_PARAMETER
    assert _capi.GRAIN_WINDOWS[0] == "Hann" and len(_capi.GRAIN_WINDOWS) == 8


def test_argument_errors_without_a_device():
    """No graph exists (the handle is null): a parameter error comes before the handle is looked at, and valid arguments report the null handle."""
    lib = _capi.load()
    fcc = _capi.fourcc
    for prefix in ("pg_graph_", "pg_sharded_"):
        f = lambda name: getattr(lib, prefix + name)
        for args in ((fcc("GXYZ"), 0.5, 0), (fcc("gsiz"), 0.5, 1), (0, 0.5, 0), (fcc("ML1R"), 1.0, 0), (fcc("GSIZ"), math.nan, 0), (fcc("GWND"), math.nan, 1), (fcc("GOVM"), math.nan, 0)):
            assert f("set_voice_granular_parameter")(None, 0, *args, 0) == _capi.PG_ERR_PARAMETER, args
            assert b"null" not in lib.pg_last_error_message(), args
        for args in ((1, -0.1, 0.5), (1, 0.2, 1.5), (1, math.nan, 0.5), (1, 0.5, math.nan), (1, math.inf, 0.5)):
            assert f("set_voice_grain_loop_range")(None, 0, *args, 0) == _capi.PG_ERR_PARAMETER, args
            assert b"null" not in lib.pg_last_error_message(), args
        for id4 in _capi.GRANULAR_PARAM_IDS:          # valid arguments (out-of-range values are clamped, not refused): the null handle errors
            for args in ((0.5, 0), (0.5, 1), (1.0e9, 0), (-5.0, 1)):
                assert f("set_voice_granular_parameter")(None, 0, fcc(id4), *args, 0) == _capi.PG_ERR_PARAMETER and b"null" in lib.pg_last_error_message(), (id4, args)
        for args in ((1, 0.0, 1.0), (1, 0.75, 0.25), (1, 0.5, 0.5), (0, 0.0, 0.0), (0, math.nan, 7.0)):   # (what pg_granular_params_check accepts; no loop range: the points are not looked at)
            assert f("set_voice_grain_loop_range")(None, 0, *args, 0) == _capi.PG_ERR_PARAMETER and b"null" in lib.pg_last_error_message(), args
        p = _capi.GranularParams()
        assert f("voice_granular_params")(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_voice_granular_params(None, 0, None) == _capi.PG_ERR_PARAMETER


def test_loop_range_check_is_pg_granular_params_check():
    lib = _capi.load()
    for lr in ((0.0, 1.0), (0.75, 0.25), (-0.1, 0.5), (0.2, 1.5), (math.nan, 0.5)):
        ok = lib.pg_granular_params_check(C.byref(_capi.granular_params(loop_range=lr))) == _capi.PG_OK
        rc = lib.pg_graph_set_voice_grain_loop_range(None, 0, 1, lr[0], lr[1], 0)
        assert rc == _capi.PG_ERR_PARAMETER and (b"null" in lib.pg_last_error_message()) == ok, lr


def test_grain_state_layout_is_unchanged():
    """`reserved` became `overlap_mode`: same offset, same size."""
    assert _capi.GrainState.overlap_mode.offset == 20 and _capi.GrainState.overlap_mode.size == 4 and _capi.GrainState.speed.offset == 24
    assert C.sizeof(_capi.GrainState) == 24 + 8 + 8 + 32 + 100 * C.sizeof(_capi.GrainSlot) and C.sizeof(_capi.GrainSlot) == 64
    assert C.sizeof(_capi.GranularParams) == 56 + 32


def test_header_and_integration_md_agree():
    header = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert re.search(r"pub fn " + s + r"\s*\(", doc), s
    # parameter changes left both out-of-scope lists; what stays out of scope is named
    assert "changing granular parameters after the voice has started" not in header and "parameters themselves after the voice has started" not in header
    scope = header[header.index("Granular playback voices"):header.index("typedef struct pg_granular_params")]
    for phrase in ("OUT OF SCOPE", "voice-stealing", "playback-position status events", "base transpose, finetune, volume and panning", "AHDSR parameter changes on a running envelope"):
        assert phrase in scope, phrase
    for phrase in ("a binding loops over its voices", "set_granular_parameter", "GrainPool::set_loop_range", "Exponential(2.0)"):
        assert phrase in header, phrase
    assert "int32_t overlap_mode;      /*" in header and "pg_graph_set_voice_granular_parameter" in doc and "SetLoopRange" in doc
