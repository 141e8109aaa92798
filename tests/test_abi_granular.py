"""The granular entry points of include/phonic_gpu.h: exported, defaults as GranularParameters::default (src/generator/sampler/granular.rs:268-283),
every bound of GranularParameters::validate (:291-335) rejected on both sides before anything touches a graph or a device, and the header and
INTEGRATION.md in step."""
import ctypes as C
import math
import os
import re

import pytest

from phonic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pg_granular_params_default", "pg_granular_params_check", "pg_graph_add_granular_voice", "pg_graph_voice_grain_state",
           "pg_sharded_add_granular_voice", "pg_sharded_voice_grain_state"]


def test_granular_symbols_are_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_defaults():
    lib = _capi.load()
    p = _capi.GranularParams()
    C.memset(C.byref(p), 0xAB, C.sizeof(p))
    lib.pg_granular_params_default(C.byref(p))
    assert (p.overlap_mode, p.window, p.playback_direction) == (_capi.GRAIN_CLOUD, _capi.GRAIN_WINDOWS.index("Triangle"), _capi.GRAIN_FORWARD)
    assert (p.size, p.density, p.spray, p.variation, p.pan_spread, p.position, p.step) == (100.0, 10.0, 0.0, 0.0, 0.0, 0.5, 0.0)
    assert p.has_loop_range == 0 and list(p.rng_state) == [0, 0, 0, 0]
    assert lib.pg_granular_params_check(C.byref(p)) == _capi.PG_OK
    assert bytes(p) == bytes(_capi.granular_params())
    assert C.sizeof(_capi.GranularParams) == 88 and C.sizeof(_capi.GrainSlot) == 64 and C.sizeof(_capi.GrainState) == 72 + 100 * 64


BOUNDS = {"size": (1.0, 1000.0), "density": (1.0, 100.0), "spray": (0.0, 1.0), "variation": (0.0, 1.0), "pan_spread": (0.0, 1.0), "position": (0.0, 1.0),
          "step": (-4.0, 4.0)}
BAD = [{k: lo - 0.001} for k, (lo, hi) in BOUNDS.items()] + [{k: hi + 0.001} for k, (lo, hi) in BOUNDS.items()] + [{k: math.nan} for k in BOUNDS]
BAD += [dict(loop_range=(-0.01, 0.5)), dict(loop_range=(0.2, 1.01)), dict(loop_range=(1.5, 0.5)), dict(loop_range=(0.5, -0.5)), dict(window=8), dict(window=-1),
        dict(overlap_mode=2), dict(playback_direction=3)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_validation_errors_without_a_device(kw):
    """No graph exists (the handle is null): the parameter error comes before the handle is looked at."""
    lib = _capi.load()
    p = _capi.granular_params(**kw)
    assert lib.pg_granular_params_check(C.byref(p)) == _capi.PG_ERR_PARAMETER
    one = (C.c_float * 1)(0.0)
    assert lib.pg_graph_add_granular_voice(None, 0, one, 1, C.byref(p), None) == -_capi.PG_ERR_PARAMETER
    assert b"null" not in lib.pg_last_error_message()
    assert lib.pg_sharded_add_granular_voice(None, 0, one, 1, C.byref(p), None) == -_capi.PG_ERR_PARAMETER
    assert b"null" not in lib.pg_last_error_message()


def test_closed_ends_are_valid():
    lib = _capi.load()
    for kw in [{k: lo for k, (lo, hi) in BOUNDS.items()}, {k: hi for k, (lo, hi) in BOUNDS.items()}, dict(loop_range=(0.0, 1.0)), dict(loop_range=(1.0, 0.0)),
               dict(window=7, overlap_mode=1, playback_direction=2)]:
        p = _capi.granular_params(**kw)
        assert lib.pg_granular_params_check(C.byref(p)) == _capi.PG_OK
        one = (C.c_float * 1)(0.0)
        assert lib.pg_graph_add_granular_voice(None, 0, one, 1, C.byref(p), None) == -_capi.PG_ERR_PARAMETER   # the null handle is what is reported then
        assert b"null" in lib.pg_last_error_message()
    assert lib.pg_granular_params_check(None) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_add_granular_voice(None, 0, None, 0, None, None) == -_capi.PG_ERR_PARAMETER
    st = _capi.GrainState()
    assert lib.pg_graph_voice_grain_state(None, 0, C.byref(st)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_sharded_voice_grain_state(None, 0, C.byref(st)) == _capi.PG_ERR_PARAMETER


def test_header_and_integration_md_agree():
    header = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert re.search(r"pub fn " + s + r"\s*\(", doc), s
    # the out-of-scope list and the unverified-draws note are part of the contract
    for phrase in ("modulation matrix", "UNVERIFIED", "create_granular_sample_buffer", "playback-position status events"):
        assert phrase in header, phrase
    assert "granular.rs" in doc and "pg_graph_voice_grain_state" in doc
