"""The modulation-matrix entry points of include/phonic_gpu.h: exported, the defaults of Sampler::modulation_config (src/generator/sampler.rs:369-427),
the errors of ModulationState::set_modulation (src/modulation/state.rs:195-201) on both handles before anything touches a graph or a device, and the
header and INTEGRATION.md in step."""
import ctypes as C
import math
import os
import re

import pytest

from phonic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["set_voice_modulation_matrix", "set_voice_modulation", "clear_voice_modulation", "set_voice_lfo_rate", "set_voice_lfo_waveform", "voice_modulation_state"]
SYMBOLS = ["pg_modulation_params_default", "pg_modulation_params_check"] + ["pg_graph_" + c for c in CALLS] + ["pg_sharded_" + c for c in CALLS]


def test_modulation_symbols_are_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_defaults():
    lib = _capi.load()
    p = _capi.ModulationParams()
    C.memset(C.byref(p), 0xAB, C.sizeof(p))
    lib.pg_modulation_params_default(C.byref(p))
    assert (p.lfo[0].rate_hz, p.lfo[0].waveform, p.lfo[1].rate_hz, p.lfo[1].waveform) == (1.0, _capi.LFO_WAVEFORMS.index("Sine"), 2.0, _capi.LFO_WAVEFORMS.index("Triangle"))
    assert p.velocity == 1.0 and p.note == 60
    assert all(list(p.lfo[l].rng_state) == [0, 0, 0, 0] for l in range(2))
    assert all(p.routes[s][t].amount == 0.0 and p.routes[s][t].bipolar == 0 for s in range(_capi.MOD_SOURCES) for t in range(_capi.MOD_TARGETS))
    assert lib.pg_modulation_params_check(C.byref(p)) == _capi.PG_OK
    assert bytes(p) == bytes(_capi.modulation_params())
    assert C.sizeof(_capi.ModLfo) == 40 and C.sizeof(_capi.ModulationParams) == 80 + 8 + 4 * 7 * 8 and C.sizeof(_capi.ModulationState) == 2 * 56 + 8 + 4 * 7 * 8 + 32
    assert (_capi.MOD_SOURCES, _capi.MOD_TARGETS) == (4, 7) and len(_capi.MOD_SOURCE_NAMES) == 4 and len(_capi.MOD_TARGET_NAMES) == 7


BAD = [dict(routes=[(0, 0, 1.5, 1)]), dict(routes=[(3, 6, -1.001, 0)]), dict(routes=[(1, 2, math.nan, 1)]), dict(waveforms=(7, None)), dict(waveforms=(None, -1)),
       dict(rates=(math.nan, None)), dict(velocity=1.01), dict(velocity=-0.01), dict(velocity=math.nan), dict(note=128), dict(note=-1)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_validation_errors_without_a_device(kw):
    """No graph exists (the handle is null): the parameter error comes before the handle is looked at."""
    lib = _capi.load()
    p = _capi.modulation_params(**kw)
    assert lib.pg_modulation_params_check(C.byref(p)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_set_voice_modulation_matrix(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER
    assert b"null" not in lib.pg_last_error_message()
    assert lib.pg_sharded_set_voice_modulation_matrix(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER
    assert b"null" not in lib.pg_last_error_message()


def test_closed_ends_and_clamped_rates_are_valid():
    lib = _capi.load()
    for kw in [dict(routes=[(0, 0, 1.0, 1), (3, 6, -1.0, 0)]), dict(rates=(0.0, 1000.0)), dict(rates=(-5.0, math.inf)), dict(waveforms=(6, 0)), dict(velocity=0.0, note=0),
               dict(velocity=1.0, note=127)]:
        p = _capi.modulation_params(**kw)
        assert lib.pg_modulation_params_check(C.byref(p)) == _capi.PG_OK, kw
        assert lib.pg_graph_set_voice_modulation_matrix(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER   # the null handle is what is reported then
        assert b"null" in lib.pg_last_error_message()
    assert lib.pg_modulation_params_check(None) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_set_voice_modulation_matrix(None, 0, None) == _capi.PG_ERR_PARAMETER


def test_timed_calls_check_their_arguments_and_the_handle():
    lib = _capi.load()
    for prefix in ("pg_graph_", "pg_sharded_"):
        f = lambda name: getattr(lib, prefix + name)
        for args in ((4, 0, 0.5, 1), (-1, 0, 0.5, 1), (0, 7, 0.5, 1), (0, -1, 0.5, 0), (0, 0, 1.5, 1), (0, 0, -1.5, 1), (0, 0, math.nan, 0)):
            assert f("set_voice_modulation")(None, 0, *args, 0) == _capi.PG_ERR_PARAMETER
            assert b"null" not in lib.pg_last_error_message(), args
        assert f("clear_voice_modulation")(None, 0, 4, 0, 0) == _capi.PG_ERR_PARAMETER and b"null" not in lib.pg_last_error_message()
        assert f("set_voice_lfo_rate")(None, 0, 2, 1.0, 0) == _capi.PG_ERR_PARAMETER and b"null" not in lib.pg_last_error_message()
        assert f("set_voice_lfo_rate")(None, 0, 0, math.nan, 0) == _capi.PG_ERR_PARAMETER and b"null" not in lib.pg_last_error_message()
        assert f("set_voice_lfo_waveform")(None, 0, 0, 7, 0) == _capi.PG_ERR_PARAMETER and b"null" not in lib.pg_last_error_message()
        assert f("set_voice_lfo_waveform")(None, 0, -1, 0, 0) == _capi.PG_ERR_PARAMETER and b"null" not in lib.pg_last_error_message()
        # valid arguments: the null handle errors
        assert f("set_voice_modulation")(None, 0, 0, 0, 0.5, 1, 0) == _capi.PG_ERR_PARAMETER and b"null" in lib.pg_last_error_message()
        assert f("clear_voice_modulation")(None, 0, 3, 6, 0) == _capi.PG_ERR_PARAMETER and b"null" in lib.pg_last_error_message()
        assert f("set_voice_lfo_rate")(None, 0, 1, 100.0, 0) == _capi.PG_ERR_PARAMETER and b"null" in lib.pg_last_error_message()
        assert f("set_voice_lfo_waveform")(None, 0, 1, 6, 0) == _capi.PG_ERR_PARAMETER and b"null" in lib.pg_last_error_message()
        st = _capi.ModulationState()
        assert f("voice_modulation_state")(None, 0, C.byref(st)) == _capi.PG_ERR_PARAMETER


def test_header_and_integration_md_agree():
    header = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert re.search(r"pub fn " + s + r"\s*\(", doc), s
    # the matrix left the granular voices' out-of-scope list; what stays out of scope is named
    scope = header[header.index("Granular playback voices"):header.index("typedef struct pg_granular_params")]
    assert "OUT OF SCOPE: the modulation matrix" not in scope and "OUT OF SCOPE" in scope
    for phrase in ("matrix.rs", "lfo.rs", "Envelope modulation sources".lower(), "FunDSP", "UNVERIFIED", "a binding loops over its voices"):
        assert phrase in header, phrase
    assert "set_modulation" in doc and "pg_graph_set_voice_modulation_matrix" in doc
