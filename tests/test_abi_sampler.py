"""The sampler's entry points as far as they go without a device: option defaults and every pg_sampler_options_check error, the four base
parameter descriptors against the reference's constants (src/generator/sampler.rs:98-127), and the argument errors that are answered before
the handle is looked at."""
import ctypes as C
import math

import pytest

from phonic_amd import _capi
from phonic_amd.graph import sampler_parameters


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def _err(lib):
    return lib.pg_last_error_message().decode()


def test_option_defaults(lib):
    o = _capi.SamplerOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib.pg_sampler_options_default(C.byref(o))
    assert (o.voice_count, o.has_envelope, o.has_loop_range, o.transient, o.loop_start, o.loop_end, o.start_time) == (8, 0, 0, 0, 0, 0, 0)
    d = _capi.ahdsr_params()   # AhdsrParameters::default
    assert [getattr(o.envelope, n) for n, _ in _capi.AhdsrParams._fields_] == [getattr(d, n) for n, _ in _capi.AhdsrParams._fields_]
    assert lib.pg_sampler_options_check(C.byref(o)) == _capi.PG_OK
    lib.pg_sampler_options_default(None)   # a null pointer is left alone
    py = _capi.sampler_options()
    assert bytes(py) == bytes(o)


@pytest.mark.parametrize("change, text", [
    (dict(voice_count=0), "voice count"),
    (dict(voice_count=65), "voice count"),
    (dict(envelope=dict(attack_s=-1.0)), "attack time"),
    (dict(envelope=dict(hold_s=math.inf)), "hold time"),
    (dict(envelope=dict(decay_s=math.nan)), "decay time"),
    (dict(envelope=dict(release_s=-0.5)), "release time"),
    (dict(envelope=dict(attack_scaling=1.5)), "attack scaling"),
    (dict(envelope=dict(decay_scaling=-2.0)), "decay scaling"),
    (dict(envelope=dict(release_scaling=math.nan)), "release scaling"),
    (dict(envelope=dict(sustain_level=1.01)), "sustain level"),
    (dict(loop_range=(10, 10)), "loop range"),
    (dict(loop_range=(11, 10)), "loop range"),
])
def test_option_errors(lib, change, text):
    o = _capi.sampler_options(**change)
    assert lib.pg_sampler_options_check(C.byref(o)) == _capi.PG_ERR_PARAMETER
    assert text in _err(lib).lower()
    assert lib.pg_graph_add_sampler(None, 1, 0, C.byref(o)) == -_capi.PG_ERR_PARAMETER and text in _err(lib).lower()   # before the handle


def test_option_check_accepts_the_edges_and_refuses_null(lib):
    for kw in (dict(voice_count=1), dict(voice_count=64), dict(envelope=dict(attack_s=0.0, hold_s=0.0, decay_s=0.0, release_s=0.0, sustain_level=0.0)),
               dict(envelope=dict(attack_scaling=-1.0, decay_scaling=1.0, release_scaling=-1.0, sustain_level=1.0)), dict(loop_range=(0, 1)), dict(transient=True)):
        o = _capi.sampler_options(**kw)
        assert lib.pg_sampler_options_check(C.byref(o)) == _capi.PG_OK, kw
    bad = _capi.sampler_options(envelope=dict(attack_s=-1.0))
    bad.has_envelope = 0   # envelope values count only when the sampler has one
    assert lib.pg_sampler_options_check(C.byref(bad)) == _capi.PG_OK
    assert lib.pg_sampler_options_check(None) == _capi.PG_ERR_PARAMETER and "null" in _err(lib)


def test_descriptors_match_the_reference_constants(lib):
    f = _capi.fourcc
    p = sampler_parameters()
    assert lib.pg_sampler_param_count() == 4
    assert [d["fourcc"] for d in p] == [f("STRN"), f("SFTN"), f("SVOL"), f("SPAN")]   # Sampler::base_parameters() order
    assert [d["name"] for d in p] == ["Transpose", "Finetune", "Volume", "Panning"]
    PG_PARAM_FLOAT, PG_PARAM_INTEGER = 0, 3
    assert [d["type"] for d in p] == [PG_PARAM_INTEGER, PG_PARAM_INTEGER, PG_PARAM_FLOAT, PG_PARAM_FLOAT]
    assert [(d["min"], d["max"], d["default"]) for d in p[:2]] == [(-48.0, 48.0, 0.0), (-100.0, 100.0, 0.0)]
    vol, pan = p[2], p[3]
    assert abs(vol["min"] - 0.000001) < 1e-12 and abs(vol["max"] - 15.848932) < 1e-6 and vol["default"] == 1.0
    assert vol["scaling"] == 2 and vol["scaling_args"] == (-60.0, 24.0)   # ParameterScaling::Decibel(-60, 24)
    assert (pan["min"], pan["max"], pan["default"], pan["scaling"]) == (-1.0, 1.0, 0.0, 0)
    assert all(d["scaling"] == 0 for d in p[:2]) and all(d["n_values"] == 0 for d in p)
    d = _capi.ParamDesc()
    assert lib.pg_sampler_param(4, C.byref(d)) == _capi.PG_ERR_NOT_FOUND and lib.pg_sampler_param(-1, C.byref(d)) == _capi.PG_ERR_NOT_FOUND
    assert lib.pg_sampler_param(0, None) == _capi.PG_ERR_PARAMETER


def test_argument_errors_come_before_the_handle(lib):
    E = _capi.PG_ERR_PARAMETER
    nan, inf = math.nan, math.inf
    for vol, pan, text in ((-0.1, 0.0, "volume"), (nan, 0.0, "volume"), (inf, 0.0, "volume"), (1.0, nan, "panning"), (1.0, inf, "panning")):
        assert lib.pg_graph_sampler_note_on(None, 0, 60, vol, pan, 0) == -E and text in _err(lib)
    assert lib.pg_graph_sampler_note_on(None, 0, 60, 1.0, 0.0, 0) == -E and "handle is null" in _err(lib)
    for speed in (0.0, -1.0, nan, inf):
        assert lib.pg_graph_sampler_set_note_speed(None, 0, 1, speed, 0.0, 0) == E and "speed" in _err(lib)
    assert lib.pg_graph_sampler_set_note_volume(None, 0, 1, -1.0, 0) == E and "volume" in _err(lib)
    assert lib.pg_graph_sampler_set_note_panning(None, 0, 1, nan, 0) == E and "panning" in _err(lib)
    f = _capi.fourcc
    assert lib.pg_graph_sampler_set_parameter(None, 0, f("GSIZ"), 1.0, 0, 0) == E and "unknown" in _err(lib)
    assert lib.pg_graph_sampler_set_parameter(None, 0, f("SVOL"), nan, 0, 0) == E and "not a number" in _err(lib)
    for n in (-0.01, 1.01):   # player/handles/generator.rs:342-348
        assert lib.pg_graph_sampler_set_parameter(None, 0, f("STRN"), n, 1, 0) == E and "normalized" in _err(lib)
    assert lib.pg_graph_sampler_set_parameter(None, 0, f("STRN"), 60.0, 0, 0) == E and "handle is null" in _err(lib)   # a raw value is clamped, not refused
    for call in (lib.pg_graph_sampler_note_off, ):
        assert call(None, 0, 1, 0) == E and "handle is null" in _err(lib)
    for call in (lib.pg_graph_sampler_all_notes_off, lib.pg_graph_sampler_stop):
        assert call(None, 0, 0) == E and "handle is null" in _err(lib)
    assert lib.pg_graph_remove_sampler(None, 0) == E and "handle is null" in _err(lib)
    assert lib.pg_graph_sampler_state(None, 0, None) == E and "output" in _err(lib)
    st = _capi.SamplerState()
    assert lib.pg_graph_sampler_state(None, 0, C.byref(st)) == E and "handle is null" in _err(lib)
    o = _capi.sampler_options()
    assert lib.pg_graph_add_sampler(None, 1, 0, C.byref(o)) == -E and "handle is null" in _err(lib)
    assert lib.pg_graph_add_sampler(None, 1, 0, None) == -E and "handle is null" in _err(lib)   # null options = the defaults


def test_struct_sizes_match_the_header():
    assert C.sizeof(_capi.SamplerOptions) == 4 + 4 + 32 + 4 + 4 + 8 + 8 + 8
    assert C.sizeof(_capi.SamplerSlotState) == 32
    assert C.sizeof(_capi.SamplerState) == 32 + 64 * 32
