"""The C ABI of the sampler messages that change every voice while notes sound (envelope parameters, modulation, loop range), without a device:
the nine symbols in the header, the library, the ctypes layer and INTEGRATION.md; the five descriptors against the reference's constants; the
layout of pg_sampler_envelope_state against its ctypes mirror; every refusal that is decided before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sampler_live_model as L
from phonic_amd import _capi, graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pg_sampler_envelope_param_count", "pg_sampler_envelope_param", "pg_graph_sampler_set_envelope_parameter", "pg_graph_sampler_envelope_params",
           "pg_graph_sampler_set_modulation", "pg_graph_sampler_clear_modulation", "pg_graph_sampler_set_lfo_rate", "pg_graph_sampler_set_lfo_waveform",
           "pg_graph_sampler_set_loop_range"]
ENV_FIELDS = ["attack_rate", "decay_rate", "release_rate", "sustain_level", "hold_samples", "attack_scaling", "decay_scaling", "release_scaling", "zero_times"]
PG_SCALE_EXPONENTIAL = 1


def _header():
    return open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()


def test_the_nine_symbols_are_everywhere():
    header, integration = _header(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _capi.load()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        fn = getattr(lib, name)                                   # the library exports it ...
        assert fn.argtypes is not None and fn.restype is C.c_int, name   # ... and _capi has declared it
        assert "pub fn %s(" % name in integration, name
    # behind the granular sampler's options, next to pg_graph_sampler_set_granular_parameter
    assert header.index("int pg_graph_sampler_set_envelope_parameter(") > header.index("typedef struct pg_granular_sampler_options")
    for method in ("sampler_set_envelope_parameter", "sampler_envelope_params", "sampler_set_modulation", "sampler_clear_modulation", "sampler_set_lfo_rate",
                   "sampler_set_lfo_waveform", "sampler_set_loop_range"):
        assert callable(getattr(graph.Graph, method)), method
    assert not re.search(r"\bpg_sharded_[a-z_]*sampler", header)   # no sharded entry points


def test_descriptors_are_the_references():
    """Sampler::envelope_parameters() (sampler.rs:130-181): times 0..=10 s, Exponential(2.0), defaults 0.001 / 0.75 / 0.5 / 1.0; sustain 0..=1, linear, 0.75."""
    lib = _capi.load()
    assert lib.pg_sampler_envelope_param_count() == 5
    descs = graph.sampler_envelope_parameters()
    assert len(descs) == 5
    for d, (fourcc, name, lo, hi, default, exponent) in zip(descs, L.ENV_DESCRIPTORS):
        assert d["fourcc"] == _capi.fourcc(fourcc) and d["name"] == name and d["type"] == 0   # PG_PARAM_FLOAT
        assert (d["min"], d["max"]) == (lo, hi) and d["default"] == pytest.approx(default, rel=1e-7)
        if exponent is None:
            assert d["scaling"] == 0
        else:
            assert d["scaling"] == PG_SCALE_EXPONENTIAL and d["scaling_args"][0] == exponent
    assert [d["fourcc"] for d in descs] == [_capi.fourcc(x) for x in _capi.SAMPLER_ENVELOPE_PARAM_IDS] == [_capi.fourcc(x) for x in ("AATK", "AHLD", "ADCY", "ASTN", "AREL")]
    d = _capi.ParamDesc()
    assert lib.pg_sampler_envelope_param(5, C.byref(d)) == _capi.PG_ERR_NOT_FOUND and lib.pg_sampler_envelope_param(-1, C.byref(d)) == _capi.PG_ERR_NOT_FOUND
    assert lib.pg_sampler_envelope_param(0, None) == _capi.PG_ERR_PARAMETER
    # disjoint tables: the base parameters' call does not take the envelope's ids, nor this one the base ids
    base = {d["fourcc"] for d in graph.sampler_parameters()}
    assert not base & {d["fourcc"] for d in descs}


def test_envelope_state_layout_matches_the_ctypes_mirror(tmp_path):
    cc = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(cc):
        cc = "cc"
    name = "pg_sampler_envelope_state"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "phonic_gpu.h"', "int main(void) {", f'  printf("{name} %zu\\n", sizeof({name}));']
    lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in ENV_FIELDS]
    lines += ["  return 0;", "}"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[name]) == C.sizeof(_capi.SamplerEnvelopeState) == 36
    assert [f for f, _ in _capi.SamplerEnvelopeState._fields_] == ENV_FIELDS
    for f in ENV_FIELDS:
        assert int(got[f"{name}.{f}"]) == getattr(_capi.SamplerEnvelopeState, f).offset, f


def test_refusals_without_a_device():
    lib = _capi.load()
    f, P, msg = _capi.fourcc, _capi.PG_ERR_PARAMETER, lib.pg_last_error_message
    nan = float("nan")
    # envelope parameters: an unknown id (the base parameters' among them), a NaN; a null handle last
    assert lib.pg_graph_sampler_set_envelope_parameter(None, 0, f("zzzz"), 0.5, 0, 0) == P and b"unknown envelope parameter" in msg()
    assert lib.pg_graph_sampler_set_envelope_parameter(None, 0, f("SVOL"), 0.5, 0, 0) == P and b"unknown envelope parameter" in msg()
    assert lib.pg_graph_sampler_set_envelope_parameter(None, 0, f("AATK"), nan, 0, 0) == P and b"not a number" in msg()
    assert lib.pg_graph_sampler_set_envelope_parameter(None, 0, f("ASTN"), nan, 1, 0) == P and b"not a number" in msg()
    for fourcc in _capi.SAMPLER_ENVELOPE_PARAM_IDS:
        assert lib.pg_graph_sampler_set_envelope_parameter(None, 0, f(fourcc), 0.5, 0, 0) == P and b"handle is null" in msg()
        assert lib.pg_graph_sampler_set_envelope_parameter(None, 0, f(fourcc), 7.0, 1, 0) == P and b"handle is null" in msg()   # a normalized value is clamped, not refused
        assert lib.pg_graph_sampler_set_parameter(None, 0, f(fourcc), 0.5, 0, 0) == P and b"unknown sampler parameter" in msg()  # the base call keeps refusing AMP_*
    st = _capi.SamplerEnvelopeState()
    assert lib.pg_graph_sampler_envelope_params(None, 0, 0, None) == P and b"output is null" in msg()
    assert lib.pg_graph_sampler_envelope_params(None, 0, 0, C.byref(st)) == P and b"handle is null" in msg()
    # modulation: source / target / LFO / waveform out of range, an amount outside [-1, 1] or NaN
    for source, target in ((-1, 0), (4, 0), (0, -1), (0, 7)):
        assert lib.pg_graph_sampler_set_modulation(None, 0, source, target, 0.5, 0, 0) == P and b"Unknown modulation" in msg()
        assert lib.pg_graph_sampler_clear_modulation(None, 0, source, target, 0) == P and b"Unknown modulation" in msg()
    for amount in (1.5, -1.0001, nan):
        assert lib.pg_graph_sampler_set_modulation(None, 0, 0, 0, amount, 0, 0) == P and b"amount" in msg()
    assert lib.pg_graph_sampler_set_modulation(None, 0, 3, 6, -1.0, 1, 0) == P and b"handle is null" in msg()
    assert lib.pg_graph_sampler_clear_modulation(None, 0, 3, 6, 0) == P and b"handle is null" in msg()
    for lfo in (-1, 2):
        assert lib.pg_graph_sampler_set_lfo_rate(None, 0, lfo, 1.0, 0) == P and b"LFO index" in msg()
        assert lib.pg_graph_sampler_set_lfo_waveform(None, 0, lfo, 0, 0) == P and b"LFO index" in msg()
    assert lib.pg_graph_sampler_set_lfo_rate(None, 0, 0, nan, 0) == P and b"not a number" in msg()
    assert lib.pg_graph_sampler_set_lfo_rate(None, 0, 1, 100.0, 0) == P and b"handle is null" in msg()      # a rate is clamped, not refused
    for waveform in (-1, 7):
        assert lib.pg_graph_sampler_set_lfo_waveform(None, 0, 0, waveform, 0) == P and b"waveform" in msg()
    assert lib.pg_graph_sampler_set_lfo_waveform(None, 0, 1, 6, 0) == P and b"handle is null" in msg()
    # loop range: inverted or empty
    assert lib.pg_graph_sampler_set_loop_range(None, 0, 1, 10, 5, 0) == P and b"Invalid loop range" in msg()
    assert lib.pg_graph_sampler_set_loop_range(None, 0, 1, 7, 7, 0) == P and b"Invalid loop range" in msg()
    assert lib.pg_graph_sampler_set_loop_range(None, 0, 1, 5, 10, 0) == P and b"handle is null" in msg()
    assert lib.pg_graph_sampler_set_loop_range(None, 0, 0, 10, 5, 0) == P and b"handle is null" in msg()      # None: the numbers are not read
