"""The C ABI of samplers on the main mixer, without a device: the seven symbols in the header, the library, the ctypes layer and INTEGRATION.md;
the defaults and GeneratorPlaybackOptions::validate's refusals; the order in which the add calls answer — sampler options, granular options,
generator options, then the handle — and the bounds of the two timed calls, all decided before a handle is looked at or a device touched; what the
header says of the sub-mixer case and of what stays out of scope. (The refusals that need a graph — PG_ERR_STATE for a sampler in a sub-mixer —
run against the stub runtime in tests/test_host_main_sampler.py, and on the device in tests/test_gpu_main_sampler.py.)"""
import ctypes as C
import math
import os
import re

from phonic_amd import _capi, graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"pg_generator_options_default": None, "pg_generator_options_check": C.c_int, "pg_graph_add_sampler_to_main": C.c_int,
           "pg_graph_add_granular_sampler_to_main": C.c_int, "pg_graph_sampler_set_volume": C.c_int, "pg_graph_sampler_set_panning": C.c_int,
           "pg_graph_sampler_output_state": C.c_int}


def _header():
    return open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()


def _message():
    return _capi.load().pg_last_error_message().decode()


def test_the_seven_symbols_are_everywhere():
    header, integration = _header(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _capi.load()
    for name, restype in SYMBOLS.items():
        assert re.search(r"^(int|void) %s\(" % name, header, re.M), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is restype, name
        assert "pub fn %s(" % name in integration, name
    for method in ("add_sampler_to_main", "add_granular_sampler_to_main", "sampler_set_volume", "sampler_set_panning", "sampler_output_state"):
        assert callable(getattr(graph.Graph, method)), method
    assert not re.search(r"\bpg_sharded_[a-z_]*(sampler|generator)", header)   # the sharded handle stays out of scope
    # the structs as the header states them
    assert re.search(r"typedef struct pg_generator_options \{ float volume; float panning; \} pg_generator_options;", header)
    assert C.sizeof(_capi.GeneratorOptions) == 8 and C.sizeof(_capi.SamplerOutputState) == 24
    fields = re.search(r"typedef struct pg_sampler_output_state \{(.*?)\} pg_sampler_output_state;", header, re.S).group(1)
    assert re.findall(r"\b([a-z_]+)[,;]", fields) == [f for f, _ in _capi.SamplerOutputState._fields_]


def test_defaults_and_validate():
    lib = _capi.load()
    o = _capi.GeneratorOptions(-3.0, 7.0)
    lib.pg_generator_options_default(C.byref(o))
    assert (o.volume, o.panning) == (1.0, 0.0) and lib.pg_generator_options_check(C.byref(o)) == _capi.PG_OK
    lib.pg_generator_options_default(None)
    assert lib.pg_generator_options_check(None) == _capi.PG_ERR_PARAMETER
    # GeneratorPlaybackOptions::validate (generator.rs:120-140): volume < 0 or NaN; panning outside [-1, 1] or NaN — with its wording
    for volume in (-0.001, -1.0, math.nan, -math.inf):
        assert lib.pg_generator_options_check(C.byref(_capi.GeneratorOptions(volume, 0.0))) == _capi.PG_ERR_PARAMETER, volume
        assert _message().startswith("playback options 'volume' value is '"), _message()
    for panning in (-1.001, 1.5, math.nan, math.inf):
        assert lib.pg_generator_options_check(C.byref(_capi.GeneratorOptions(1.0, panning))) == _capi.PG_ERR_PARAMETER, panning
        assert _message().startswith("playback options 'panning' value is '"), _message()
    for volume, panning in ((0.0, -1.0), (15.0, 1.0), (math.inf, 0.0)):   # (validate has no upper bound on the volume)
        assert lib.pg_generator_options_check(C.byref(_capi.GeneratorOptions(volume, panning))) == _capi.PG_OK
    g = _capi.generator_options(volume=0.5)
    assert (g.volume, g.panning) == (0.5, 0.0)


def test_the_add_calls_answer_in_the_stated_order_without_a_handle():
    lib = _capi.load()
    ok, bad_voices = _capi.sampler_options(), _capi.sampler_options()
    bad_voices.voice_count = 0
    gok = _capi.granular_sampler_options(_capi.granular_params())
    gbad = _capi.granular_sampler_options(_capi.granular_params())
    gbad.params.size = 0.0
    gen_bad, gen_ok = _capi.GeneratorOptions(-1.0, 0.0), _capi.GeneratorOptions(1.0, 0.0)
    P = _capi.PG_ERR_PARAMETER
    add, gadd = lib.pg_graph_add_sampler_to_main, lib.pg_graph_add_granular_sampler_to_main
    assert add(None, 0, C.byref(bad_voices), C.byref(gen_bad)) == -P and "Invalid voice count" in _message()
    assert add(None, 0, C.byref(ok), C.byref(gen_bad)) == -P and "playback options 'volume'" in _message()
    assert add(None, 0, C.byref(ok), C.byref(gen_ok)) == -P and "graph handle is null" in _message()
    assert add(None, 0, None, None) == -P and "graph handle is null" in _message()          # null options: the defaults
    assert gadd(None, 0, C.byref(bad_voices), C.byref(gbad), C.byref(gen_bad)) == -P and "Invalid voice count" in _message()
    assert gadd(None, 0, C.byref(ok), C.byref(gbad), C.byref(gen_bad)) == -P and "Grain size" in _message()
    assert gadd(None, 0, C.byref(ok), None, C.byref(gen_bad)) == -P and "granular sampler options must not be null" in _message()
    assert gadd(None, 0, C.byref(ok), C.byref(gok), C.byref(gen_bad)) == -P and "playback options 'volume'" in _message()
    assert gadd(None, 0, C.byref(ok), C.byref(gok), C.byref(_capi.GeneratorOptions(1.0, 2.0))) == -P and "playback options 'panning'" in _message()
    assert gadd(None, 0, C.byref(ok), C.byref(gok), None) == -P and "graph handle is null" in _message()


def test_the_timed_calls_check_their_value_first():
    lib = _capi.load()
    P = _capi.PG_ERR_PARAMETER
    for volume in (-0.5, math.nan, math.inf):
        assert lib.pg_graph_sampler_set_volume(None, 0, volume, 0) == P and "Invalid volume" in _message(), volume
    for panning in (math.nan, math.inf, -math.inf):
        assert lib.pg_graph_sampler_set_panning(None, 0, panning, 0) == P and "Invalid panning" in _message(), panning
    assert lib.pg_graph_sampler_set_volume(None, 0, 0.0, 0) == P and "graph handle is null" in _message()
    assert lib.pg_graph_sampler_set_panning(None, 0, -3.0, 0) == P and "graph handle is null" in _message()   # finite: the pan law clamps it, like a note's
    st = _capi.SamplerOutputState()
    assert lib.pg_graph_sampler_output_state(None, 0, None) == P and "output is null" in _message()
    assert lib.pg_graph_sampler_output_state(None, 0, C.byref(st)) == P and "graph handle is null" in _message()


def test_the_header_documents_the_new_calls_and_what_stays_out():
    header = _header()
    para = header[header.index("/* Samplers on the MAIN mixer"):header.index("typedef struct pg_generator_options")]
    para = re.sub(r"\s*\n \*\s*", " ", para)   # (the comment's line breaks are not part of what it says)
    for what in ("GeneratorPlaybackOptions::target_mixer", "add_or_play_generator", "sampler options, granular options,", "generator options, handle, buffer, loop range",
                 "gen == NULL", "one next() per interleaved SAMPLE", "one next() per FRAME", "1e-6", "Both stand still over a write that returned 0",
                 "PG_ERR_QUEUE_FULL", "a time before the start time acts at the start time", "the LAST one sent counts", "PG_ERR_STATE: a sampler that lives in",
                 "no sum of the sampler exists to scale", "min(remaining, 4096)", "sampler.rs:974-981"):
        assert what in para, what
    out = para[para.rindex("OUT OF SCOPE"):]
    for what in ("sharded handle", "sub-mixer", "measure_cpu_load", "playback", "FunDSP"):
        assert what in out, what
    # the two existing entry points still refuse the main mixer and say where it went
    first = header[header.index("The Sampler generator's note layer"):header.index("#define PG_SAMPLER_MAX_VOICES")]
    assert "pg_graph_add_sampler_to_main" in first[first.rindex("OUT OF SCOPE"):]
    # the library's wording for a sampler in a sub-mixer is the header's reason
    src = open(os.path.join(ROOT, "phonic_amd", "csrc", "pg_sampler.hip")).read()
    assert src.count("lives in a sub-mixer: its pool is summed there source by source") == 2
