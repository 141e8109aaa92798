"""The granular samplers' part of the C ABI without a device: struct sizes and offsets against the ctypes mirror, defaults and checks, the
state-derivation rule against the model's, and the refusals that are decided before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import granular_sampler_model as G
from phonic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"pg_granular_sampler_options": (_capi.GranularSamplerOptions, ["params", "modulation", "rng_states"])}


def test_struct_sizes_and_offsets_match_the_ctypes_mirror(tmp_path):
    """A C program prints sizeof and offsetof of the header's struct; the ctypes mirror must agree."""
    cc = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(cc):
        cc = "cc"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "phonic_gpu.h"', "int main(void) {"]
    for name, (_, fields) in FIELDS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for f in fields:
            lines.append(f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, (cls, fields) in FIELDS.items():
        assert int(got[name]) == C.sizeof(cls)
        for f in fields:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)


def test_defaults_and_checks():
    lib = _capi.load()
    o = _capi.GranularSamplerOptions()
    lib.pg_granular_sampler_options_default(C.byref(o))
    assert not o.modulation and not o.rng_states
    assert (o.params.size, o.params.density, o.params.window, o.params.position) == (100.0, 10.0, 2, 0.5)   # GranularParameters::default()
    assert lib.pg_granular_sampler_options_check(C.byref(o)) == _capi.PG_OK
    assert lib.pg_granular_sampler_options_check(None) == _capi.PG_ERR_PARAMETER
    o.params.size = 0.5
    assert lib.pg_granular_sampler_options_check(C.byref(o)) == _capi.PG_ERR_PARAMETER and b"Grain size" in lib.pg_last_error_message()
    o.params.size = 5.0
    bad = _capi.modulation_params(routes=[(0, 0, 0.5, True)])
    bad.routes[1][1].amount = 2.0
    o = _capi.granular_sampler_options(o.params, bad)
    assert lib.pg_granular_sampler_options_check(C.byref(o)) == _capi.PG_ERR_PARAMETER
    o = _capi.granular_sampler_options(o.params, _capi.modulation_params(routes=[(0, 0, 0.5, True)]), [((1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12))])
    assert lib.pg_granular_sampler_options_check(C.byref(o)) == _capi.PG_OK and o.rng_states[4] == 5


def test_the_state_rule_is_the_models():
    given = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111222233334444, 0x5555666677778888)
    seen = set()
    for base in (None, given):
        for slot in (0, 1, 31, 32, 63):
            for gen in range(3):
                s = _capi.granular_sampler_rng_state(base, slot, gen)
                assert s == G.derive_state(base, slot, gen)
                seen.add(s)
    assert len(seen) == 2 * 5 * 3


def test_refusals_without_a_device():
    lib = _capi.load()
    go = _capi.granular_sampler_options()
    so = _capi.sampler_options()
    st, ms, gp = _capi.GrainState(), _capi.ModulationState(), _capi.GranularParams()
    # a null handle: after the argument checks
    assert lib.pg_graph_add_granular_sampler(None, 1, 0, C.byref(so), C.byref(go)) == -_capi.PG_ERR_PARAMETER and b"handle is null" in lib.pg_last_error_message()
    assert lib.pg_graph_add_granular_sampler(None, 1, 0, C.byref(so), None) == -_capi.PG_ERR_PARAMETER and b"options" in lib.pg_last_error_message()
    so.voice_count = 65
    assert lib.pg_graph_add_granular_sampler(None, 1, 0, C.byref(so), C.byref(go)) == -_capi.PG_ERR_PARAMETER and b"voice count" in lib.pg_last_error_message()
    f = _capi.fourcc
    assert lib.pg_graph_sampler_set_granular_parameter(None, 0, f("GSIZ"), 5.0, 0, 0) == _capi.PG_ERR_PARAMETER and b"handle is null" in lib.pg_last_error_message()
    assert lib.pg_graph_sampler_set_granular_parameter(None, 0, f("zzzz"), 5.0, 0, 0) == _capi.PG_ERR_PARAMETER and b"unknown" in lib.pg_last_error_message()
    assert lib.pg_graph_sampler_set_granular_parameter(None, 0, f("GSIZ"), float("nan"), 0, 0) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_sampler_voice_grain_state(None, 0, 0, C.byref(st)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_sampler_voice_modulation_state(None, 0, 0, C.byref(ms)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_sampler_granular_params(None, 0, C.byref(gp)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_sampler_granular_params(None, 0, None) == _capi.PG_ERR_PARAMETER


def test_header_says_what_is_out_of_scope():
    text = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    para = text[text.index("int pg_graph_sampler_state("):text.index("typedef struct pg_granular_sampler_options")]
    para = para[para.rindex("OUT OF SCOPE"):]
    for what in ("main mixer", "sharded handle", "modulation messages", "set_loop_range while playing", "AMP_*", "playback status events", "GeneratorPlaybackOptions::volume", "54-entry"):
        assert what in para, what
    assert not re.search(r"\bpg_sharded_[a-z_]*sampler", text)
