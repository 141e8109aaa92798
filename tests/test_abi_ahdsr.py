"""The envelope entry points of include/phonic_gpu.h: exported, defaults as AhdsrParameters::default (src/utils/ahdsr.rs:348-359), and the
reference's parameter errors (ahdsr.rs:143-152, :179-188, :224-233, :259-268) returned before anything touches a graph or a device."""
import ctypes as C
import math

import pytest

from phonic_amd import _capi

SYMBOLS = ["pg_ahdsr_params_default", "pg_graph_set_voice_envelope", "pg_graph_release_voice", "pg_graph_voice_envelope_stage",
           "pg_sharded_set_voice_envelope", "pg_sharded_release_voice", "pg_sharded_voice_envelope_stage"]


def test_envelope_symbols_are_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_defaults():
    lib = _capi.load()
    p = _capi.AhdsrParams()
    lib.pg_ahdsr_params_default(C.byref(p))
    f = lambda x: C.c_float(x).value
    assert (p.attack_s, p.hold_s, p.decay_s, p.sustain_level, p.release_s) == (f(0.010), 1.0, 0.5, 0.75, 1.0)
    assert (p.attack_scaling, p.decay_scaling, p.release_scaling) == (0.0, 0.0, 0.0)
    q = _capi.ahdsr_params()
    assert bytes(p) == bytes(q)
    assert C.sizeof(_capi.AhdsrParams) == 32


BAD = [dict(attack_scaling=1.5), dict(attack_scaling=-1.01), dict(decay_scaling=2.0), dict(decay_scaling=-1.5), dict(release_scaling=1.0001),
       dict(release_scaling=-7.0), dict(attack_scaling=math.nan), dict(sustain_level=1.1), dict(sustain_level=-0.1), dict(sustain_level=math.nan),
       dict(attack_s=-0.01), dict(hold_s=-1.0), dict(decay_s=-1e-9), dict(release_s=-2.0),
       dict(attack_s=math.inf), dict(hold_s=math.nan), dict(decay_s=math.inf), dict(release_s=math.nan)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_validation_errors_without_a_device(kw):
    """No graph exists (the handle is null): the call must return the parameter error before it looks at the handle."""
    lib = _capi.load()
    p = _capi.ahdsr_params(**kw)
    assert lib.pg_graph_set_voice_envelope(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER
    assert b"Invalid" in lib.pg_last_error_message()
    assert lib.pg_sharded_set_voice_envelope(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER


def test_null_params_is_an_error():
    lib = _capi.load()
    assert lib.pg_graph_set_voice_envelope(None, 0, None) == _capi.PG_ERR_PARAMETER
    assert lib.pg_sharded_set_voice_envelope(None, 0, None) == _capi.PG_ERR_PARAMETER


def test_edge_values_are_valid_parameters():
    """The closed ends of the ranges and zero times pass the parameter check (the null handle is what is reported then)."""
    lib = _capi.load()
    for kw in (dict(attack_scaling=1.0, decay_scaling=-1.0, release_scaling=1.0), dict(sustain_level=0.0), dict(sustain_level=1.0),
               dict(attack_s=0.0, hold_s=0.0, decay_s=0.0, release_s=0.0)):
        p = _capi.ahdsr_params(**kw)
        assert lib.pg_graph_set_voice_envelope(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER
        assert b"null" in lib.pg_last_error_message()
        assert lib.pg_sharded_set_voice_envelope(None, 0, C.byref(p)) == _capi.PG_ERR_PARAMETER
        assert b"null" in lib.pg_last_error_message()
    assert lib.pg_graph_release_voice(None, 0, 0) == _capi.PG_ERR_PARAMETER and lib.pg_sharded_release_voice(None, 0, 0) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_voice_envelope_stage(None, 0) == -1 and lib.pg_sharded_voice_envelope_stage(None, 0) == -1
