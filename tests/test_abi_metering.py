"""The metering entry points of include/phonic_gpu.h: exported, pg_audio_level is 16 bytes, and the errors that need no graph are returned
before anything touches a device."""
import ctypes as C
import math

import pytest

from phonic_amd import _capi

SYMBOLS = ["pg_graph_set_metering", "pg_graph_mixer_audio_level", "pg_sharded_set_metering", "pg_sharded_mixer_audio_level"]


def test_metering_symbols_are_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_audio_level_is_sixteen_bytes():
    assert C.sizeof(_capi.AudioLevel) == 16
    assert _capi.AudioLevel.peak.offset == 0 and _capi.AudioLevel.rms.offset == 8


@pytest.mark.parametrize("interval", [math.nan, math.inf], ids=["nan", "inf"])
def test_bad_interval_is_a_parameter_error_without_a_device(interval):
    lib = _capi.load()
    assert lib.pg_graph_set_metering(None, interval) == _capi.PG_ERR_PARAMETER
    assert b"Invalid metering interval" in lib.pg_last_error_message()
    assert lib.pg_sharded_set_metering(None, interval) == _capi.PG_ERR_PARAMETER
    assert b"Invalid metering interval" in lib.pg_last_error_message()


@pytest.mark.parametrize("interval", [0.0, 0.05, -1.0], ids=["zero", "50ms", "off"])
def test_null_handle_is_a_parameter_error(interval):
    lib = _capi.load()
    assert lib.pg_graph_set_metering(None, interval) == _capi.PG_ERR_PARAMETER
    assert b"null" in lib.pg_last_error_message()
    assert lib.pg_sharded_set_metering(None, interval) == _capi.PG_ERR_PARAMETER
    assert b"null" in lib.pg_last_error_message()


def test_level_query_null_arguments():
    lib = _capi.load()
    out = _capi.AudioLevel()
    assert lib.pg_graph_mixer_audio_level(None, 0, C.byref(out)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_sharded_mixer_audio_level(None, 0, C.byref(out)) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_mixer_audio_level(None, 0, None) == _capi.PG_ERR_PARAMETER
    assert lib.pg_sharded_mixer_audio_level(None, 0, None) == _capi.PG_ERR_PARAMETER


def test_level_db():
    raw = _capi.AudioLevel()
    raw.peak[0], raw.peak[1], raw.rms[0], raw.rms[1] = 1.0, 0.0, 0.5, 0.1
    lv = _capi.Level(raw)
    assert lv.peak_db == (0.0, -math.inf)
    assert abs(lv.rms_db[0] - 20.0 * math.log10(0.5)) < 1e-12 and abs(lv.rms_db[1] + 20.0) < 1e-5
