"""The playback status entry points of include/phonic_gpu.h: declared in the header, exported by the library, mirrored in _capi.py;
pg_status_event is 40 bytes with the header's layout; the errors that need no graph come back before anything touches a device."""
import ctypes as C
import math
import os
import re

from phonic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["enable_status", "set_voice_status", "poll_status", "status_dropped"]
SYMBOLS = [p + n for p in ("pg_graph_", "pg_sharded_") for n in NAMES]


def test_status_symbols_in_header_library_and_bindings():
    header = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    lib = C.CDLL(_capi.LIB_PATH)
    bound = _capi.load()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert hasattr(lib, s), s
        assert getattr(bound, s).argtypes is not None, s
    assert bound.pg_graph_status_dropped.restype is C.c_uint64 and bound.pg_sharded_status_dropped.restype is C.c_uint64


def test_status_event_layout():
    header = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    body = re.search(r"typedef struct pg_status_event \{(.*?)\} pg_status_event;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|uint64_t|double)\s+(\w+);", body, re.M)
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_capi.StatusEvent._fields_)
    assert C.sizeof(_capi.StatusEvent) == 40
    assert [getattr(_capi.StatusEvent, n).offset for n, _ in _capi.StatusEvent._fields_] == [0, 4, 8, 16, 24, 32, 36]
    assert "#define PG_STATUS_POSITION 0" in header and re.search(r"#define PG_STATUS_STOPPED\s+1", header)
    assert (_capi.PG_STATUS_POSITION, _capi.PG_STATUS_STOPPED) == (0, 1)


def test_errors_that_need_no_graph():
    lib = _capi.load()
    for prefix in ("pg_graph_", "pg_sharded_"):
        assert getattr(lib, prefix + "enable_status")(None, 16) == _capi.PG_ERR_PARAMETER
        assert b"null" in lib.pg_last_error_message()
        assert getattr(lib, prefix + "set_voice_status")(None, 0, 0.05, 1) == _capi.PG_ERR_PARAMETER
        assert getattr(lib, prefix + "set_voice_status")(None, 0, math.nan, 1) == _capi.PG_ERR_PARAMETER
        out = (_capi.StatusEvent * 4)()
        assert getattr(lib, prefix + "poll_status")(None, out, 4) == 0
        assert getattr(lib, prefix + "status_dropped")(None) == 0


def test_status_tuple():
    e = _capi.StatusEvent(_capi.PG_STATUS_POSITION, 3, 4096, 6001, 6001 / 48000, 0, 0)
    assert _capi.status_tuple(e) == ("position", 3, 4096, 6001, 6001 / 48000)
    e = _capi.StatusEvent(_capi.PG_STATUS_STOPPED, 3, 4096, 0, 0.0, 1, 0)
    assert _capi.status_tuple(e) == ("stopped", 3, 4096, True)
