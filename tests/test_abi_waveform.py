"""pg_graph_sample_buffer_waveform of include/phonic_gpu.h without a device: exported and mirrored in _capi, the point's layout, every argument
error that is answered before the handle (the handle is null in every call here) with its message, the null-handle answer, and the header,
INTEGRATION.md and DESIGN.md in step. The sharded handle has no such call, on purpose. CPU only."""
import ctypes as C
import os
import re

import pytest

from phonic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pg_graph_sample_buffer_waveform"


def test_symbol_is_exported_and_mirrored():
    raw = C.CDLL(_capi.LIB_PATH)
    assert hasattr(raw, SYMBOL) and hasattr(raw, "pg_debug_sample_buffer_waveform_time")
    assert not hasattr(raw, "pg_sharded_sample_buffer_waveform")
    fn = getattr(_capi.load(), SYMBOL)
    assert fn.restype is C.c_int64
    assert fn.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_capi.WaveformPoint), C.c_size_t]
    assert (_capi.PG_WAVEFORM_MIXED_DOWN, _capi.PG_WAVEFORM_MULTI_CHANNEL, _capi.PG_WAVEFORM_OF_FILE, _capi.PG_WAVEFORM_OF_GRANULAR) == (0, 1, 0, 1)


def test_point_layout():
    P = _capi.WaveformPoint
    assert C.sizeof(P) == 24
    assert (P.frame.offset, P.time.offset, P.min.offset, P.max.offset, P.reserved.offset) == (0, 8, 12, 16, 20)


def _call(lib, out=True, source=0, mode=0, first=0, n=1000, res=100, cap=None, handle=None):
    p = min(n, res)
    buf = (_capi.WaveformPoint * 4096)()
    return getattr(lib, SYMBOL)(handle, 0, source, mode, first, n, res, buf if out else None, 2 * p if cap is None else cap)


BAD = {
    "null out": (dict(out=False), b"output must not be null"),
    "resolution 0": (dict(res=0), b"resolution must be > 0"),
    "no frames": (dict(n=0), b"slice must not be empty"),
    "source 2": (dict(source=2), b"source must be"),
    "source -1": (dict(source=-1), b"source must be"),
    "mode 2": (dict(mode=2), b"mode must be"),
    "mode -1": (dict(mode=-1), b"mode must be"),
    "downscale, capacity one short": (dict(n=1000, res=100, cap=99), b"100 are needed"),
    "upscale, capacity one short": (dict(n=100, res=1000, cap=99), b"100 are needed"),
    "multi-channel, capacity below one channel": (dict(mode=1, n=1000, res=100, cap=99), b"100 are needed"),
    "no capacity": (dict(cap=0), b"are needed"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_errors_come_before_the_handle(what):
    lib = _capi.load()
    kw, message = BAD[what]
    assert _call(lib, **kw) == -_capi.PG_ERR_PARAMETER
    msg = lib.pg_last_error_message()
    assert message in msg, msg
    assert b"handle is null" not in msg   # the argument is what is reported, not the null handle


def test_valid_arguments_reach_the_handle_check():
    lib = _capi.load()
    for kw in (dict(), dict(source=1), dict(mode=1), dict(source=1, mode=1), dict(n=100, res=1000), dict(n=1, res=1, cap=1), dict(first=1 << 40),
               dict(mode=1, cap=100),    # multi-channel with room for one channel: enough for a mono source, decided once the buffer is known
               dict(mode=0, cap=100), dict(n=(1 << 40), res=4096), dict(n=5, res=0xFFFFFFFF, cap=5)):
        assert _call(lib, **kw) == -_capi.PG_ERR_PARAMETER
        assert b"handle is null" in lib.pg_last_error_message(), kw
    out = C.c_float(1.0)
    assert lib.pg_debug_sample_buffer_waveform_time(None, 0, C.byref(out)) == _capi.PG_ERR_PARAMETER


def test_header_and_documents_agree():
    header = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"\b" + SYMBOL + r"\s*\(", header)
    assert re.search(r"pub fn " + SYMBOL + r"\s*\(", doc)
    assert "Duration::from_secs_f32" in doc and "Vec<Vec<Point>>" in doc
    for name in ("PG_WAVEFORM_MIXED_DOWN", "PG_WAVEFORM_MULTI_CHANNEL", "PG_WAVEFORM_OF_FILE", "PG_WAVEFORM_OF_GRANULAR", "pg_waveform_point"):
        assert name in header, name
    m = re.search(r"typedef struct pg_waveform_point \{(.*?)\} pg_waveform_point;", header, flags=re.S)
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", fields) == ["frame", "time", "min", "max", "reserved"]
    assert "pg_sharded_sample_buffer_waveform" not in header and "pg_sharded_sample_buffer_waveform" not in doc
    assert "NOT a real-time call" in header and "single-device graph" in header
    for phrase in ("Waveform overviews", "pg_k_waveform", "pg_waveform_split_kernel", "pg_waveform_bucket_kernel"):
        assert phrase in design, phrase


def test_sharded_graph_says_where_to_take_overviews_from():
    from phonic_amd.graph import ShardedGraph

    s = ShardedGraph.__new__(ShardedGraph)   # no handle, no device: the method must not need either
    s._h = None
    with pytest.raises(NotImplementedError, match="single-device"):
        s.sample_buffer_waveform(0, 1024)
