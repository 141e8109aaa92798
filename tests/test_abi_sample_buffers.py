"""The sample-buffer entry points of include/phonic_gpu.h: exported on both handles, their argument checks answered before a graph or a device
is touched (the handle is null in every call here), the structs' layouts, and the header and INTEGRATION.md in step. CPU only."""
import ctypes as C
import os
import re

import pytest

from phonic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["add_sample_buffer", "release_sample_buffer", "add_voice_from_buffer", "add_granular_voice_from_buffer", "prepare_granular_buffer",
         "sample_buffer_info", "read_granular_buffer"]
SYMBOLS = [p + n for p in ("pg_graph_", "pg_sharded_") for n in NAMES]


def test_sample_buffer_symbols_are_exported_on_both_handles():
    lib = C.CDLL(_capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_struct_layouts():
    assert C.sizeof(_capi.SampleBufferDesc) == 32 and _capi.SampleBufferDesc.loop_start.offset == 16
    assert C.sizeof(_capi.SampleBufferInfo) == 48 and _capi.SampleBufferInfo.granular_frames.offset == 40


N = 8
BAD = {
    "null pcm": dict(pcm=False),
    "null desc": dict(desc=False),
    "no frames": dict(n_frames=0),
    "no channels": dict(channels=0),
    "three channels": dict(channels=3),
    "rate 0": dict(rate=0),
    "loop start at the end": dict(loop=(N, N)),
    "loop start behind the end": dict(loop=(N + 5, N)),
    "loop end behind the end": dict(loop=(0, N + 1)),
    "empty loop inside the buffer": dict(loop=(3, 3)),       # AudioFileBuffer::new (file/buffer.rs:49-55): start >= end
    "reversed loop inside the buffer": dict(loop=(5, 2)),
}


@pytest.mark.parametrize("prefix", ["pg_graph_", "pg_sharded_"])
@pytest.mark.parametrize("what", sorted(BAD))
def test_add_sample_buffer_checks_its_arguments_without_a_device(prefix, what):
    lib = _capi.load()
    kw = BAD[what]
    pcm = (C.c_float * (3 * N))()
    d = _capi.sample_buffer_desc(kw.get("channels", 2), kw.get("rate", 48000), kw.get("loop"))
    rc = getattr(lib, prefix + "add_sample_buffer")(None, pcm if kw.get("pcm", True) else None, kw.get("n_frames", N), C.byref(d) if kw.get("desc", True) else None)
    assert rc == -_capi.PG_ERR_PARAMETER
    assert b"handle is null" not in lib.pg_last_error_message()   # the argument is what is reported, not the null handle


@pytest.mark.parametrize("prefix", ["pg_graph_", "pg_sharded_"])
def test_valid_arguments_reach_the_handle_check(prefix):
    lib = _capi.load()
    pcm = (C.c_float * (2 * N))()
    for d in (_capi.sample_buffer_desc(2, 44100), _capi.sample_buffer_desc(1, 1), _capi.sample_buffer_desc(2, 48000, (0, N)), _capi.sample_buffer_desc(1, 48000, (N - 1, N))):
        assert getattr(lib, prefix + "add_sample_buffer")(None, pcm, N, C.byref(d)) == -_capi.PG_ERR_PARAMETER
        assert b"handle is null" in lib.pg_last_error_message()
    f = lambda name: getattr(lib, prefix + name)
    assert f("release_sample_buffer")(None, 0) == _capi.PG_ERR_PARAMETER
    assert f("prepare_granular_buffer")(None, 0) == _capi.PG_ERR_PARAMETER
    assert f("add_voice_from_buffer")(None, 0, 0, None) == -_capi.PG_ERR_PARAMETER
    info = _capi.SampleBufferInfo()
    assert f("sample_buffer_info")(None, 0, C.byref(info)) == _capi.PG_ERR_PARAMETER
    out = (C.c_float * 4)()
    if prefix == "pg_graph_":
        assert lib.pg_debug_sample_buffer_times(None, 0, out) == _capi.PG_ERR_PARAMETER
    args = (None, 0, out, 4) if prefix == "pg_graph_" else (None, 0, -1, out, 4)
    assert f("read_granular_buffer")(*args) == -_capi.PG_ERR_PARAMETER
    # the granular parameters come before the handle, as for pg_graph_add_granular_voice
    bad = _capi.granular_params(size=0.5)
    assert f("add_granular_voice_from_buffer")(None, 0, 0, C.byref(bad), None) == -_capi.PG_ERR_PARAMETER
    assert b"handle is null" not in lib.pg_last_error_message()
    good = _capi.granular_params()
    assert f("add_granular_voice_from_buffer")(None, 0, 0, C.byref(good), None) == -_capi.PG_ERR_PARAMETER
    assert b"handle is null" in lib.pg_last_error_message()


def test_header_and_documents_agree():
    header = open(os.path.join(ROOT, "include", "phonic_gpu.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert re.search(r"pub fn " + s + r"\s*\(", doc), s
    assert "the mono down-mix and resample of" not in header   # the OUT OF SCOPE note on create_granular_sample_buffer is gone
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for phrase in ("Sample buffers", "pg_sample_sched_kernel", "pg_sample_interp_kernel", "HighQuality"):
        assert phrase in design, phrase
