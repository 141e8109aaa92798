"""Waveform overviews of sample buffers on the GPU (pg_graph_sample_buffer_waveform, phonic_amd/csrc/pg_k_waveform.hip) against
tests/waveform_model.py, the numpy-f32 restatement of waveform::mixed_down / multi_channel: frame, time, min and max of every point,
np.array_equal — values are compared, so +0 and -0 count as equal (the reference does not define a zero result's sign), and a NaN equals a NaN
(an upscaled point of a NaN sample is that NaN). The shapes are the ones at which the reference's f32 bucket boundaries differ from integer or
f64 ones (tests/test_waveform_model.py counts where), ramps pin both ends of every bucket, and every grid of the kernels is taken: one lane per
frame, 1 to 64 lanes per bucket, buckets split over workgroups. Every case prints its count of differing points. Everything goes through Graph;
the raw entry point is used only where the wrapper cannot make the call (a capacity one short)."""
import ctypes as C

import numpy as np
import pytest

import sample_buffer_model as SM
import waveform_model as W
from phonic_amd import _capi
from phonic_amd._wrap import PhonicError
from phonic_amd.graph import Graph

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("frame", "time", "min", "max")
MODES = ("mixed_down", "multi_channel")
RATE = {1: 48000, 2: 44100}
N_MONO_LONG, N_STEREO = 1000003, 262147
_CACHE = {}


def _pcm(kind, ch, n):
    """Read-only interleaved PCM, made once: 'ramp' (mono x[k] = k; stereo L = k, R = -k) or seeded noise in [-1, 1]."""
    key = (kind, ch, n)
    if key not in _CACHE:
        if kind == "ramp":
            k = np.arange(n, dtype=F)
            a = k if ch == 1 else np.stack([k, -k], axis=1).reshape(-1)
        else:
            a = np.random.default_rng(77 * ch + n).uniform(-1.0, 1.0, n * ch).astype(F)
        a = np.ascontiguousarray(a, dtype=F)
        a.setflags(write=False)
        _CACHE[key] = a
    return _CACHE[key]


def _model(pcm, ch, rate, res, mode, first=0, n=None):
    key = ("model", id(pcm), ch, rate, res, mode, first, n)
    if key not in _CACHE:
        _CACHE[key] = W.waveform(pcm, ch, rate, res, mode, first, n)
    return _CACHE[key]


def _compare(label, got, want):
    assert got.keys() == want.keys() == set(KEYS)
    shapes = {k: (got[k].shape, want[k].shape) for k in KEYS}
    assert all(a == b for a, b in shapes.values()), (label, shapes)
    differ = {k: int(np.count_nonzero(~((got[k] == want[k]) | ((got[k] != got[k]) & (want[k] != want[k]))))) for k in KEYS}
    print(f"{label}: {got['min'].size} points, differing frame/time/min/max: {differ['frame']}/{differ['time']}/{differ['min']}/{differ['max']}")
    assert got["frame"].dtype == np.uint64 and all(got[k].dtype == F for k in KEYS[1:])
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (label, k, differ)


def _check(g, buf, pcm, ch, res, mode, first=0, n=None, label=""):
    got = g.sample_buffer_waveform(buf, res, mode=mode, first_frame=first, n_frames=n)
    _compare(f"{label} {ch}ch res {res} {mode} [{first}, +{n}]", got, _model(pcm, ch, RATE[ch], res, mode, first, n))
    return got


class _Session:
    """One graph per buffer, made once per module: the buffers are immutable, every test reads them."""

    def __init__(self):
        self.items = {}

    def get(self, kind, ch, n):
        key = (kind, ch, n)
        if key not in self.items:
            g = Graph(48000, 2, 1024)
            self.items[key] = (g, g.add_sample_buffer(_pcm(kind, ch, n), ch, RATE[ch]))
        return self.items[key] + (_pcm(kind, ch, n),)

    def close(self):
        for g, _ in self.items.values():
            assert g.device_errors() == 0
            g.close()


@pytest.fixture(scope="module")
def buffers():
    s = _Session()
    yield s
    s.close()


# ---- bucket boundaries: the shapes at which f32 differs from integer arithmetic ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramp", "noise"])
@pytest.mark.parametrize("n,res", [(65537, 1024), (100003, 1000), (240001, 1920)])
def test_mono_boundaries(buffers, kind, n, res):
    g, buf, pcm = buffers.get(kind, 1, n)
    for mode in MODES:
        got = _check(g, buf, pcm, 1, res, mode, label=kind)
        assert got["min"].shape == ((res,) if mode == "mixed_down" else (1, res))
    if kind == "ramp":   # both ends of every bucket, read off the ramp: the f32 boundaries, not i * n // res
        b = W.boundaries(n, res)
        assert np.array_equal(got["min"][0], b[:-1].astype(F)) and np.array_equal(got["max"][0], (np.minimum(b[1:], n) - 1).astype(F))
        assert np.count_nonzero(b != W.integer_boundaries(n, res)) > 0
    assert g.device_errors() == 0


@pytest.mark.parametrize("kind", ["ramp", "noise"])
@pytest.mark.parametrize("mode", MODES)
def test_stereo_boundaries(buffers, kind, mode):
    g, buf, pcm = buffers.get(kind, 2, N_STEREO)
    got = _check(g, buf, pcm, 2, 4096, mode, label=kind)
    if kind == "ramp" and mode == "multi_channel":
        b = W.boundaries(N_STEREO, 4096)
        assert np.array_equal(got["min"][0], b[:-1].astype(F)) and np.array_equal(got["min"][1], -(np.minimum(b[1:], N_STEREO) - 1).astype(F))
    assert g.device_errors() == 0


# ---- the branch between one point per frame and buckets -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n", [1000, 1024, 1025, 2047])
def test_branch_edges(buffers, ch, n):
    g, buf, pcm = buffers.get("noise", ch, n)
    for mode in MODES:
        got = _check(g, buf, pcm, ch, 1024, mode, label="edge")
        assert got["min"].shape[-1] == min(n, 1024)
        if n <= 1024:
            assert np.array_equal(got["min"], got["max"])
    assert g.device_errors() == 0


# ---- long buckets: the split path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ramp", "noise"])
@pytest.mark.parametrize("res", [1, 3, 16])
def test_long_buckets_mono(buffers, kind, res):
    g, buf, pcm = buffers.get(kind, 1, N_MONO_LONG)
    for mode in MODES:
        _check(g, buf, pcm, 1, res, mode, label=kind)
    assert g.device_errors() == 0


@pytest.mark.parametrize("kind", ["ramp", "noise"])
def test_long_buckets_stereo(buffers, kind):
    g, buf, pcm = buffers.get(kind, 2, N_STEREO)
    for mode in MODES:
        for res in (2, 300):   # 300: buckets of 873 frames, one workgroup each
            _check(g, buf, pcm, 2, res, mode, label=kind)
    assert g.device_errors() == 0


# ---- slices -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2])
def test_slices(buffers, ch):
    g, buf, pcm = buffers.get("noise", ch, N_STEREO)
    gr, bufr, pcmr = buffers.get("ramp", 2, N_STEREO)
    for mode in MODES:
        for first in (12345, 12346):
            got = _check(g, buf, pcm, ch, 1000, mode, first, 100003, label="slice")
            assert got["frame"].reshape(-1)[0] == 0 and got["time"].reshape(-1)[0] == 0.0
        _check(g, buf, pcm, ch, 1000, mode, N_STEREO - 100003, 100003, label="slice to the last frame")
        _check(g, buf, pcm, ch, 7, mode, N_STEREO - 5001, 5001, label="slice to the last frame")
        _check(g, buf, pcm, ch, 1000, mode, 12347, 3, label="short slice")
        for first in (0, 77777, N_STEREO - 1):
            _check(g, buf, pcm, ch, 1024, mode, first, 1, label="one frame")
        _check(g, buf, pcm, ch, 2, mode, 12345, 200001, label="slice, split")
    got = _check(gr, bufr, pcmr, 2, 1000, "multi_channel", 12345, 100003, label="ramp slice")
    assert got["min"][0][0] == 12345.0 and got["max"][1][0] == -12345.0   # the values are the buffer's, the frames the slice's
    assert g.device_errors() == 0 and gr.device_errors() == 0


# ---- special values -----------------------------------------------------------------------------------------------------------------------
def _special_pcm():
    n = 3000
    pcm = np.random.default_rng(5).uniform(-1.0, 1.0, (n, 2)).astype(F)
    big = np.finfo(F).max
    b = W.boundaries(n, 1024)
    pcm[10] = (big, big)                   # the mono value stays finite: each sample is divided first
    pcm[11] = (-big, -big)
    pcm[100:104] = (1e-45, 1e-45)          # half the smallest denormal, twice: the mono value is 0, (l + r) / 2 would be 1e-45
    pcm[200] = (np.nan, 0.5)               # one NaN channel
    pcm[201] = (0.25, np.nan)
    for i in (300, 301, 500):              # whole buckets of NaN at resolution 1024: they keep f32::MAX / f32::MIN
        pcm[int(b[i]):int(b[i + 1])] = np.nan
    pcm[700] = (np.inf, np.inf)
    pcm[705] = (-np.inf, 1.0)
    pcm[710] = (np.inf, -np.inf)           # the mono value is NaN
    pcm[800:810] = -0.0
    pcm[int(b[900]):int(b[901])] = (-0.0, 0.0)
    pcm[int(b[901]):int(b[902])] = -0.0
    out = np.ascontiguousarray(pcm.reshape(-1))
    out.setflags(write=False)
    return out, b


@pytest.mark.parametrize("res", [1024, 4096])
@pytest.mark.parametrize("mode", MODES)
def test_special_values(res, mode):
    if "special" not in _CACHE:
        _CACHE["special"] = _special_pcm()
    pcm, b = _CACHE["special"]
    g = Graph(48000, 2, 1024)
    buf = g.add_sample_buffer(pcm, 2, 44100)
    got = g.sample_buffer_waveform(buf, res, mode=mode)
    _compare(f"special res {res} {mode}", got, _model(pcm, 2, 44100, res, mode))
    if res == 1024:
        mn, mx = got["min"].reshape(-1, 1024), got["max"].reshape(-1, 1024)
        for i in (300, 301, 500):
            assert (mn[:, i] == W.F32_MAX).all() and (mx[:, i] == W.F32_MIN).all()
        assert not np.isnan(mn).any() and not np.isnan(mx).any()   # a bucket never shows a NaN
        of = lambda frame: int(np.searchsorted(b, frame, side="right")) - 1   # the bucket of a frame
        assert (mx[:, of(10)] == np.finfo(F).max).all() and (mn[:, of(11)] == -np.finfo(F).max).all()   # finite in both modes
        if mode == "mixed_down":
            assert mn[0, 901] == 0.0 and mx[0, 901] == 0.0 and mn[0, 900] == 0.0   # buckets of zeros of either sign
    else:
        if mode == "mixed_down":
            assert got["min"][10] == np.finfo(F).max and got["min"][11] == -np.finfo(F).max and (got["min"][100:104] == 0.0).all()
            assert np.isnan(got["min"][200]) and np.isnan(got["max"][710]) and got["max"][700] == np.inf
        else:
            assert (got["min"][:, 100:104] == F(1e-45)).all() and np.isnan(got["min"][0][200]) and got["min"][1][200] == 0.5
    assert g.device_errors() == 0
    g.close()


# ---- the granular source ------------------------------------------------------------------------------------------------------------------
def test_granular_source():
    case = SM.CASES[1]   # stereo 44100 -> 48000
    ch, file_rate, graph_rate, n_in, n_out = case
    pcm, _ = SM.case_buffers(case)
    g = Graph(graph_rate, 2, 1024)
    buf = g.add_sample_buffer(pcm, ch, file_rate)
    assert g.sample_buffer_info(buf)["granular_frames"] == -1
    before = {(res, mode): g.sample_buffer_waveform(buf, res, mode=mode, source="granular") for res in (100, 4096) for mode in MODES}
    assert g.sample_buffer_info(buf)["granular_frames"] == n_out   # made by the first call that needed it
    g.prepare_granular_buffer(buf)
    mono = g.read_granular_buffer(buf)
    assert mono.size == n_out
    for (res, mode), got in before.items():
        want = W.waveform(mono, 1, graph_rate, res, mode)
        _compare(f"granular before prepare res {res} {mode}", got, want)
        _compare(f"granular after prepare res {res} {mode}", g.sample_buffer_waveform(buf, res, mode=mode, source="granular"), want)
        assert got["min"].shape == ((min(res, n_out),) if mode == "mixed_down" else (1, min(res, n_out)))
    part = g.sample_buffer_waveform(buf, 64, source="granular", first_frame=1001, n_frames=1500)
    _compare("granular slice", part, W.waveform(mono, 1, graph_rate, 64, "mixed_down", 1001, 1500))
    with pytest.raises(PhonicError) as e:
        g.sample_buffer_waveform(buf, 64, source="granular", first_frame=n_out - 10, n_frames=11)
    assert e.value.code == _capi.PG_ERR_PARAMETER
    assert g.sample_buffer_info(buf)["granular_frames"] == n_out and g.device_errors() == 0
    g.close()


# ---- between writes, while voices play the buffer -----------------------------------------------------------------------------------------
def test_overviews_between_writes_change_nothing():
    case = SM.CASES[1]
    ch, file_rate, graph_rate, n_in, n_out = case
    pcm, _ = SM.case_buffers(case)
    rng = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444)
    graphs = []
    for _ in range(2):
        g = Graph(graph_rate, 2, 1024)
        buf = g.add_sample_buffer(pcm, ch, file_rate, loop_range=(300, 1900))
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_GAIN, {"gain": 0.9})
        g.add_voice_from_buffer(m, buf, speed=0.7, volume=0.5)
        g.add_granular_voice_from_buffer(0, buf, _capi.granular_params(density=60.0, size=40.0, spray=0.3, rng_state=rng), volume=0.8)
        graphs.append((g, buf))
    (ga, bufa), (gb, bufb) = graphs
    first = {(mode, src): ga.sample_buffer_waveform(bufa, 200, mode=mode, source=src) for mode in MODES for src in ("file", "granular")}
    for k in range(8):
        oa, ob = np.zeros(2048, F), np.zeros(2048, F)
        assert ga.write(oa, k * 1024) == gb.write(ob, k * 1024) == 2048
        assert oa.tobytes() == ob.tobytes(), f"block {k}"
        for (mode, src), want in first.items():   # only graph a takes overviews
            got = ga.sample_buffer_waveform(bufa, 200, mode=mode, source=src)
            for key in KEYS:
                assert got[key].tobytes() == want[key].tobytes(), (k, mode, src, key)
    assert np.abs(oa).max() > 1e-3
    _compare("while playing", first[("multi_channel", "file")], W.waveform(pcm, ch, file_rate, 200, "multi_channel"))
    assert ga.device_errors() == 0 and gb.device_errors() == 0
    ga.close()
    gb.close()


# ---- errors with a device -----------------------------------------------------------------------------------------------------------------
def test_errors_with_a_device(buffers):
    g, buf, pcm = buffers.get("noise", 2, 2047)
    gm, bufm, _ = buffers.get("noise", 1, 2047)
    lib = _capi.load()

    def code(call):
        with pytest.raises(PhonicError) as e:
            call()
        return e.value.code

    assert code(lambda: g.sample_buffer_waveform(buf + 100, 64)) == _capi.PG_ERR_NOT_FOUND
    assert code(lambda: g.sample_buffer_waveform(-1, 64)) == _capi.PG_ERR_NOT_FOUND
    assert code(lambda: g.sample_buffer_waveform(buf, 64, first_frame=2000, n_frames=48)) == _capi.PG_ERR_PARAMETER   # one frame past the end
    assert code(lambda: g.sample_buffer_waveform(buf, 64, first_frame=2048, n_frames=1)) == _capi.PG_ERR_PARAMETER
    assert g.sample_buffer_waveform(buf, 64, first_frame=2000, n_frames=47)["min"].shape == (47,)
    # a capacity one short: PG_ERR_PARAMETER and nothing written (the wrapper always passes enough: the raw entry point)
    fn = lib.pg_graph_sample_buffer_waveform
    for handle, b, mode, n, res, need in ((g._h, buf, 0, 2047, 64, 64), (g._h, buf, 1, 2047, 64, 128), (g._h, buf, 1, 40, 64, 80), (gm._h, bufm, 1, 2047, 64, 64)):
        pts = (_capi.WaveformPoint * need)()
        C.memset(pts, 0xAB, C.sizeof(pts))
        assert fn(handle, b, 0, mode, 0, n, res, pts, need - 1) == -_capi.PG_ERR_PARAMETER
        assert bytes(pts) == b"\xAB" * C.sizeof(pts)
        assert fn(handle, b, 0, mode, 0, n, res, pts, need) == min(n, res)
        assert all(pts[i].reserved == 0 for i in range(need))
    # a released buffer
    g2 = Graph(48000, 2, 1024)
    b2 = g2.add_sample_buffer(pcm, 2, 44100)
    v = g2.add_voice_from_buffer(0, b2)
    assert g2.sample_buffer_waveform(b2, 16)["min"].shape == (16,)
    g2.release_sample_buffer(b2)
    assert code(lambda: g2.sample_buffer_waveform(b2, 16)) == _capi.PG_ERR_NOT_FOUND
    pts = (_capi.WaveformPoint * 16)()
    assert fn(g2._h, b2, 1, 0, 0, 100, 16, pts, 16) == -_capi.PG_ERR_NOT_FOUND
    out = np.zeros(2048, F)
    assert g2.write(out, 0) == 2048 and g2.is_voice_playing(v)   # the voice keeps playing the released buffer
    assert g.device_errors() == 0 and gm.device_errors() == 0 and g2.device_errors() == 0
    g2.close()
