"""Sample buffers on the GPU (pg_graph_add_sample_buffer and the voices made from one): the granular mono buffer the device makes
(pg_sample_sched_kernel + pg_sample_interp_kernel) against tests/sample_buffer_model.py — every sample, np.array_equal: values are compared, so
+0 and -0 count as equal (the sign of an all-zero frame's sum depends on the Rust release's `Sum` identity) —, voices from a buffer against
today's voices with a private copy, byte for byte, and the ownership rules by the library's own counters (pg_debug_hip_calls). Everything goes
through the C ABI."""
import gc

import numpy as np
import pytest

import phonic_amd
import sample_buffer_model as M
from phonic_amd import _capi, workloads
from phonic_amd.graph import Graph, ShardedGraph, hip_calls

pytestmark = pytest.mark.gpu

F = np.float32
MONO_SAME_RATE = (1, 48000, 48000, 1301, 1301)
GRAN_CASE = M.CASES[1]   # stereo 44100 -> 48000, 2301 frames in, 2503 out
RNG = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444)


def case_id(c):
    return f"{c[0]}ch-{c[1]}to{c[2]}-{c[3]}f"


# ---- conversion ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES + [MONO_SAME_RATE], ids=case_id)
def test_granular_buffer_equals_the_model(case):
    ch, file_rate, graph_rate, n_in, n_out = case
    pcm, mono = M.case_buffers(case)
    assert mono.size == n_out
    g = Graph(graph_rate, 2, 1024)
    b = g.add_sample_buffer(pcm, ch, file_rate)
    info = g.sample_buffer_info(b)
    assert (info["n_frames"], info["channels"], info["rate"], info["loop_range"], info["use_count"], info["granular_frames"]) == (n_in, ch, file_rate, None, 0, -1)
    g.prepare_granular_buffer(b)
    assert g.sample_buffer_info(b)["granular_frames"] == n_out
    c0 = hip_calls()
    g.prepare_granular_buffer(b)   # a no-op: no allocation, no copy, no wait
    assert hip_calls() == c0
    got = g.read_granular_buffer(b)
    print(f"{case_id(case)}: {got.size} frames (model {mono.size}), {int(np.count_nonzero(got[:min(got.size, mono.size)] != mono[:min(got.size, mono.size)]))} samples differ")
    assert got.size == mono.size
    assert np.array_equal(got, mono)
    assert g.device_errors() == 0
    g.close()


# ---- granular playback ---------------------------------------------------------------------------------------------------------------
def _states_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("loop", [None, (300, 1900)], ids=["no-loop", "buffer-loop"])
def test_granular_voice_from_a_buffer_renders_what_the_model_buffer_renders(loop):
    ch, file_rate, graph_rate, n_in, n_out = GRAN_CASE
    pcm, mono = M.case_buffers(GRAN_CASE)
    kw = dict(density=60.0, size=40.0, variation=0.5, spray=0.3, pan_spread=1.0, playback_direction=2, step=1.0, position=0.25)
    ga, gb = Graph(graph_rate, 2, 1024), Graph(graph_rate, 2, 1024)
    # the parent's way: the model's mono buffer, the file's loop range normalised as SamplerVoice::enable_granular_playback does (voice.rs:355-360)
    norm = None if loop is None else (float(F(loop[0]) / F(n_in)), float(F(loop[1]) / F(n_in)))
    va = ga.add_granular_voice(0, mono, _capi.granular_params(loop_range=norm, rng_state=RNG, **kw), volume=0.8, panning=-0.2, speed=1.25)
    buf = gb.add_sample_buffer(pcm, ch, file_rate, loop_range=loop)
    vb = gb.add_granular_voice_from_buffer(0, buf, _capi.granular_params(rng_state=RNG, **kw), volume=0.8, panning=-0.2, speed=1.25)
    assert gb.sample_buffer_info(buf)["use_count"] == 1 and gb.sample_buffer_info(buf)["granular_frames"] == n_out
    pa, pb = ga.voice_granular_params(va), gb.voice_granular_params(vb)
    _states_equal(pa, pb)
    for k in range(4):
        oa, ob = np.zeros(2048, F), np.zeros(2048, F)
        assert ga.write(oa, k * 1024) == gb.write(ob, k * 1024) == 2048
        assert oa.tobytes() == ob.tobytes(), f"write {k}"
        _states_equal(ga.voice_grain_state(va), gb.voice_grain_state(vb))
    assert np.abs(oa).max() > 1e-3
    assert ga.device_errors() == 0 and gb.device_errors() == 0
    ga.close()
    gb.close()


# ---- file voices ---------------------------------------------------------------------------------------------------------------------
FILE_PCM_FRAMES = 4001


def _file_pcm():
    return M.make_pcm(2, FILE_PCM_FRAMES, seed=7)


def _voice_options(i):
    o = dict(speed=(0.5, 1.0, 1.7)[i % 3], volume=0.25, panning=float(F(-0.9 + 0.12 * i)))
    if i == 3:
        o.update(has_loop_range=1, loop_start=100, loop_end=900, has_repeat=1, repeat=3)
    if i == 5:
        o.update(start_time=1024 + 300)
    if i == 7:
        o.update(source_rate=32000)
    if i == 8:
        o.update(has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    return o


def _build_file_graph(shared):
    g = Graph(48000, 2, 1024)
    pcm = _file_pcm()
    buf = g.add_sample_buffer(pcm, 2, 44100) if shared else None
    voices = []
    for i in range(16):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_GAIN, {"gain": 0.9})
        g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
        voices.append(g.add_voice_from_buffer(m, buf, **_voice_options(i)) if shared else g.add_voice(m, pcm, 2, 44100, **_voice_options(i)))
    g.stop_voice(voices[9], 2500)   # one stop with its fade-out, inside the third block
    return g, buf, voices


def test_file_voices_from_one_buffer_render_what_private_copies_render():
    ga, _, _ = _build_file_graph(False)
    gb, buf, _ = _build_file_graph(True)
    assert gb.sample_buffer_info(buf)["use_count"] == 16
    assert ga.dominant_kernel() == gb.dominant_kernel()
    for k in range(8):
        oa, ob = np.zeros(2048, F), np.zeros(2048, F)
        assert ga.write(oa, k * 1024) == gb.write(ob, k * 1024) == 2048
        assert oa.tobytes() == ob.tobytes(), f"block {k}"
        assert ga.deferred_units() == gb.deferred_units(), f"block {k}"
    assert np.abs(oa).max() > 1e-3
    assert ga.dominant_kernel() == gb.dominant_kernel()
    assert ga.device_errors() == 0 and gb.device_errors() == 0
    ga.close()
    gb.close()


def test_embedded_loop_range_loops_forever():
    """has_repeat == 0 on a buffer with a loop range: forever, over that range — pg_graph_add_voice with the range as override and PG_REPEAT_FOREVER.
    An override wins over the buffer's range."""
    pcm = M.make_pcm(2, 1201, seed=3)
    ga, gb = Graph(48000, 2, 1024), Graph(48000, 2, 1024)
    buf = gb.add_sample_buffer(pcm, 2, 44100, loop_range=(200, 1000))
    ga.add_voice(0, pcm, 2, 44100, has_loop_range=1, loop_start=200, loop_end=1000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    gb.add_voice_from_buffer(0, buf)
    ma, mb = ga.add_mixer(), gb.add_mixer()
    ga.add_voice(ma, pcm, 2, 44100, has_loop_range=1, loop_start=50, loop_end=400, has_repeat=1, repeat=2, speed=1.7)
    gb.add_voice_from_buffer(mb, buf, has_loop_range=1, loop_start=50, loop_end=400, has_repeat=1, repeat=2, speed=1.7)
    for k in range(6):   # 6144 output frames: the 1201-frame file several times over
        oa, ob = np.zeros(2048, F), np.zeros(2048, F)
        assert ga.write(oa, k * 1024) == gb.write(ob, k * 1024) == 2048
        assert oa.tobytes() == ob.tobytes(), f"block {k}"
    assert np.abs(oa).max() > 1e-3   # still playing behind the file's end
    ga.close()
    gb.close()


def test_timed_calls_on_voices_from_a_buffer_match_private_copies():
    """seek, speed (with a glide), volume, panning, stop and release reach a voice made from a buffer as they reach any file voice: the bus of a
    graph of private copies, byte for byte. The seeks land on whole frames: 0.5 s and 0.25 s x 44100 Hz x 2 channels are exact even sample
    offsets (PreloadedFileSource::seek takes `seconds x rate x channels as usize`, preloaded.rs:137-145, as it comes)."""
    st = M.make_pcm(2, 24001, seed=5)
    mo = M.make_pcm(1, 5001, seed=6)
    graphs = []
    for shared in (False, True):
        g = Graph(48000, 2, 1024)
        m1, m2 = g.add_mixer(), g.add_mixer()
        g.add_effect(m1, _capi.FX_GAIN, {"gain": 0.8})
        g.add_effect(m2, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(3))
        if shared:
            bs, bm = g.add_sample_buffer(st, 2, 44100, loop_range=(2000, 20000)), g.add_sample_buffer(mo, 1, 32000)
            v = [g.add_voice_from_buffer(m1, bs, has_repeat=1, repeat=0, volume=0.5), g.add_voice_from_buffer(m2, bs, volume=0.4, speed=1.7),
                 g.add_voice_from_buffer(0, bm, volume=0.6, panning=0.3), g.add_voice_from_buffer(m1, bs, has_repeat=1, repeat=0, volume=0.3, start_time=700)]
        else:
            loop = dict(has_loop_range=1, loop_start=2000, loop_end=20000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
            v = [g.add_voice(m1, st, 2, 44100, has_repeat=1, repeat=0, volume=0.5), g.add_voice(m2, st, 2, 44100, volume=0.4, speed=1.7, **loop),
                 g.add_voice(0, mo, 1, 32000, volume=0.6, panning=0.3), g.add_voice(m1, st, 2, 44100, has_repeat=1, repeat=0, volume=0.3, start_time=700)]
        g.seek_voice(v[0], 0.5, 1500)
        g.seek_voice(v[1], 0.25, 0)
        g.seek_voice(v[2], 0.05, 2100)
        g.set_voice_speed(v[0], 0.7, 2600, glide=24.0)
        g.set_voice_volume(v[1], 0.9, 1100)
        g.set_voice_panning(v[2], -0.6, 3000)
        g.stop_voice(v[3], 2300)
        g.release_voice(v[2], 3500)
        graphs.append(g)
    ga, gb = graphs
    for k in range(5):
        oa, ob = np.zeros(2048, F), np.zeros(2048, F)
        assert ga.write(oa, k * 1024) == gb.write(ob, k * 1024) == 2048
        assert oa.tobytes() == ob.tobytes(), f"block {k}"
        assert ga.deferred_units() == gb.deferred_units(), f"block {k}"
    assert np.abs(oa).max() > 1e-3
    assert ga.device_errors() == 0 and gb.device_errors() == 0
    ga.close()
    gb.close()


# ---- ownership -----------------------------------------------------------------------------------------------------------------------
def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def test_ownership_by_the_library_counters():
    pcm = M.make_pcm(2, 3001, seed=11)
    n_voices = 64
    gc.collect()   # (the counters are process-wide: graphs of earlier tests are released here, not inside the windows below)
    start = hip_calls()
    g = Graph(48000, 2, 1024)
    sub = g.add_mixer()
    g.add_effect(sub, _capi.FX_GAIN, {"gain": 0.5})
    # the parent's way, on a graph of its own: one PCM allocation per voice
    gp = Graph(48000, 2, 1024)
    subp = gp.add_mixer()
    gp.add_effect(subp, _capi.FX_GAIN, {"gain": 0.5})
    c0 = hip_calls()
    for i in range(n_voices):
        gp.add_voice(subp, pcm, 2, 44100, volume=0.05, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER, start_time=7 * i)
    private = _delta(c0, hip_calls())
    c0 = hip_calls()
    buf = g.add_sample_buffer(pcm, 2, 44100)
    upload = _delta(c0, hip_calls())
    voices = [g.add_voice_from_buffer(sub, buf, volume=0.05, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER, start_time=7 * i) for i in range(n_voices)]
    shared = _delta(c0, hip_calls())
    print("private copies:", private, " one buffer:", shared, " its upload:", upload)
    assert upload["alloc"] == 1
    assert private["alloc"] - (shared["alloc"] - upload["alloc"]) == n_voices   # 64 PCM allocations fewer (the one upload aside)
    assert g.sample_buffer_info(buf)["use_count"] == n_voices
    a, b = np.zeros(2048, F), np.zeros(2048, F)
    assert g.write(a, 0) == gp.write(b, 0) == 2048 and a.tobytes() == b.tobytes()
    # release while the voices play: no output byte changes, the id is gone, nothing is freed yet
    c0 = hip_calls()
    g.release_sample_buffer(buf)
    assert _delta(c0, hip_calls())["free"] == 0
    for call in (lambda: g.sample_buffer_info(buf), lambda: g.release_sample_buffer(buf), lambda: g.add_voice_from_buffer(sub, buf),
                 lambda: g.prepare_granular_buffer(buf), lambda: g.add_granular_voice_from_buffer(sub, buf)):
        with pytest.raises(phonic_amd.PhonicError) as ei:
            call()
        assert ei.value.code == _capi.PG_ERR_NOT_FOUND
    for k in range(1, 3):
        assert g.write(a, k * 1024) == gp.write(b, k * 1024) == 2048 and a.tobytes() == b.tobytes(), f"block {k}"
    assert np.abs(a).max() > 1e-3
    # the voices go: their removal travels with the next write, which frees nothing; the memory is released — like a private copy's, outside
    # the write — by the first graph-changing call behind it (here: the release of another buffer, which owns one allocation itself)
    dummy = g.add_sample_buffer(pcm[:64], 2, 44100)
    for v in voices:
        g.remove_voice(v)
    c0 = hip_calls()
    g.write(a, 3 * 1024)
    d = _delta(c0, hip_calls())
    assert d["free"] == 0 and d["alloc"] == 0
    c0 = hip_calls()
    g.release_sample_buffer(dummy)
    d = _delta(c0, hip_calls())
    print("first graph-changing call behind the last voice's removal:", d)
    assert d["free"] == 2 and d["alloc"] == 0   # the other buffer's PCM and the shared buffer's (no granular buffer was made)
    g.close()
    gp.close()
    end = hip_calls()
    print("both graphs, created to destroyed:", _delta(start, end))
    assert end["alloc"] - start["alloc"] == end["free"] - start["free"]


def test_granular_buffer_goes_with_the_buffer():
    """A converted buffer owns two allocations (PCM, granular mono buffer); a mono buffer at the graph's rate one (the granular buffer is the PCM).
    Both go when the last reference does; destroying the graph releases what is still held."""
    ch, file_rate, graph_rate, n_in, n_out = GRAN_CASE
    pcm, _ = M.case_buffers(GRAN_CASE)
    mono_pcm, _ = M.case_buffers(MONO_SAME_RATE)
    gc.collect()
    start = hip_calls()
    g = Graph(graph_rate, 2, 1024)
    b1 = g.add_sample_buffer(pcm, ch, file_rate)
    b2 = g.add_sample_buffer(mono_pcm, 1, 48000)
    c0 = hip_calls()
    g.prepare_granular_buffer(b2)
    assert _delta(c0, hip_calls())["alloc"] == 0   # aliased, not copied
    g.prepare_granular_buffer(b1)
    d = _delta(c0, hip_calls())
    assert d["alloc"] - d["free"] == 1             # the scratch tables are gone again, the mono buffer stays
    c0 = hip_calls()
    g.release_sample_buffer(b1)
    assert _delta(c0, hip_calls())["free"] == 2
    c0 = hip_calls()
    g.release_sample_buffer(b2)
    assert _delta(c0, hip_calls())["free"] == 1
    b3 = g.add_sample_buffer(pcm, ch, file_rate)
    v = g.add_granular_voice_from_buffer(0, b3, _capi.granular_params(rng_state=RNG))
    out = np.zeros(2048, F)
    assert g.write(out, 0) == 2048
    g.close()   # a held buffer with a playing voice
    end = hip_calls()
    assert end["alloc"] - start["alloc"] == end["free"] - start["free"], _delta(start, end)


# ---- sharded handle ------------------------------------------------------------------------------------------------------------------
def _build_two_mixers(g):
    pcm = _file_pcm()
    buf = g.add_sample_buffer(pcm, 2, 44100, loop_range=(500, 3500))
    for i in range(2):   # one sub-mixer per shard (the least loaded one takes the next): the bus is the sum of two rows on either handle
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_GAIN, {"gain": 0.9})
        g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
        g.add_voice_from_buffer(m, buf, speed=(1.0, 1.7)[i], volume=0.4, panning=(-0.5, 0.5)[i])
        g.add_voice_from_buffer(m, buf, speed=0.5, volume=0.3, start_time=700 + 300 * i, has_repeat=1, repeat=1)
    return buf


def test_sharded_handle_two_shards_on_one_device():
    ga, gs = Graph(48000, 2, 1024), ShardedGraph([0, 0], 48000, 2, 1024)
    _build_two_mixers(ga)
    buf = _build_two_mixers(gs)
    assert gs.shard_count() == 2 and gs._lib.pg_sharded_shard_of_mixer(gs._h, 1) != gs._lib.pg_sharded_shard_of_mixer(gs._h, 2)
    assert gs.sample_buffer_info(buf)["use_count"] == 4
    for k in range(4):
        oa, ob = np.zeros(2048, F), np.zeros(2048, F)
        assert ga.write(oa, k * 1024) == gs.write(ob, k * 1024) == 2048
        assert oa.tobytes() == ob.tobytes(), f"block {k}"
    assert np.abs(oa).max() > 1e-3
    ch, file_rate, graph_rate, n_in, n_out = GRAN_CASE
    pcm, mono = M.case_buffers(GRAN_CASE)
    gbuf = gs.add_sample_buffer(pcm, ch, file_rate)
    r0, r1 = gs.read_granular_buffer(gbuf, 0), gs.read_granular_buffer(gbuf, 1)
    assert np.array_equal(r0, mono) and np.array_equal(r1, mono)
    gs.release_sample_buffer(gbuf)
    with pytest.raises(phonic_amd.PhonicError) as ei:
        gs.sample_buffer_info(gbuf)
    assert ei.value.code == _capi.PG_ERR_NOT_FOUND
    ga.close()
    gs.close()
