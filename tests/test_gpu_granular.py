"""Granular voices on the GPU (pg_graph_add_granular_voice, pg_grain_kernel) against the independent numpy model of the reference's grain
engine (tests/granular_model.py, src/generator/sampler/granular.rs). Everything goes through the C ABI.

After EVERY write two things are checked:
  state   pg_graph_voice_grain_state equals the model bit for bit, every field of the pool and of its 100 grains;
  output  |gpu - model| <= 2 n 2^-23 S per frame and channel, n = the grains that contribute to the frame and S = the sum of their |terms|, both
          from the model: the bound of re-ordering an f32 sum of n exact terms (each partial sum is within n 2^-24 S of exact in either order).
          It is derived, not measured; with n <= 1 it is 0 and the output is bit-equal. (tests/test_granular_model.py checks that the model
          against itself over call cuttings stays inside it for these inputs.)
The source is 2048 mono frames of a seeded sine plus ramp; the graph runs at 8000 Hz so that 100 concurrent grains are reached within 8000
frames. The model's process calls are cut where the device's are: at the ends of the writes, on the 4096-frame chunk grid, at the voice's
events (volume, panning, speed, release) and at a stop time; the voice ends with the call in which the pool became exhausted or the envelope
Idle."""
import numpy as np
import pytest

import ahdsr_model as A
import granular_model as gm
from phonic_amd import _capi
from phonic_amd.graph import Graph, ShardedGraph

pytestmark = pytest.mark.gpu

SR = 8000
MF = 1024
RNG = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444)
CLOUD = dict(density=100.0, size=1000.0, variation=1.0, spray=1.0, pan_spread=1.0, playback_direction=gm.RANDOM, step=1.0)
EVENTS = ("volume", "panning", "speed", "release")   # events of the voice's mixer: its chunk is cut there


class Model:
    """The voice as the model renders it: frame t of the graph is frame t - start of the pool."""

    def __init__(self, kw, sr=SR, buf=None, rng=RNG, speed=1.0, volume=1.0, panning=0.0, start=0, cmds=(), env=None):
        self.buf = gm.make_buffer(2048) if buf is None else buf
        self.pool = gm.GrainPool(sr, self.buf, gm.Params(**kw), rng, speed, volume, panning)
        self.sr, self.start, self.cmds, self.env_kw = sr, start, sorted(cmds, key=lambda c: c[0]), env
        self.t = 0
        self.ended = False
        self.env = None
        if env is not None:
            self.env_params = A.Params(sr, **env)
            self.env = A.Envelope()
            self.env.note_on(self.env_params, 1.0)
        self.has_env = env is not None

    def _apply(self, t):
        for (ct, name, value) in self.cmds:
            if ct != t:
                continue
            if name == "volume":
                self.pool.set_volume(value)
            elif name == "panning":
                self.pool.set_panning(value)
            elif name == "speed":
                self.pool.set_speed(value)
            elif name == "stop":
                self.pool.stop()
            elif name == "release":
                if self.has_env:
                    self.env.note_off(self.env_params)
                else:
                    self.pool.stop()

    def write(self, n):
        """One write call of n frames: (out[n, 2] f32, cnt[n], S[n, 2])."""
        t0, t1 = self.t, self.t + n
        cuts = {t1} | {t0 + k for k in range(4096, n, 4096)}
        cuts |= {ct for (ct, name, _) in self.cmds if t0 < ct < t1}
        if t0 < self.start < t1:
            cuts.add(self.start)
        out, cnt, S = np.zeros((n, 2), np.float32), np.zeros(n, np.int64), np.zeros((n, 2))
        a = t0
        for b in sorted(cuts):
            self._apply(a)
            if not self.ended and b > self.start:
                o, c, s = self.pool.process(b - a)
                if self.env is not None:
                    if self.env.stage in (A.SUSTAIN, A.IDLE):
                        gains = np.full(b - a, self.env.output, dtype=np.float32)
                    else:
                        gains = np.array([self.env.run(self.env_params) for _ in range(b - a)], dtype=np.float32)
                    o = (o * gains[:, None]).astype(np.float32)
                    s = s * gains[:, None].astype(np.float64)
                out[a - t0:b - t0], cnt[a - t0:b - t0], S[a - t0:b - t0] = o, c, s
                if self.pool.is_exhausted() or (self.env is not None and self.env.stage == A.IDLE):
                    self.ended = True
            a = b
        self.t = t1
        return out, cnt, S


def _add(g, mixer, m, **extra):
    p = m.pool.p
    gp = _capi.granular_params(loop_range=p.loop_range, rng_state=RNG if extra.get("rng") is None else extra["rng"], overlap_mode=p.overlap_mode, window=p.window,
                               size=p.size, density=p.density, variation=p.variation, spray=p.spray, pan_spread=p.pan_spread,
                               playback_direction=p.playback_direction, position=p.position, step=p.step)
    v = g.add_granular_voice(mixer, m.buf, gp, speed=float(m.pool.speed), volume=float(m.pool.volume), panning=float(m.pool.panning), start_time=m.start)
    if m.env_kw is not None:
        g.set_voice_envelope(v, **m.env_kw)
    for (t, name, value) in m.cmds:
        if name == "volume":
            g.set_voice_volume(v, value, t)
        elif name == "panning":
            g.set_voice_panning(v, value, t)
        elif name == "speed":
            g.set_voice_speed(v, value, t)
        elif name == "stop":
            g.stop_voice(v, t)
        elif name == "release":
            g.release_voice(v, t)
    return v


def _check_write(g, v, m, got, exp, cnt, S, tag, exact=False):
    exp = exp + np.float32(0.0)   # the mixer ADDS the voice into its zeroed block (add_buffers, mixed.rs:558-624): 0.0 + -0.0 = +0.0
    got, bound = got.reshape(-1, 2), 2.0 * cnt[:, None] * 2.0 ** -23 * S
    diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    bad = np.flatnonzero((diff > bound).any(axis=1))
    assert len(bad) == 0, (tag, "output", int(bad[0]), float(diff.max()), int(cnt[bad[0]]))
    one = cnt <= 1
    assert np.array_equal(got[one].view(np.uint32), exp[one].view(np.uint32)), (tag, "frames with at most one grain are bit-equal")
    if exact:
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (tag, "bit-equal throughout")
    st = g.voice_grain_state(v)
    assert gm.states_equal(m.pool.state(), st) == [], (tag, gm.states_equal(m.pool.state(), st))
    assert g.is_voice_playing(v) == (not m.ended), (tag, "playing", m.ended)


def _run(kw, sizes, mf=MF, exact=False, graph=None, mixer=0, **mkw):
    m = Model(kw, **mkw)
    g = graph or Graph(m.sr, 2, mf, 0)
    v = _add(g, mixer, m)
    pos, outs, stats = 0, [], dict(max_n=0, peak=0.0)
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        exp, cnt, S = m.write(n)
        _check_write(g, v, m, buf, exp, cnt, S, (k, pos), exact)
        stats["max_n"] = max(stats["max_n"], int(cnt.max()))
        stats["peak"] = max(stats["peak"], float(np.abs(exp).max()))
        pos += n
        outs.append(buf)
    assert g.device_errors() == 0
    return m, np.concatenate(outs), stats, g, v


def test_defaults_one_grain_at_a_time():
    m, out, st, g, v = _run(dict(), [MF] * 5, exact=True)
    assert st["max_n"] == 1 and st["peak"] > 0.05 and len(m.pool.activations) >= 6


def test_defaults_at_44100_with_a_start_time():
    m, out, st, g, v = _run(dict(), [MF] * 6, exact=True, sr=44100, start=300)
    assert st["max_n"] == 1 and st["peak"] > 0.05 and (out.reshape(-1, 2)[:300] == 0).all() and len(m.pool.activations) == 2


def test_cloud_fills_the_pool():
    """100 concurrent grains (slots in both waves' lanes), failed activations, random directions, a moving playhead."""
    m, out, st, g, v = _run(CLOUD, [MF] * 9)
    assert st["max_n"] >= 90 and m.pool.failed_activations >= 1 and m.pool.active.sum() >= 99 and st["peak"] > 0.3
    assert (m.pool.increment < 0).any() and (m.pool.increment > 0).any()


@pytest.mark.parametrize("window", range(8), ids=gm.WINDOWS)
def test_windows(window):
    m, out, st, g, v = _run(dict(window=window, size=20.0, density=60.0, variation=0.5), [MF, 517])
    assert st["max_n"] >= 2 and st["peak"] > 0.02


@pytest.mark.parametrize("window", [0, 4], ids=["Hann", "Trapezoid"])
def test_sequential(window):
    m, out, st, g, v = _run(dict(overlap_mode=gm.SEQUENTIAL, window=window, size=50.0, variation=0.7), [MF, MF, 333])
    assert st["max_n"] >= 2 and len(m.pool.activations) >= 4 and m.pool.primary >= 0   # (sizes vary: an old long grain may outlive its successor)


def test_sequential_shortest_grains_reuse_a_slot_inside_a_tile():
    m, out, st, g, v = _run(dict(overlap_mode=gm.SEQUENTIAL, window=2, size=1.0, variation=1.0), [257, 64])
    assert len(m.pool.activations) >= 30


@pytest.mark.parametrize("step,position,direction", [(2.0, 0.1, gm.FORWARD), (-2.0, 0.9, gm.BACKWARD)], ids=["forward", "backward"])
def test_loop_range(step, position, direction):
    """The playhead enters (0.25, 0.75) from either side and folds; grains activated inside carry the range."""
    m, out, st, g, v = _run(dict(loop_range=(0.25, 0.75), step=step, position=position, density=50.0, size=40.0, playback_direction=direction), [MF] * 3)
    assert m.pool.playing_loop_range and m.pool.has_loop.any() and 0.25 <= float(m.pool.playhead) < 0.75


def test_backward_grains_cross_zero():
    m, out, st, g, v = _run(dict(playback_direction=gm.BACKWARD, position=0.01, size=200.0, density=20.0), [MF] * 2, speed=2.0)
    assert (m.pool.position[m.pool.active] > 0.5).any()      # wrapped from below 0 to the end of the buffer


def test_grains_pass_one():
    m, out, st, g, v = _run(dict(position=0.99, size=200.0, density=20.0), [MF] * 2, speed=2.0)
    assert (m.pool.position[m.pool.active] < 0.5).any()


def test_one_frame_buffer():
    m, out, st, g, v = _run(dict(density=50.0), [MF], buf=np.array([0.625], dtype=np.float32))
    assert st["peak"] > 0.1                                    # max_index == 0: every read is frame 0


@pytest.mark.parametrize("sizes", [[1] * 40 + [7] * 20 + [64] * 4 + [256] * 2 + [76], [1024]], ids=["pieces", "one"])
def test_write_sizes(sizes):
    """Writes of 1, 7, 64 and 256 frames, 1024 frames in all, against one 1024-frame write: the same state after the last write (both equal the
    model's), outputs inside the bound."""
    assert sum(sizes) == 1024
    _run(dict(density=100.0, size=60.0, variation=1.0, spray=0.5, pan_spread=1.0, playback_direction=gm.RANDOM, step=0.5), sizes)


def test_super_block_write_against_per_block_writes():
    kw = dict(density=80.0, size=80.0, variation=0.6, pan_spread=0.5)
    g = Graph(SR, 2, 256, 0)
    g.set_max_blocks_per_launch(8)
    _, a, _, _, _ = _run(kw, [2048, 2048], mf=256, graph=g)
    _, b, _, _, _ = _run(kw, [256] * 16, mf=256)
    assert np.array_equal(a, b)                                # the same slot order of the sum either way


def test_commands_inside_a_block():
    """Volume, panning and speed at frames inside a block: running grains keep their values, grains activated from that frame on take the new ones."""
    cmds = [(300, "volume", 0.25), (300, "panning", -0.5), (700, "speed", 2.0), (1500, "volume", 0.9), (1500, "panning", 0.75)]
    m, out, st, g, v = _run(dict(density=50.0, size=100.0), [MF] * 2, cmds=cmds, volume=0.8, panning=0.2)
    vols = {float(x) for x in m.pool.volume_g[:6]}
    assert {0.25, float(np.float32(0.9))} <= vols and (m.pool.increment[:6] == 2.0 / 2048.0).all() and len(m.pool.activations) >= 12


def test_stop_inside_a_block():
    """GrainPool::stop() at frame 1234: no new grains; the voice ends with the write in which the last grain ran out, and writes that write in full."""
    m, out, st, g, v = _run(dict(density=80.0, size=100.0, variation=1.0), [MF] * 4, cmds=[(1234, "stop", None)], volume=0.7, panning=-0.3)
    assert m.ended and m.t == 4 * MF and not m.pool.trigger_new_grains
    last = int(np.flatnonzero(np.abs(out.reshape(-1, 2)).sum(axis=1))[-1])
    assert 1234 < last < 4 * MF - 1


def test_release_without_envelope_is_the_pools_stop():
    m, out, st, g, v = _run(dict(density=80.0, size=100.0), [MF] * 3, cmds=[(777, "release", None)])
    assert m.ended and not m.pool.trigger_new_grains and len(m.pool.activations) == sum(1 for f, _ in m.pool.activations if f < 777)


ENV = dict(attack_s=0.02, hold_s=0.03, decay_s=0.05, sustain_level=0.6, release_s=0.04)


def test_envelope_release_ends_the_voice_on_idle():
    m, out, st, g, v = _run(dict(), [MF] * 3, exact=True, env=ENV, cmds=[(1400, "release", None)])
    assert m.ended and m.pool.trigger_new_grains and m.env.stage == A.IDLE and st["peak"] > 0.02
    assert g.voice_envelope_stage(v) == A.IDLE


def test_envelope_whose_release_outlasts_the_pool():
    env = dict(ENV, release_s=2.0)
    m, out, st, g, v = _run(dict(), [MF] * 4, exact=True, env=env, cmds=[(1400, "release", None), (1400, "stop", None)])
    assert m.ended and m.env.stage == A.RELEASE and m.pool.is_exhausted()
    assert g.voice_envelope_stage(v) == A.RELEASE


def test_under_a_sub_mixer_with_a_filter():
    """The granular voice under a sub-mixer with a Filter = the model's output as a host-fed voice through the same chain (the tolerance of
    tests/test_gpu_effects.py: 1e-5 RMS, 1e-4 max)."""
    kw = dict(density=60.0, size=80.0, variation=0.5, pan_spread=0.6)
    n_blocks = 4
    g = Graph(SR, 2, MF, 0)
    mx = g.add_mixer()
    g.add_effect(mx, _capi.FX_FILTER, {"cuto": 1200.0})
    m = Model(kw)
    v = _add(g, mx, m)
    r = Graph(SR, 2, MF, 0)
    rx = r.add_mixer()
    r.add_effect(rx, _capi.FX_FILTER, {"cuto": 1200.0})
    rv = r.add_stream_voice(rx, 2, SR, 8192)
    pos = 0
    for k in range(n_blocks):
        exp, cnt, S = m.write(MF)
        r.feed_voice(rv, exp.reshape(-1))
        a, b = np.zeros(2 * MF, np.float32), np.zeros(2 * MF, np.float32)
        g.write(a, pos), r.write(b, pos)
        r.stream_voice_consumed(rv)
        d = a.astype(np.float64) - b.astype(np.float64)
        assert np.abs(b).max() > 0.01
        assert float(np.sqrt(np.mean(d * d))) <= 1e-5 and float(np.abs(d).max()) <= 1e-4, (k, float(np.abs(d).max()))
        assert gm.states_equal(m.pool.state(), g.voice_grain_state(v)) == []
        pos += MF
    assert g.device_errors() == 0


def test_file_voice_beside_a_granular_voice():
    """One file voice plus one granular voice on the main mixer = the file voice alone + the granular voice alone (f32 sum of the two units)."""
    tone = (0.4 * np.sin(2 * np.pi * 220.0 * np.arange(4 * MF + 64) / SR)).astype(np.float32)
    kw = dict(density=40.0, size=120.0)
    both, alone = Graph(SR, 2, MF, 0), Graph(SR, 2, MF, 0)
    both.add_voice(0, np.repeat(tone, 2), 2, SR)
    alone.add_voice(0, np.repeat(tone, 2), 2, SR)
    m = Model(kw)
    v = _add(both, 0, m)
    pos = 0
    for k in range(4):
        a, b = np.zeros(2 * MF, np.float32), np.zeros(2 * MF, np.float32)
        both.write(a, pos), alone.write(b, pos)
        exp, cnt, S = m.write(MF)
        want = (b.reshape(-1, 2) + exp).astype(np.float32)
        tol = 2.0 * cnt[:, None] * 2.0 ** -23 * S + 2.0 ** -23 * np.abs(want)      # + one rounding of the sum of the two units
        assert (np.abs(a.reshape(-1, 2).astype(np.float64) - want) <= tol).all(), k
        assert gm.states_equal(m.pool.state(), both.voice_grain_state(v)) == []
        pos += MF
    assert both.device_errors() == 0


def test_two_granular_voices_with_different_seeds():
    g = Graph(SR, 2, MF, 0)
    mx = g.add_mixer()
    kw = dict(density=70.0, size=60.0, variation=1.0, spray=1.0, pan_spread=1.0)
    seeds = [(1, 2, 3, 4), (5, 6, 7, 8)]
    ms = [Model(kw, rng=s) for s in seeds]
    vs = [_add(g, mx, m, rng=s) for m, s in zip(ms, seeds)]
    pos = 0
    for k in range(3):
        a = np.zeros(2 * MF, np.float32)
        g.write(a, pos)
        r = [m.write(MF) for m in ms]
        want = (r[0][0] + r[1][0]).astype(np.float32)
        tol = sum(2.0 * c[:, None] * 2.0 ** -23 * s for _, c, s in r) + 2.0 ** -23 * np.abs(want)
        assert (np.abs(a.reshape(-1, 2).astype(np.float64) - want) <= tol).all(), k
        for m, v in zip(ms, vs):
            assert gm.states_equal(m.pool.state(), g.voice_grain_state(v)) == []
        pos += MF
    assert ms[0].pool.rng.s != ms[1].pool.rng.s and g.device_errors() == 0


def test_sharded_equals_single():
    """One sub-mixer per shard, a granular voice in each (one enveloped and released): the sharded handle = the plain graph, bit for bit — both
    add the bus in the same order, (0 + m1) + m2 against (0 + m1) + (0 + m2) — and the grain state is forwarded to the voice's shard."""
    def build(g):
        ids, ms = [], []
        for i in range(2):
            mx = g.add_mixer()
            g.add_effect(mx, _capi.FX_GAIN, {"gain": 0.9})
            m = Model(dict(density=50.0 + 20 * i, size=70.0, variation=0.8, pan_spread=1.0), rng=(9 + i, 8, 7, 6), env=ENV if i == 0 else None,
                      cmds=[(1500, "release", None)] if i == 0 else [(900, "volume", 0.5)])
            ids.append(_add(g, mx, m, rng=(9 + i, 8, 7, 6)))
            ms.append(m)
        return g, ids, ms

    single, sid, _ = build(Graph(SR, 2, MF, 0))
    sharded, hid, ms = build(ShardedGraph([0, 0], SR, 2, MF))
    assert sharded.shard_of_mixer(1) != sharded.shard_of_mixer(2)
    pos = 0
    for k in range(3):
        a, b = np.zeros(2 * MF, np.float32), np.zeros(2 * MF, np.float32)
        single.write(a, pos), sharded.write(b, pos)
        assert np.array_equal(a, b) and np.abs(a).max() > 0.01, k
        for m, v, w in zip(ms, sid, hid):
            m.write(MF)
            assert gm.states_equal(m.pool.state(), sharded.voice_grain_state(w)) == [] and gm.states_equal(m.pool.state(), single.voice_grain_state(v)) == []
        pos += MF
    assert not sharded.is_voice_playing(hid[0]) and sharded.is_voice_playing(hid[1]) and sharded.device_errors() == 0


def test_errors():
    g = Graph(SR, 2, MF, 0)
    m = Model(dict())
    v = _add(g, 0, m)
    lib = _capi.load()
    assert lib.pg_graph_seek_voice(g._h, v, 0.5, 0) == _capi.PG_ERR_STATE
    import ctypes as C
    buf = m.buf
    for kw in (dict(size=0.5), dict(density=101.0), dict(step=4.5), dict(loop_range=(0.2, 1.5))):
        p = _capi.granular_params(**kw)
        assert lib.pg_graph_add_granular_voice(g._h, 0, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, C.byref(p), None) == -_capi.PG_ERR_PARAMETER
    p = _capi.granular_params()
    assert lib.pg_graph_add_granular_voice(g._h, 0, buf.ctypes.data_as(C.POINTER(C.c_float)), 0, C.byref(p), None) == -_capi.PG_ERR_PARAMETER
    f = g.add_voice(0, np.zeros(256, np.float32), 2, SR)
    st = _capi.GrainState()
    assert lib.pg_graph_voice_grain_state(g._h, f, C.byref(st)) == _capi.PG_ERR_NOT_FOUND
    out = np.zeros(2 * MF, np.float32)
    g.write(out, 0)
    exp, cnt, S = m.write(MF)
    assert np.array_equal(out.reshape(-1, 2), exp + np.float32(0.0)) and g.device_errors() == 0


def test_a_finished_voice_leaves_the_exact_kernel():
    """The unit of a granular voice is rendered by the exact kernel while the voice lives and returns to its own kernel once pg_grain_kernel has
    reported the end."""
    g = Graph(SR, 2, MF, 0)
    tone = (0.2 * np.sin(2 * np.pi * 330.0 * np.arange(16 * MF + 64) / SR)).astype(np.float32)
    mx = g.add_mixer()
    g.add_voice(mx, np.repeat(tone, 2), 2, SR)
    m = Model(dict(), cmds=[(1500, "stop", None)])
    v = _add(g, mx, m)
    deferred, pos = [], 0
    for k in range(10):
        out = np.zeros(2 * MF, np.float32)
        g.write(out, pos)
        deferred.append(g.deferred_units())
        pos += MF
    assert max(deferred[:3]) == 1 and deferred[-1] == 0, deferred
    assert not g.is_voice_playing(v) and g.device_errors() == 0
