"""The modulation matrix of granular voices on the GPU (pg_graph_set_voice_modulation_matrix and its timed calls, phase 0 of pg_grain_kernel)
against the independent numpy model of the reference's matrix and modulated grain pool (tests/modulation_model.py: src/modulation/matrix.rs,
src/utils/dsp/lfo.rs, src/generator/sampler/modulation.rs, src/generator/sampler/granular.rs). Everything goes through the C ABI.

In the shape of tests/test_gpu_granular.py: 8000 Hz, the 2048-frame seeded buffer, the same pool RNG state. After EVERY write:
  grain state   pg_graph_voice_grain_state equals the model bit for bit. trigger_phase and playhead are f32 recurrences that take density_mod
                and speed_mod every frame, the draws and the grains' fields take the other five: one wrong modulation value at any frame shows here
                (tests/test_modulation_model.py::test_every_input_shows_in_the_state checks that on the CPU for these parameters);
  matrix state  pg_graph_voice_modulation_state equals the model bit for bit: LFO phases, increments, held random values, generator states,
                the 4 x 7 routes and the seven sums of the last rendered frame;
  output        within the derived bound 2 n 2^-23 S per frame and channel of tests/test_gpu_granular.py, bit-equal where n <= 1.
The model's process calls are cut where the device's are: at the ends of the writes, on the 4096-frame chunk grid, at the voice's events (the
matrix's timed calls are events of its mixer like a volume command) and at its start time."""
import ctypes as C

import numpy as np
import pytest

import granular_model as gm
import modulation_model as mm
from phonic_amd import _capi
from phonic_amd.graph import Graph, ShardedGraph

pytestmark = pytest.mark.gpu

SR = 8000
MF = 1024
RNG = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444)
LFO_RNG = ((0xA5A5A5A5DEADBEEF, 2, 3, 4), (5, 6, 0xC0FFEE1234567890, 8))
# every target matters: Cloud (density), a moving playhead (step), room for the additive sums on both sides
BASE = dict(density=50.0, size=60.0, variation=0.3, spray=0.3, pan_spread=0.3, step=1.0, position=0.2, playback_direction=gm.RANDOM)
LOOPED = dict(BASE, loop_range=(0.25, 0.75))
TILE_EDGES = [1, 31, 32, 33, 64, 1887]     # 2048 frames; the kernel's tile is 32 frames
AMOUNTS = [1.0, -1.0, 0.37]
ALL_ROUTES = [(s, t, AMOUNTS[(s + t) % 3], (s * 7 + t) % 2 == 0) for s in range(4) for t in range(7)]
TARGETS = ["size", "density", "variation", "spray", "pan_spread", "position", "step"]
SOURCES = ["lfo1", "lfo2", "velocity", "keytrack"]


class Model:
    """The voice as the model renders it. cmds: (frame, name, args) with name in route (source, target, amount, bipolar) / clear (source, target)
    / rate (lfo, hz) / waveform (lfo, shape) / volume (value)."""

    def __init__(self, kw, matrix=None, start=0, cmds=(), volume=1.0):
        self.buf = gm.make_buffer(2048)
        self.mkw = matrix
        if matrix is None:
            self.pool = gm.GrainPool(SR, self.buf, gm.Params(**kw), RNG, 1.0, volume, 0.0)
        else:
            self.pool = mm.ModGrainPool(SR, self.buf, gm.Params(**kw), mm.make_matrix(SR, **matrix), RNG, 1.0, volume, 0.0)
        self.start, self.cmds, self.volume = start, sorted(cmds, key=lambda c: c[0]), volume
        self.t = 0
        self.ended = False

    def _apply(self, t):
        for (ct, name, a) in self.cmds:
            if ct != t:
                continue
            if name == "route":
                self.pool.matrix.set_modulation(*a)
            elif name == "clear":
                self.pool.matrix.clear_modulation(*a)
            elif name == "rate":
                self.pool.matrix.set_lfo_rate(*a)
            elif name == "waveform":
                self.pool.matrix.set_lfo_waveform(*a)
            elif name == "volume":
                self.pool.set_volume(*a)

    def write(self, n):
        t0, t1 = self.t, self.t + n
        cuts = {t1} | {t0 + k for k in range(4096, n, 4096)} | {ct for (ct, _, _) in self.cmds if t0 < ct < t1}
        if t0 < self.start < t1:
            cuts.add(self.start)
        out, cnt, S = np.zeros((n, 2), np.float32), np.zeros(n, np.int64), np.zeros((n, 2))
        a = t0
        for b in sorted(cuts):
            self._apply(a)
            if not self.ended and b > self.start:
                out[a - t0:b - t0], cnt[a - t0:b - t0], S[a - t0:b - t0] = self.pool.process(b - a)
                self.ended = self.pool.is_exhausted()
            a = b
        self.t = t1
        return out, cnt, S


def _add(g, mixer, m):
    p = m.pool.p
    gp = _capi.granular_params(loop_range=p.loop_range, rng_state=RNG, overlap_mode=p.overlap_mode, window=p.window, size=p.size, density=p.density,
                               variation=p.variation, spray=p.spray, pan_spread=p.pan_spread, playback_direction=p.playback_direction, position=p.position, step=p.step)
    v = g.add_granular_voice(mixer, m.buf, gp, volume=m.volume, start_time=m.start)
    if m.mkw is not None:
        g.set_voice_modulation_matrix(v, **m.mkw)
    for (t, name, a) in m.cmds:
        if name == "route":
            g.set_voice_modulation(v, a[0], a[1], a[2], a[3], t)
        elif name == "clear":
            g.clear_voice_modulation(v, a[0], a[1], t)
        elif name == "rate":
            g.set_voice_lfo_rate(v, a[0], a[1], t)
        elif name == "waveform":
            g.set_voice_lfo_waveform(v, a[0], a[1], t)
        elif name == "volume":
            g.set_voice_volume(v, a[0], t)
    return v


def _check_write(g, v, m, got, exp, cnt, S, tag):
    exp = exp + np.float32(0.0)   # the mixer ADDS the voice into its zeroed block: 0.0 + -0.0 = +0.0
    got, bound = got.reshape(-1, 2), 2.0 * cnt[:, None] * 2.0 ** -23 * S
    st = g.voice_grain_state(v)
    assert gm.states_equal(m.pool.state(), st) == [], (tag, "grain state", gm.states_equal(m.pool.state(), st))
    if m.mkw is not None:
        ms = g.voice_modulation_state(v)
        assert gm.states_equal(m.pool.matrix.state(), ms) == [], (tag, "matrix state", gm.states_equal(m.pool.matrix.state(), ms))
    diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    bad = np.flatnonzero((diff > bound).any(axis=1))
    assert len(bad) == 0, (tag, "output", int(bad[0]), float(diff.max()), int(cnt[bad[0]]))
    one = cnt <= 1
    assert np.array_equal(got[one].view(np.uint32), exp[one].view(np.uint32)), (tag, "frames with at most one grain are bit-equal")
    assert g.is_voice_playing(v) == (not m.ended), (tag, "playing", m.ended)


def _run(kw, sizes, graph=None, mixer=0, **mkw):
    """mixer "sub": the voice sits on a sub-mixer without effects. An event of the MAIN mixer ends the main chunk, so a command of a main-mixer
    voice always reaches pg_grain_kernel at frame 0 of a launch; a sub-mixer's event stays inside the piece (frame = time - piece start) and
    reaches the kernel in the middle of a launch and of a tile."""
    m = Model(kw, **mkw)
    g = graph or Graph(SR, 2, MF, 0)
    if mixer == "sub":
        mixer = g.add_mixer()
    v = _add(g, mixer, m)
    pos, outs, peak = 0, [], 0.0
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        exp, cnt, S = m.write(n)
        _check_write(g, v, m, buf, exp, cnt, S, (k, pos))
        peak = max(peak, float(np.abs(exp).max()))
        pos += n
        outs.append(buf)
    assert g.device_errors() == 0 and peak > 0.02
    return m, np.concatenate(outs), g, v


# ---- 1: one route at a time ----
@pytest.mark.parametrize("bipolar", [0, 1], ids=["unipolar", "bipolar"])
@pytest.mark.parametrize("target", range(7), ids=TARGETS)
@pytest.mark.parametrize("source", range(4), ids=SOURCES)
def test_one_route(source, target, bipolar):
    amount = AMOUNTS[(source + target + bipolar) % 3]
    matrix = dict(rates=(20.0, 20.0), rng_states=LFO_RNG, velocity=0.8, note=72, routes=[(source, target, amount, bool(bipolar))])
    m, out, g, v = _run(BASE, TILE_EDGES, matrix=matrix)
    mx = m.pool.matrix
    assert mx.has_route(source, target) and mx.amount.astype(bool).sum() == 1 and mx.last[target] != 0 and not np.delete(mx.last, target).any()
    assert len(m.pool.activations) >= 3 and mx.lfos[0].phase != 0     # 20 Hz: five wraps in 2048 frames


# ---- 2: all 28 routes at once, both LFOs on every waveform ----
@pytest.mark.parametrize("overlap", [gm.CLOUD, gm.SEQUENTIAL], ids=["cloud", "sequential"])
@pytest.mark.parametrize("waveform", range(7), ids=_capi.LFO_WAVEFORMS)
def test_all_routes(waveform, overlap):
    """A loop range and step 1.0: position_mod passes the loop fold, speed_mod drives the playhead into the loop."""
    matrix = dict(rates=(20.0, 13.0), waveforms=(waveform, (waveform + 3) % 7), rng_states=LFO_RNG, velocity=0.8, note=72, routes=ALL_ROUTES)
    m, out, g, v = _run(dict(LOOPED, overlap_mode=overlap), TILE_EDGES, matrix=matrix)
    assert m.pool.playing_loop_range and m.pool.matrix.last.all() and len(m.pool.activations) >= 3


# ---- 3: the random shapes ----
@pytest.mark.parametrize("waveform", [mm.RANDOM, mm.SMOOTH_RANDOM], ids=["Random", "SmoothRandom"])
def test_random_shapes_with_a_seed(waveform):
    """The draws of Lfo::new, of the reset at note-on and of every wrap are the model's; the other LFO keeps the default seed (all-zero state)."""
    matrix = dict(rates=(20.0, 17.0), waveforms=(waveform, mm.RANDOM), rng_states=(LFO_RNG[0], None), velocity=0.6, note=40,
                  routes=[(0, mm.POSITION, 0.37, True), (0, mm.DENSITY, 1.0, True), (1, mm.SIZE, -1.0, False), (1, mm.STEP, 1.0, True)])
    m, out, g, v = _run(BASE, TILE_EDGES, matrix=matrix)
    l0, l1 = m.pool.matrix.lfos
    assert l0.draws == 3 + 2 + 2 * 5 and l1.draws == 3 + 2 + 2 * 4    # Lfo::new, reset, the wraps of 2048 frames at 20 / 17 Hz


def test_waveform_becomes_random_by_a_timed_command():
    """The reset at note-on did not redraw (the shape was Sine): the held value is the construction draw until the first wrap."""
    matrix = dict(rates=(20.0, 2.0), rng_states=LFO_RNG, routes=[(0, mm.STEP, 1.0, True), (0, mm.PAN_SPREAD, 0.37, False)])
    m = Model(BASE, matrix=matrix, cmds=[(100, "waveform", (0, mm.RANDOM))])
    construction_draw = m.pool.matrix.lfos[0].sample_hold
    g = Graph(SR, 2, MF, 0)
    v = _add(g, 0, m)
    pos = 0
    for k, n in enumerate([300, 99, 1649]):       # the first wrap of a 20 Hz LFO is at frame 399
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        _check_write(g, v, m, buf, *m.write(n), (k, pos))
        if k == 0:
            assert m.pool.matrix.last[mm.STEP] == construction_draw and m.pool.matrix.lfos[0].draws == 3
        pos += n
    assert m.pool.matrix.lfos[0].draws == 3 + 2 * 5 and g.device_errors() == 0


# ---- 4: timed commands ----
# The voices sit on a sub-mixer (see _run): the commands reach the kernel inside a launch, at the tile frames named below. Writes begin at
# multiples of the piece size or at 500, a piece begins with its write, tiles are 32 frames from the piece's start.
def _timed(at, extra=()):
    return [(at, "route", (0, mm.DENSITY, 1.0, True)), (at, "route", (2, mm.STEP, -1.0, True)), (at, "rate", (0, 7.5)), (at, "waveform", (1, mm.SQUARE))] + list(extra)


PLACES = {"first_frame_of_a_write": 500, "last_frame_of_a_write": 1199, "tile_frame_0": 500 + 64, "tile_frame_31": 500 + 31, "tile_frame_32": 500 + 32,
          "tile_frame_33": 500 + 33, "with_a_volume_command": 777}


@pytest.mark.parametrize("mixer", ["sub", 0], ids=["sub_mixer", "main_mixer"])
@pytest.mark.parametrize("where", list(PLACES))
def test_timed_commands(where, mixer):
    """A route set, changed and cleared, an LFO rate and an LFO waveform: each acts in front of its frame, wherever that frame sits in a write,
    a piece or a tile (sub-mixer), or at the first frame of a launch (main mixer: its events end the chunk)."""
    sizes = [500, 700, 848]
    at = PLACES[where]
    cmds = _timed(at, [(777, "volume", (0.5,))] if where == "with_a_volume_command" else [])
    cmds += [(at + 200, "route", (0, mm.DENSITY, -0.37, False)), (at + 200, "route", (1, mm.SPRAY, 0.0009, True)), (at + 200, "route", (3, mm.SIZE, 1.0, False)),
             (at + 431, "clear", (0, mm.DENSITY)), (at + 431, "route", (3, mm.SIZE, -0.0009, True)), (at + 431, "rate", (1, 500.0))]
    matrix = dict(rates=(20.0, 20.0), rng_states=LFO_RNG, velocity=0.8, note=72, routes=[(1, mm.POSITION, 0.37, True)])
    m, out, g, v = _run(BASE, sizes, mixer=mixer, matrix=matrix, cmds=cmds)
    mx = m.pool.matrix
    assert not mx.has_route(0, mm.DENSITY) and not mx.has_route(3, mm.SIZE) and not mx.has_route(1, mm.SPRAY) and mx.has_route(2, mm.STEP)
    assert mx.lfos[0].phase_inc == np.float32(7.5 / SR) and mx.lfos[1].phase_inc == np.float32(20.0 / SR) and mx.lfos[1].waveform == mm.SQUARE


@pytest.mark.parametrize("mixer", ["sub", 0], ids=["sub_mixer", "main_mixer"])
def test_timed_commands_behind_the_chunk_edge(mixer):
    """A 5000-frame write is rendered as chunks of 4096 + 904 frames (pieces of 1024): commands at frame 4096 + 500, and two at the edge itself."""
    cmds = _timed(4596) + [(4096, "route", (1, mm.VARIATION, 1.0, False)), (4096, "rate", (1, 3.0)), (4800, "clear", (2, mm.STEP))]
    matrix = dict(rates=(20.0, 20.0), rng_states=LFO_RNG, velocity=0.8, note=72, routes=[(1, mm.POSITION, 0.37, True)])
    m, out, g, v = _run(BASE, [5000], mixer=mixer, matrix=matrix, cmds=cmds)
    assert m.pool.matrix.has_route(1, mm.VARIATION) and not m.pool.matrix.has_route(2, mm.STEP)


def _one_tile_commands(t0):
    """Commands on frames t0 .. t0 + 29, t0 the first frame of a tile: ten route commands three frames apart, two more on one frame for the same route
    (the later one holds), a clear, and both LFOs' rate and waveform in the same tile."""
    cmds = [(t0 + k, "route", (k % 4, (3 * k) % 7, AMOUNTS[k % 3], k % 2 == 0)) for k in range(0, 30, 3)]
    cmds += [(t0 + 12, "route", (0, mm.STEP, 0.5, True)), (t0 + 12, "route", (0, mm.STEP, -0.25, False)), (t0 + 13, "clear", (0, mm.SIZE))]
    cmds += [(t0 + 5, "rate", (0, 3.0)), (t0 + 12, "waveform", (0, mm.RANDOM)), (t0 + 13, "waveform", (1, mm.SMOOTH_RANDOM)), (t0 + 20, "rate", (1, 19.0)), (t0 + 31, "waveform", (0, mm.SINE))]
    return cmds


@pytest.mark.parametrize("t0", [1024 + 32, 64, 1024 + 992], ids=["second_tile_of_a_piece", "third_tile_of_a_write", "last_tile_of_a_piece"])
def test_many_commands_in_one_tile(t0):
    """Several segments inside ONE 32-frame tile of a launch (the voice is a sub-mixer's): the tile's sums are cut at every route command, the LFO
    lanes take rate and waveform between two frames of their walk."""
    matrix = dict(rates=(20.0, 11.0), rng_states=LFO_RNG, velocity=0.8, note=72, routes=[(0, mm.SIZE, 1.0, True)])
    m, out, g, v = _run(BASE, [2048], mixer="sub", matrix=matrix, cmds=_one_tile_commands(t0))
    mx = m.pool.matrix
    assert mx.amount[0, mm.STEP] == np.float32(-0.25) and mx.amount.astype(bool).sum() >= 8 and mx.lfos[1].waveform == mm.SMOOTH_RANDOM


def test_more_commands_than_the_kernels_list_holds():
    """More than 64 commands of the voice in one piece: every lane then walks the launch's own command list. 90 route commands five frames apart,
    LFO commands between them, a volume command among them."""
    cmds = [(40 + 5 * k, "route", (k % 4, (5 * k) % 7, AMOUNTS[k % 3] if k % 11 else 0.0, k % 2 == 1)) for k in range(90)]
    cmds += [(43 + 50 * k, "rate", (k % 2, 1.0 + 2.0 * k)) for k in range(8)] + [(61 + 70 * k, "waveform", (k % 2, (2 * k + 1) % 7)) for k in range(6)]
    cmds += [(222, "volume", (0.6,))]
    matrix = dict(rates=(20.0, 11.0), rng_states=LFO_RNG, velocity=0.8, note=72, routes=[(0, mm.SIZE, 1.0, True)])
    m, out, g, v = _run(BASE, [1024, 512], mixer="sub", matrix=matrix, cmds=cmds)
    assert len(cmds) > 64 + 30 and m.pool.matrix.amount.astype(bool).sum() >= 12


def test_a_voice_with_a_matrix_ends():
    """GrainPool::stop() at frame 1234: the voice ends with the write in which its last grain ran out. The matrix advanced through that write and
    not beyond it: phases, generator states and `last` stay what they were when the voice ended."""
    matrix = dict(rates=(20.0, 13.0), waveforms=(mm.SMOOTH_RANDOM, mm.SINE), rng_states=LFO_RNG, velocity=0.8, note=72, routes=ALL_ROUTES)
    m = Model(dict(BASE, size=100.0), matrix=matrix)
    g = Graph(SR, 2, MF, 0)
    v = _add(g, 0, m)
    g.stop_voice(v, 1234)
    pos, ended_at = 0, None
    for k in range(5):
        buf = np.zeros(2 * MF, dtype=np.float32)
        g.write(buf, pos)
        if pos <= 1234 < pos + MF:      # (a stop is a message, not an event: the model's call is cut there by hand)
            o1, o2 = m.write(1234 - pos), None
            m.pool.stop()
            o2 = m.write(pos + MF - 1234)
            exp = tuple(np.concatenate([a, b]) for a, b in zip(o1, o2))
        else:
            exp = m.write(MF)
        _check_write(g, v, m, buf, *exp, (k, pos))
        if m.ended and ended_at is None:
            ended_at = k
            frozen = m.pool.matrix.state()
        pos += MF
    assert ended_at is not None and ended_at < 4 and gm.states_equal(frozen, g.voice_modulation_state(v)) == [] and g.device_errors() == 0


# ---- 5: a start time in the middle of a write ----
def test_start_time_inside_a_write():
    """Frames in front of the start time produce nothing and advance nothing: the LFO phases read 0 until then; a route command in front of the
    start still reaches the matrix."""
    matrix = dict(rates=(20.0, 13.0), rng_states=LFO_RNG, velocity=0.8, note=72, routes=ALL_ROUTES)
    m = Model(BASE, matrix=matrix, start=45 + 64, cmds=[(20, "route", (0, mm.DENSITY, -1.0, False))])
    g = Graph(SR, 2, MF, 0)
    v = _add(g, 0, m)
    pos = 0
    for k, n in enumerate([64, 500, 1484]):       # the start is frame 45 of the second write
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        _check_write(g, v, m, buf, *m.write(n), (k, pos))
        if k == 0:
            ms = g.voice_modulation_state(v)
            assert ms["lfo0_phase"] == 0 and ms["lfo1_phase"] == 0 and not ms["last"].any() and ms["amount"][0, mm.DENSITY] == np.float32(-1.0)
        if k == 1:
            assert not buf.reshape(-1, 2)[:45].any() and m.pool.frame == 500 - 45
        pos += n
    assert g.device_errors() == 0


# ---- 6: no routes ----
def test_empty_matrix_equals_no_matrix():
    """`x + 0.0` and `x * (1.0 + 0.0)`: output and grain state bit-equal to the same voice without a matrix, while the LFOs run."""
    with_matrix, without = Graph(SR, 2, MF, 0), Graph(SR, 2, MF, 0)
    ma, mb = Model(LOOPED, matrix=dict()), Model(LOOPED)
    va, vb = _add(with_matrix, 0, ma), _add(without, 0, mb)
    pos = 0
    for k, n in enumerate(TILE_EDGES):
        a, b = np.zeros(2 * n, np.float32), np.zeros(2 * n, np.float32)
        with_matrix.write(a, pos), without.write(b, pos)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
        assert gm.states_equal(with_matrix.voice_grain_state(va), without.voice_grain_state(vb)) == []
        _check_write(with_matrix, va, ma, a, *ma.write(n), (k, pos))
        pos += n
    ms = with_matrix.voice_modulation_state(va)
    assert ms["lfo0_phase"] != 0 and ms["lfo0_phase_inc"] == np.float32(1.0 / SR) and ms["lfo1_waveform"] == mm.TRIANGLE and not ms["last"].any()
    assert ms["velocity"] == 1.0 and ms["note_pitch"] == np.float32(60.0) / np.float32(127.0) and np.abs(a).max() > 0.01
    assert with_matrix.device_errors() == 0 and without.device_errors() == 0


# ---- 7: error paths ----
def test_errors():
    lib = _capi.load()
    g = Graph(SR, 2, MF, 0)
    m = Model(BASE, matrix=dict(routes=[(0, mm.SIZE, 0.5, True)]))
    v = _add(g, 0, m)
    plain = g.add_granular_voice(0, m.buf, _capi.granular_params())
    f = g.add_voice(0, np.zeros(256, np.float32), 2, SR)
    p = _capi.modulation_params()
    st = _capi.ModulationState()
    assert lib.pg_graph_set_voice_modulation_matrix(g._h, f, C.byref(p)) == _capi.PG_ERR_NOT_FOUND          # a file voice
    assert lib.pg_graph_set_voice_modulation_matrix(g._h, 99, C.byref(p)) == _capi.PG_ERR_NOT_FOUND
    assert lib.pg_graph_voice_modulation_state(g._h, f, C.byref(st)) == _capi.PG_ERR_NOT_FOUND
    assert lib.pg_graph_voice_modulation_state(g._h, plain, C.byref(st)) == _capi.PG_ERR_STATE
    for voice in (plain, f):                                                                                # timed calls without a matrix
        assert lib.pg_graph_set_voice_modulation(g._h, voice, 0, 0, 0.5, 1, 0) == _capi.PG_ERR_STATE
        assert lib.pg_graph_clear_voice_modulation(g._h, voice, 0, 0, 0) == _capi.PG_ERR_STATE
        assert lib.pg_graph_set_voice_lfo_rate(g._h, voice, 0, 5.0, 0) == _capi.PG_ERR_STATE
        assert lib.pg_graph_set_voice_lfo_waveform(g._h, voice, 1, 2, 0) == _capi.PG_ERR_STATE
    assert lib.pg_graph_set_voice_modulation(g._h, 99, 0, 0, 0.5, 1, 0) == _capi.PG_ERR_NOT_FOUND
    assert lib.pg_graph_set_voice_modulation(g._h, v, 0, 0, 1.5, 1, 0) == _capi.PG_ERR_PARAMETER             # amount 1.5
    assert lib.pg_graph_set_voice_modulation(g._h, v, 4, 0, 0.5, 1, 0) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_set_voice_lfo_waveform(g._h, v, 0, 7, 0) == _capi.PG_ERR_PARAMETER
    out = np.zeros(2 * MF, np.float32)
    g.write(out, 0)
    assert lib.pg_graph_set_voice_modulation_matrix(g._h, v, C.byref(p)) == _capi.PG_ERR_STATE              # after the first write
    assert lib.pg_graph_set_voice_modulation_matrix(g._h, plain, C.byref(p)) == _capi.PG_ERR_STATE
    m.write(MF)
    assert gm.states_equal(m.pool.state(), g.voice_grain_state(v)) == [] and gm.states_equal(m.pool.matrix.state(), g.voice_modulation_state(v)) == []
    assert g.device_errors() == 0


# ---- 8: the sharded handle ----
def test_sharded_equals_single():
    """All 28 routes with timed commands, one voice per sub-mixer and shard: the sharded handle renders what the plain graph renders, bit for bit,
    and forwards the matrix's state."""
    def build(g):
        ids, ms = [], []
        for i in range(2):
            mx = g.add_mixer()
            g.add_effect(mx, _capi.FX_GAIN, {"gain": 0.9})
            matrix = dict(rates=(20.0, 13.0), waveforms=(mm.SMOOTH_RANDOM if i else mm.SINE, mm.RAMP_DOWN), rng_states=LFO_RNG, velocity=0.8, note=72, routes=ALL_ROUTES)
            m = Model(LOOPED, matrix=matrix, cmds=[(700 + 100 * i, "clear", (0, mm.POSITION)), (1500, "rate", (1, 5.0))])
            ids.append(_add(g, mx, m))
            ms.append(m)
        return g, ids, ms

    single, sid, _ = build(Graph(SR, 2, MF, 0))
    sharded, hid, ms = build(ShardedGraph([0, 0], SR, 2, MF))
    assert sharded.shard_of_mixer(1) != sharded.shard_of_mixer(2)
    pos = 0
    for k in range(2):
        a, b = np.zeros(2 * MF, np.float32), np.zeros(2 * MF, np.float32)
        single.write(a, pos), sharded.write(b, pos)
        assert np.array_equal(a, b) and np.abs(a).max() > 0.01, k
        for m, v, w in zip(ms, sid, hid):
            m.write(MF)
            assert gm.states_equal(m.pool.state(), sharded.voice_grain_state(w)) == [] and gm.states_equal(m.pool.state(), single.voice_grain_state(v)) == []
            assert gm.states_equal(m.pool.matrix.state(), sharded.voice_modulation_state(w)) == [] and gm.states_equal(m.pool.matrix.state(), single.voice_modulation_state(v)) == []
        pos += MF
    assert sharded.device_errors() == 0 and single.device_errors() == 0
