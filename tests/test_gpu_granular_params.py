"""Granular parameters and the loop range changed while a granular voice plays (pg_graph_set_voice_granular_parameter / _grain_loop_range:
CMD_VOICE_GRAIN_PARAM / _LOOP in phase 1 of pg_grain_kernel, per-grain windows in phase 3, the pool's own overlap mode) against the independent
numpy model tests/granular_params_model.py (Sampler::set_granular_parameter, GrainPool::set_loop_range and try_trigger_grain's mode-change step
of the reference's src/generator/sampler.rs and src/generator/sampler/granular.rs). Everything goes through the C ABI.

In the shape of tests/test_gpu_modulation.py, whose comparison this file uses (_check_write: grain state and matrix state bit for bit, output within
the derived sum-order bound and bit-equal where at most one grain sounds): 8000 Hz, the 2048-frame seeded buffer, the same generator states. After
EVERY write additionally the parameter read-back (pg_graph_voice_granular_params) equals the model's parameters bit for bit. The model's process
calls are cut where the device's are: at the ends of the writes, on the 4096-frame chunk grid, at the voice's events and at its start time.
Every case asserts on the model that what it is about happened, so none passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import granular_model as gm
import granular_params_model as gpm
import modulation_model as mm
import test_gpu_modulation as tgm
from phonic_amd import _capi
from phonic_amd.graph import Graph, ShardedGraph

pytestmark = pytest.mark.gpu

SR, MF, RNG, LFO_RNG = tgm.SR, tgm.MF, tgm.RNG, tgm.LFO_RNG
BASE = tgm.BASE                  # density 50, size 60 ms, variation / spray / pan spread 0.3, step 1, position 0.2, Random direction
LOOPED = tgm.LOOPED              # ... and the loop range (0.25, 0.75)
SIZES = [64, 1000, 37, 947]      # 2048 frames, cut unevenly; the kernel's tile is 32 frames, a piece 1024


class Model(tgm.Model):
    """tgm.Model with the parameter model as its pool. cmds: tgm's (route / clear / rate / waveform / volume) and
    param (id4, value, normalized) / loop (range or None) / stop () - a stop is a message, not an event: it cuts nothing on the device, the model's
    extra cut changes no value."""

    def __init__(self, kw, matrix=None, start=0, cmds=(), volume=1.0):
        super().__init__(kw, matrix, start, cmds, volume)
        self.pool = gpm.ParamGrainPool(SR, self.buf, gm.Params(**kw), None if matrix is None else mm.make_matrix(SR, **matrix), RNG, 1.0, volume, 0.0)

    def _apply(self, t):
        for (ct, name, a) in self.cmds:
            if ct != t:
                continue
            if name == "param":
                if not self.pool.is_exhausted():      # a voice whose pool has run dry takes no parameters any more
                    self.pool.set_parameter(a[0], a[1], a[2], started=t >= self.start)
            elif name == "loop":
                if not self.pool.is_exhausted():
                    self.pool.set_loop_range(a[0])
            elif name == "route":
                self.pool.matrix.set_modulation(*a)
            elif name == "rate":
                self.pool.matrix.set_lfo_rate(*a)
            elif name == "volume":
                self.pool.set_volume(*a)
        if any(ct == t and name == "stop" for (ct, name, _) in self.cmds):   # GrainPool::stop() in front of the frame, behind the frame's commands
            self.pool.stop()


def _add(g, mixer, m):
    p = m.pool.p
    gp = _capi.granular_params(loop_range=p.loop_range, rng_state=RNG, overlap_mode=p.overlap_mode, window=p.window, size=p.size, density=p.density,
                               variation=p.variation, spray=p.spray, pan_spread=p.pan_spread, playback_direction=p.playback_direction, position=p.position, step=p.step)
    v = g.add_granular_voice(mixer, m.buf, gp, volume=m.volume, start_time=m.start)
    if m.mkw is not None:
        g.set_voice_modulation_matrix(v, **m.mkw)
    for (t, name, a) in m.cmds:
        if name == "param":
            g.set_voice_granular_parameter(v, a[0], a[1], t, normalized=a[2])
        elif name == "loop":
            g.set_voice_grain_loop_range(v, a[0], t)
        elif name == "route":
            g.set_voice_modulation(v, a[0], a[1], a[2], a[3], t)
        elif name == "rate":
            g.set_voice_lfo_rate(v, a[0], a[1], t)
        elif name == "volume":
            g.set_voice_volume(v, a[0], t)
        elif name == "stop":
            g.stop_voice(v, t)
    return v


def _check_write(g, v, m, got, exp, cnt, S, tag):
    tgm._check_write(g, v, m, got, exp, cnt, S, tag)
    bad = gm.states_equal(m.pool.params_state(), g.voice_granular_params(v))
    assert bad == [], (tag, "parameters", bad)


def _run(kw, sizes, graph=None, mixer=0, **mkw):
    """mixer "sub": the voice sits on a sub-mixer without effects, so its events stay inside the main mixer's chunk and reach pg_grain_kernel in the
    middle of a launch and of a tile; a main-mixer voice's events end the chunk and arrive at frame 0 of a launch."""
    m = Model(kw, **mkw)
    g = graph or Graph(SR, 2, MF, 0)
    if mixer == "sub":
        mixer = g.add_mixer()
    v = _add(g, mixer, m)
    assert g.voice_grain_state(v)["overlap_mode"] == gm.CLOUD      # GrainPool::new, until the first rendered frame
    pos, peak = 0, 0.0
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        exp, cnt, S = m.write(n)
        _check_write(g, v, m, buf, exp, cnt, S, (k, pos))
        peak = max(peak, float(np.abs(exp).max()))
        pos += n
    assert g.device_errors() == 0 and peak > 0.02
    return m, g, v


def _reference_state(kw, sizes, **mkw):
    """The same run without the commands (model only): what a case's final state must differ from."""
    m = Model(kw, **mkw)
    for n in sizes:
        m.write(n)
    return m.pool.state()


MIXERS = pytest.mark.parametrize("mixer", ["sub", 0], ids=["sub_mixer", "main_mixer"])

# ---- 1: each parameter once, raw and normalized, at frame 45 of the second write's second tile ----
ONE = {"GOVM": (1.0, 1.0), "GWND": (5.0, 0.5), "GSIZ": (20.0, 0.1), "GDEN": (90.0, 0.9), "GVAR": (0.9, 0.95), "GSPY": (0.9, 0.95), "GPAN": (0.9, 0.95), "GDIR": (1.0, 0.5),
       "GPOS": (0.7, 0.65), "GSTP": (-2.0, 0.9)}


@MIXERS
@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("id4", list(ONE))
def test_one_parameter(id4, normalized, mixer):
    kw = dict(BASE, step=0.0) if id4 == "GPOS" else BASE          # the position places grains only while step == 0
    cmds = [(64 + 45, "param", (id4, ONE[id4][int(normalized)], normalized))]
    m, g, v = _run(kw, SIZES, mixer=mixer, cmds=cmds)
    expected = gpm.resolve(id4, ONE[id4][int(normalized)], normalized)
    assert m.pool.params_state()[gpm.FIELD[id4]] == expected and expected != gm.Params(**kw).__dict__[gpm.FIELD[id4]]
    assert gm.states_equal(_reference_state(kw, SIZES), m.pool.state()) != []


# ---- 2: per-grain windows ----
def test_window_changed_twice_inside_one_launch():
    """Density 100 Hz, size 100 ms: ten grains overlap. Triangle -> Trapezoid -> Exponential inside the first piece of one write (a sub-mixer's
    voice): grains of three windows sound in the same frames - one row is staged in LDS, the others come from the global table."""
    kw = dict(BASE, density=100.0, size=100.0, variation=0.1)
    cmds = [(300, "param", ("GWND", 4, False)), (333, "param", ("GWND", 5, False))]
    probe = Model(kw, cmds=cmds)        # the model alone, frame by frame: the windows above the threshold in front of each frame
    most = 0
    for t in range(700):
        probe._apply(t)
        most = max(most, len(probe.pool.windows_above_threshold()))
        probe.pool.process(1)
    assert most == 3
    m, g, v = _run(kw, [2048], mixer="sub", cmds=cmds)
    assert set(m.pool.window_mode[m.pool.active]) == {5} and m.pool.params_state()["window"] == 5
    # the next write's launches stage the new row; grains of the old ones are gone
    m2, g2, v2 = _run(kw, [700, 1348], mixer="sub", cmds=cmds)
    assert gm.states_equal(m.pool.state(), m2.pool.state()) == []


# ---- 3 / 4: the pool's overlap mode ----
@MIXERS
def test_cloud_sequential_cloud(mixer):
    cmds = [(64 + 45, "param", ("GOVM", 1, False)), (900, "param", ("GOVM", 0.2, True)), (1300, "param", ("GOVM", 1.0, True)), (1700, "param", ("GOVM", 0, False))]
    m, g, v = _run(BASE, SIZES, mixer=mixer, cmds=cmds)
    assert m.pool.cleared_primaries >= 2 and m.pool.blocked_frames > 0 and m.pool.primary == -1 and m.pool.state()["overlap_mode"] == gm.CLOUD


@MIXERS
def test_window_change_moves_the_crossfade_point(mixer):
    """Sequential, 100 ms grains without variation: under Hann the next grain starts at phase 0.5 of the primary. Trapezoid's point is 0.9: after the
    change the primary blocks the trigger through 0.5 .. 0.9. Back to Hann while the primary stands in between: the next grain starts at once.
    A change Hann -> Trapezoid cannot itself land while the primary's phase is between 0.5 and 0.9: under Hann a primary never gets there, the
    grain triggered at 0.5 takes its place with phase 0. So the change lands early in a primary's life (frame 109, phase about 0.14), what is asserted
    is that frames are blocked with the primary PAST 0.5 - the stretch only the new window's point explains - and the change that does land inside
    0.5 .. 0.9 is the one back to Hann (frame 1300)."""
    kw = dict(BASE, overlap_mode=gm.SEQUENTIAL, window=0, size=100.0, variation=0.0)
    probe = Model(kw, cmds=[(64 + 45, "param", ("GWND", 4, False))])
    probe.write(1300)
    phase = probe.pool.window_phase[probe.pool.primary]
    assert 0.5 <= phase < 0.9 and probe.pool.blocked_past_half > 0              # frame 1300 lies in the blocked stretch
    cmds = [(64 + 45, "param", ("GWND", 4, False)), (1300, "param", ("GWND", 0.0, True))]
    m, g, v = _run(kw, SIZES, mixer=mixer, cmds=cmds)
    assert m.pool.blocked_past_half > 0 and (1300, ) == tuple(f for f, _ in m.pool.activations if f == 1300)
    assert gm.states_equal(_reference_state(kw, SIZES), m.pool.state()) != []


# ---- 5: step, position and the loop range ----
@MIXERS
def test_step_position_and_loop_range(mixer):
    """step 0 -> 2 -> 0 -> -1 with position changes on the way: the playhead starts from where it stood, the position counts only while step == 0.
    The loop range is replaced, removed and restored while grains that took the old one are alive and playing_loop_range stays set."""
    kw = dict(BASE, step=0.0, position=0.2, loop_range=(0.25, 0.75))
    cmds = [(64 + 45, "param", ("GPOS", 0.3, False)), (300, "param", ("GSTP", 2.0, False)), (700, "loop", ((0.4, 0.6),)), (900, "loop", (None,)),
            (1100, "loop", ((0.1, 0.9),)), (1300, "param", ("GSTP", 0.5, True)), (1400, "param", ("GPOS", 0.8, False)), (1700, "param", ("GSTP", -1.0, False)),
            (1800, "param", ("GPOS", 0.1, True))]
    probe = Model(kw, cmds=cmds)
    probe.write(299)
    assert not probe.pool.playing_loop_range and probe.pool.playhead == np.float32(0.2)      # step 0: the playhead rests
    probe.write(401 + 10)
    old = probe.pool.has_loop & probe.pool.active & (probe.pool.loop_end == float(np.float32(0.75)))
    assert probe.pool.playing_loop_range and old.any() and probe.pool.loop == (np.float32(0.4), np.float32(0.6))
    m, g, v = _run(kw, SIZES, mixer=mixer, cmds=cmds)
    assert m.pool.playing_loop_range and m.pool.params_state()["loop_end"] == np.float32(0.9) and m.pool.params_state()["step"] == np.float32(-1.0)
    ends = set(m.pool.loop_end[m.pool.active & m.pool.has_loop])
    assert float(np.float32(0.9)) in ends


# ---- 6: direction ----
@MIXERS
def test_direction_becomes_random(mixer):
    kw = dict(BASE, playback_direction=gm.FORWARD)
    m, g, v = _run(kw, SIZES, mixer=mixer, cmds=[(64 + 45, "param", ("GDIR", 2, False))])
    ref = Model(kw)
    for n in SIZES:
        ref.write(n)
    assert m.pool.rng_draws > ref.pool.rng_draws and (m.pool.increment[m.pool.active] < 0).any()


# ---- 7: a parameter and a route on the same target ----
@MIXERS
def test_parameter_with_a_route_on_it(mixer):
    matrix = dict(rates=(20.0, 13.0), rng_states=LFO_RNG, velocity=0.8, note=72, routes=[(0, mm.SIZE, 1.0, True), (1, mm.DENSITY, -1.0, True), (2, mm.POSITION, 0.37, False)])
    cmds = [(64 + 45, "param", ("GSIZ", 0.3, True)), (64 + 45, "param", ("GDEN", 100.0, False)), (700, "route", (0, mm.SIZE, -0.37, False)), (1500, "param", ("GDEN", 0.2, True))]
    m, g, v = _run(LOOPED, SIZES, mixer=mixer, matrix=matrix, cmds=cmds)
    assert m.pool.matrix.last[mm.SIZE] != 0 and m.pool.matrix.last[mm.DENSITY] != 0
    assert gm.states_equal(_reference_state(LOOPED, SIZES, matrix=matrix, cmds=[cmds[2]]), m.pool.state()) != []


# ---- 8: placement ----
def _placed(at):
    return [(at, "param", ("GDEN", 80.0, False)), (at, "param", ("GWND", 6, False)), (at, "loop", ((0.1, 0.5),)), (at, "param", ("GSIZ", 0.2, True)),
            (at + 200, "param", ("GOVM", 1, False)), (at + 200, "param", ("GPOS", 0.6, False)), (at + 431, "param", ("GOVM", 0, False)), (at + 431, "param", ("GDIR", 0.5, True)),
            (at + 431, "loop", (None,))]


@MIXERS
@pytest.mark.parametrize("where", list(tgm.PLACES))
def test_placement(where, mixer):
    """tgm.PLACES: the first and the last frame of a write, frames 0, 31, 32, 33 of a tile, next to a volume command (sizes 500 / 700 / 848)."""
    at = tgm.PLACES[where]
    cmds = _placed(at) + ([(777, "volume", (0.5,))] if where == "with_a_volume_command" else [])
    m, g, v = _run(LOOPED, [500, 700, 848], mixer=mixer, cmds=cmds)
    ps = m.pool.params_state()
    assert ps["has_loop_range"] == 0 and ps["window"] == 6 and ps["playback_direction"] == 1 and ps["density"] == np.float32(80.0) and m.pool.cleared_primaries >= 1


@MIXERS
def test_behind_the_chunk_edge(mixer):
    """A 5000-frame write is rendered as chunks of 4096 + 904 frames: commands at frame 4096 + 500, and two at the edge itself."""
    cmds = _placed(4596 - 431) + [(4096, "param", ("GVAR", 1.0, False)), (4096, "loop", ((0.5, 0.5),)), (4800, "param", ("GSTP", 0.0, False))]
    m, g, v = _run(LOOPED, [5000], mixer=mixer, cmds=cmds)
    assert m.pool.params_state()["variation"] == np.float32(1.0) and m.pool.params_state()["step"] == 0


@pytest.mark.parametrize("t0", [1024 + 32, 64, 1024 + 992], ids=["second_tile_of_a_piece", "third_tile_of_a_write", "last_tile_of_a_piece"])
def test_many_commands_in_one_tile(t0):
    """24 commands on the 32 frames of ONE tile of a launch (a sub-mixer's voice), several on the same frame: those apply in the order of the calls."""
    cmds = [(t0 + k, "param", (gpm.IDS[k % 10], [0.15, 0.8, 0.45][k % 3], True)) for k in range(0, 30, 2)]
    cmds += [(t0 + 12, "param", ("GDEN", 30.0, False)), (t0 + 12, "param", ("GDEN", 95.0, False)), (t0 + 12, "loop", ((0.2, 0.3),)), (t0 + 12, "loop", ((0.6, 0.9),)),
             (t0 + 13, "param", ("GOVM", 1, False)), (t0 + 13, "param", ("GOVM", 0, False)), (t0 + 13, "param", ("GOVM", 1, False)), (t0 + 31, "param", ("GWND", 7, False)),
             (t0 + 31, "param", ("GWND", 3, False))]
    m, g, v = _run(LOOPED, [2048], mixer="sub", cmds=cmds)
    ps = m.pool.params_state()
    assert len(cmds) >= 20 and ps["density"] == np.float32(95.0) and ps["loop_start"] == np.float32(0.6) and ps["window"] == 3 and ps["overlap_mode"] == 0 and m.pool.cleared_primaries >= 1


def test_more_commands_than_the_kernels_list_holds():
    """More than 64 commands of the voice in one piece: the scheduler lane walks the launch's own command list."""
    cmds = [(40 + 5 * k, "param", (gpm.IDS[(3 * k) % 10], [0.15, 0.8, 0.45][k % 3], True)) for k in range(90)]
    cmds += [(43 + 50 * k, "loop", ((0.1 * (k % 3), 0.5 + 0.1 * (k % 4)) if k % 4 else None,)) for k in range(8)] + [(222, "volume", (0.6,))]
    m, g, v = _run(LOOPED, [1024, 512], mixer="sub", cmds=cmds)
    assert len([c for c in cmds if c[0] < 1024]) > 64 + 30 and m.pool.cleared_primaries >= 1


# ---- 9: in front of the start time ----
def test_commands_in_front_of_a_start_time_inside_a_write():
    """The voice starts at frame 45 of the second write. Commands in front of it change the parameters, and the playhead takes the position that
    holds at the first rendered frame (GrainPool::start reads it at note-on); a position behind the start moves no playhead."""
    start = 64 + 45
    cmds = [(20, "param", ("GPOS", 0.9, False)), (20, "param", ("GDEN", 100.0, False)), (64 + 10, "param", ("GPOS", 0.6, False)), (64 + 10, "loop", ((0.5, 0.8),)),
            (start, "param", ("GWND", 0, False)), (start + 100, "param", ("GPOS", 0.1, False))]
    m = Model(BASE, start=start, cmds=cmds)
    g = Graph(SR, 2, MF, 0)
    v = _add(g, 0, m)
    pos = 0
    for k, n in enumerate([64, 500, 1484]):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        _check_write(g, v, m, buf, *m.write(n), (k, pos))
        if k == 0:
            st = g.voice_grain_state(v)
            assert st["playhead"] == np.float32(0.9) and st["overlap_mode"] == gm.CLOUD and not st["active"].any() and g.voice_granular_params(v)["density"] == np.float32(100.0)
        if k == 1:
            assert not buf.reshape(-1, 2)[:45].any() and m.pool.frame == 500 - 45
        pos += n
    assert m.pool.playing_loop_range and m.pool.params_state()["position"] == np.float32(0.1) and g.device_errors() == 0


# ---- 10: the voice ends, or is removed ----
def test_commands_around_the_voices_end():
    """GrainPool::stop() at frame 700 (step 0: an exhausted pool changes no more): a command on the stop's frame and one while the last grains
    sound are taken, those behind the frame at which the pool ran dry are not - in the same write or later."""
    kw = dict(BASE, step=0.0, size=30.0, variation=0.0)      # grains of 240 frames: the pool runs dry at about frame 940
    cmds = [(700, "param", ("GDEN", 99.0, False)), (700, "stop", ()), (800, "param", ("GSIZ", 500.0, False)), (800, "loop", ((0.3, 0.4),)), (1000, "param", ("GSIZ", 7.0, False)),
            (1000, "loop", (None,)), (1500, "param", ("GWND", 1, False)), (2100, "param", ("GDEN", 5.0, False))]
    m, g, v = _run(kw, [600, 424, 1024, 512], cmds=cmds)
    ps = m.pool.params_state()
    assert m.ended and ps["density"] == np.float32(99.0) and ps["size"] == np.float32(500.0) and ps["loop_end"] == np.float32(0.4) and ps["window"] == 2


def test_remove_voice_with_commands_pending():
    """The removed voice's pending commands become the mixer's no-op split: the other voice of the mixer renders what its model renders, its own
    commands arrive, and the removed voice's record stays what it was."""
    g = Graph(SR, 2, MF, 0)
    mx = g.add_mixer()
    gone = Model(BASE, cmds=[(300, "param", ("GDEN", 90.0, False)), (1500, "param", ("GWND", 5, False)), (1600, "loop", ((0.1, 0.2),))])
    stays = Model(LOOPED, cmds=[(1550, "param", ("GSIZ", 0.1, True)), (1700, "loop", (None,))])
    va, vb = _add(g, mx, gone), _add(g, mx, stays)
    one = Graph(SR, 2, MF, 0)
    vo = _add(one, one.add_mixer(), Model(LOOPED, cmds=stays.cmds))
    pos = 0
    for k, n in enumerate([1000, 1048]):
        if k == 1:
            before = g.voice_granular_params(va)
            g.remove_voice(va)
            assert g._lib.pg_graph_set_voice_granular_parameter(g._h, va, _capi.fourcc("GDEN"), 50.0, 0, 0) == _capi.PG_ERR_NOT_FOUND
        buf, alone = np.zeros(2 * n, dtype=np.float32), np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos), one.write(alone, pos)
        ea, eb = gone.write(n), stays.write(n)
        if k == 0:
            assert gm.states_equal(gone.pool.params_state(), g.voice_granular_params(va)) == [] and gone.pool.params_state()["density"] == np.float32(90.0)
        else:   # only `stays` sounds: what the same voice renders alone on its mixer, bit for bit
            assert np.array_equal(buf.view(np.uint32), alone.view(np.uint32)) and np.abs(buf).max() > 0.02
            assert gm.states_equal(before, g.voice_granular_params(va)) == [] and not g.is_voice_playing(va)
        assert gm.states_equal(stays.pool.state(), g.voice_grain_state(vb)) == [] and gm.states_equal(stays.pool.params_state(), g.voice_granular_params(vb)) == []
        pos += n
    assert stays.pool.params_state()["has_loop_range"] == 0 and g.device_errors() == 0 and one.device_errors() == 0


# ---- 11: error paths ----
def test_errors():
    lib = _capi.load()
    g = Graph(SR, 2, MF, 0)
    m = Model(BASE)
    v = _add(g, 0, m)
    f = g.add_voice(0, np.zeros(256, np.float32), 2, SR)
    other = Graph(SR, 2, MF, 0)          # (never written: a stream voice is fed by its host)
    s = other.add_stream_voice(0, 2, SR, 4096)
    fcc = _capi.fourcc
    p = _capi.GranularParams()
    for h, voice in ((g._h, 99), (g._h, -1), (g._h, f), (other._h, s)):       # unknown, a file voice, a stream voice
        assert lib.pg_graph_set_voice_granular_parameter(h, voice, fcc("GSIZ"), 50.0, 0, 0) == _capi.PG_ERR_NOT_FOUND, voice
        assert lib.pg_graph_set_voice_granular_parameter(h, voice, fcc("GWND"), 99.0, 0, 0) == _capi.PG_ERR_NOT_FOUND, voice
        assert lib.pg_graph_set_voice_grain_loop_range(h, voice, 1, 0.2, 0.6, 0) == _capi.PG_ERR_NOT_FOUND, voice
        assert lib.pg_graph_voice_granular_params(h, voice, C.byref(p)) == _capi.PG_ERR_NOT_FOUND, voice
    assert lib.pg_graph_set_voice_granular_parameter(g._h, v, fcc("GXYZ"), 0.5, 0, 0) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_set_voice_granular_parameter(g._h, v, fcc("GSIZ"), float("nan"), 0, 0) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_set_voice_grain_loop_range(g._h, v, 1, 0.2, 1.6, 0) == _capi.PG_ERR_PARAMETER
    assert lib.pg_graph_set_voice_granular_parameter(g._h, v, fcc("GWND"), 8.0, 0, 0) == _capi.PG_OK          # a raw index that names no variant: ignored
    assert lib.pg_graph_set_voice_granular_parameter(g._h, v, fcc("GSIZ"), 1.0e9, 0, 0) == _capi.PG_OK        # clamped to 1000 ms
    m.cmds = [(0, "param", ("GSIZ", 1.0e9, False))]
    out = np.zeros(2 * MF, np.float32)
    g.write(out, 0)
    _check_write(g, v, m, out, *m.write(MF), "after the errors")
    assert g.voice_granular_params(v)["size"] == np.float32(1000.0) and g.voice_granular_params(v)["window"] == 2 and g.device_errors() == 0


# ---- 12: the sharded handle ----
def test_sharded_equals_single():
    def build(g):
        ids, ms = [], []
        for i in range(2):
            mx = g.add_mixer()
            g.add_effect(mx, _capi.FX_GAIN, {"gain": 0.9})
            cmds = [(300 + 100 * i, "param", ("GWND", 4 + i, False)), (700, "param", ("GOVM", 1.0, True)), (900, "loop", ((0.3, 0.5),) if i else (None,)), (1500, "param", ("GSTP", -2.0, False))]
            m = Model(LOOPED, cmds=cmds)
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
            assert gm.states_equal(m.pool.params_state(), sharded.voice_granular_params(w)) == [] and gm.states_equal(m.pool.params_state(), single.voice_granular_params(v)) == []
        pos += MF
    assert ms[0].pool.cleared_primaries == 0 and ms[1].pool.params_state()["loop_end"] == np.float32(0.5)
    assert sharded.device_errors() == 0 and single.device_errors() == 0
