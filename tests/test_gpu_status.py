"""Playback status events on the GPU (pg_graph_enable_status / _set_voice_status / _poll_status / _status_dropped) against the independent
model of the reference's rules (tests/status_model.py): every graph is built twice — on the device through the C ABI and as the model's
mixer tree, whose sources restate playback_pos after every Source::write (the resampler's f32 consumption recurrence, loops, the fader's
arrival; the envelope and the grain pool come from tests/ahdsr_model.py, tests/granular_model.py and tests/modulation_model.py) — and driven
by the same calls. Every record is compared for equality: integers and exactly specified f64 / f32 operations, no tolerance.
48 kHz, max_frames 1024."""
import ctypes as C

import numpy as np
import pytest

import ahdsr_model as am
import granular_model as gm
import modulation_model as mm
import status_model as sm
from phonic_amd import _capi, workloads
from phonic_amd.graph import Graph, ShardedGraph

pytestmark = pytest.mark.gpu

SR = 48000
MF = 1024
RNG = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444)


class Rig:
    """One graph on the device and its model, built and driven together."""

    def __init__(self, graph=None, capacity=1 << 16, max_blocks=None):
        self.g = graph if graph is not None else Graph(SR, 2, MF, 0)
        if max_blocks:
            self.g.set_max_blocks_per_launch(max_blocks)
        self.g.enable_status(capacity)
        self.model = sm.Mixer()
        self.mixers = {0: self.model}
        self.sources = {}      # voice id -> (Playing, source, mixer id)
        self.ev = []           # the model's records, in the order of pg_graph_poll_status
        self.raw = []          # ... as the reference's traversal sends them during one write
        self.pending = []
        self.n = 0

    def add_mixer(self, parent=0):
        m = self.g.add_mixer(parent or None)
        self.mixers[m] = self.mixers[parent].add_mixer()
        return m

    def add_file(self, mixer=0, frames=6000, channels=2, rate=SR, emit=0.05, stopped=True, status=True, **opts):
        pcm = workloads.tone_buffer(self.n, rate, frames / rate, channels)
        self.n += 1
        v = self.g.add_voice(mixer, pcm, channels, rate, **opts)
        if status:
            self.g.set_voice_status(v, emit, stopped)
        s = sm.Sender(v, SR, emit if status else None, stopped and status, channels, rate, self.raw)
        loop = (opts["loop_start"], opts["loop_end"]) if opts.get("has_loop_range") else None
        f = sm.FileSource(s, pcm.size // channels, channels, rate, SR, speed=opts.get("speed", 1.0), repeat=opts.get("repeat", 0), loop_range=loop,
                          fade_out_seconds=opts.get("fade_out_seconds", 0.05))
        src = sm.Mapped(f) if channels == 1 else f
        self.sources[v] = (self.mixers[mixer].add_source(src, opts.get("start_time", 0)), f, mixer)
        return v

    def add_sampler_voice(self, mixer, v, source, start_time=0):
        self.sources[v] = (self.mixers[mixer].add_source(source, start_time), source, mixer)

    # control calls: the device's, and the same thing on the model (messages at the next write's top, events at their time)
    def stop(self, v, t):
        self.g.stop_voice(v, t)
        self.pending.append(lambda: setattr(self.sources[v][0], "stop_time", t))

    def event(self, v, t, fn=lambda: None):
        self.mixers[self.sources[v][2]].add_event(t, fn)

    def volume(self, v, value, t):
        self.g.set_voice_volume(v, value, t)
        self.event(v, t)

    def seek(self, v, seconds, t):
        self.g.seek_voice(v, seconds, t)
        self.event(v, t, lambda: self.sources[v][1].seek(seconds))

    def speed(self, v, speed, t):
        self.g.set_voice_speed(v, speed, t)
        self.event(v, t, lambda: self.sources[v][1].set_speed(speed))

    def remove(self, v):
        self.g.remove_voice(v)
        ps, _, m = self.sources[v]
        self.pending.append(lambda: self.mixers[m].remove_source(ps) if ps in self.mixers[m].sources else None)

    def _ranks(self):
        rank, out = [0], {}

        def walk(m):
            for c in m.mixers:
                walk(c)
            for ps in m.sources:
                for v, (p, _, _) in self.sources.items():
                    if p is ps:
                        out[v] = rank[0]
                rank[0] += 1

        walk(self.model)
        return out

    def write(self, frames, pos):
        for fn in self.pending:
            fn()
        self.pending = []
        out = np.zeros(2 * frames, np.float32)
        self.g.write(out, pos)
        ranks = self._ranks()
        del self.raw[:]
        self.model.write(frames, pos)
        self.ev += sorted(self.raw, key=lambda e: (e[2], ranks[e[1]]))   # by sample_time, then the traversal; stable: emission order inside a write
        return out

    def run(self, sizes, pos=0):
        outs = []
        for n in sizes:
            outs.append(self.write(n, pos))
            pos += n
        return np.concatenate(outs)

    def check(self):
        got = self.g.poll_status(1 << 16)
        for i, (a, b) in enumerate(zip(got, self.ev)):
            assert a == b, (i, a, b, got[max(0, i - 3):i + 3], self.ev[max(0, i - 3):i + 3])
        assert len(got) == len(self.ev), (len(got), len(self.ev), got[-4:], self.ev[-4:])
        assert self.g.status_dropped() == 0
        assert self.g.device_errors() == 0
        return got


# ---- the emit grid against the call grid ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[128] * 64, [1024] * 8, [8192]], ids=["128", "1024", "8192"])
def test_emit_grid_follows_the_call_grid(sizes):
    r = Rig()
    v = r.add_file(0, 6000)
    r.run(sizes)
    got = r.check()
    first = {128: 2432, 1024: 3072, 8192: 4096}[sizes[0]]   # the first write whose start is 2400 frames or more behind the clock's start
    assert got[0][:3] == ("position", v, first)
    assert got[-1] == ("stopped", v, {128: 5888, 1024: 5120, 8192: 4096}[sizes[0]], True)   # the write that hit the end of the file


def test_the_grids_differ_as_the_model_says():
    lists = []
    for sizes in ([128] * 64, [1024] * 8, [8192]):
        r = Rig()
        r.add_file(0, 6000)
        r.run(sizes)
        lists.append(r.check())
    assert lists[0] != lists[1] and lists[1] != lists[2] and [len(l) for l in lists] == [3, 2, 2]


@pytest.mark.parametrize("speed", [0.5, 2.0])
def test_speed(speed):
    r = Rig()
    r.add_file(0, 9000, speed=speed, emit=0.03)
    r.add_file(r.add_mixer(), 9000, channels=1, rate=44100, speed=speed, emit=0.02)
    r.run([1024] * 6 + [333, 691] + [1024] * 14)
    assert len(r.check()) > 6


def test_loop_with_repeat_and_seek_and_speed_change():
    r = Rig()
    m = r.add_mixer()
    a = r.add_file(m, 3000, repeat=2, has_repeat=1, has_loop_range=1, loop_start=500, loop_end=2500, emit=0.02)
    b = r.add_file(0, 20000, emit=0.02)
    c = r.add_file(m, 20000, emit=0.02)
    r.seek(b, 0.25, 2500)
    r.seek(c, 0.1, 3000)
    r.speed(c, 1.5, 5000)
    r.run([1024] * 12)
    got = r.check()
    assert ("stopped", a, 6144, True) in got and any(e[0] == "position" and e[1] == b and e[3] > 12000 for e in got)


def test_a_volume_change_inside_a_block_is_one_more_source_write():
    r = Rig()
    m = r.add_mixer()
    v = r.add_file(m, 20000, emit=0.03125)    # 1500 frames
    w = r.add_file(0, 20000, emit=0.03125)
    r.volume(v, 0.5, 1500)
    r.volume(w, 0.5, 1500)
    r.run([4096, 1024])
    got = r.check()
    # the write [0, 1500) sends nothing (elapsed 0), the one that begins at 1500 does: without the event the chunk [0, 4096) would send nothing
    assert got[0][:3] == ("position", v, 1500) and got[1][:3] == ("position", w, 1500)


def test_stops():
    r = Rig()
    m = r.add_mixer()
    fade = r.add_file(m, 40000, emit=None)
    cut = r.add_file(m, 40000, emit=0.01, fade_out_seconds=-1.0)
    main_cut = r.add_file(0, 40000, emit=0.01, fade_out_seconds=-1.0)
    early = r.add_file(0, 40000, emit=0.01, fade_out_seconds=-1.0, start_time=3000)
    wet = r.add_mixer()
    r.g.add_effect(wet, 5)                                    # a Reverb: the staged kernel renders this unit
    late_fade = r.add_file(wet, 40000, emit=0.01, rate=44100)  # default fade-out, resampled
    main_fade = r.add_file(0, 40000, emit=0.01)
    r.write(1024, 0)
    r.stop(fade, 1500)
    r.stop(cut, 2600)       # inside the piece [2048, 3072) of a later write: the time-parallel kernels render the write that ends there
    r.stop(late_fade, 3700) # ... and with a fade-out: the position behind the write that ends at 3700 is what PgVoice::stop_pos_lo / _hi keep
    r.stop(main_fade, 4600)
    r.stop(main_cut, 2048)  # at a write's first frame
    r.stop(early, 100)      # in front of the voice's start: taken by its first write
    r.run([1024] * 8, 1024)
    got = r.check()
    assert ("stopped", cut, 2600, False) in got and ("stopped", main_cut, 2048, False) in got and ("stopped", early, 3000, False) in got
    assert [e for e in got if e[1] == fade] == [("stopped", fade, 6144, False)]   # the write in which the fader arrived
    for v, t in ((late_fade, 3700), (main_fade, 4600)):      # a write ends at the stop time, the next begins there: both take the emit test
        assert [e[2] for e in got if e[1] == v and e[0] == "position" and t - t % 1024 <= e[2] <= t] == [t - t % 1024, t]


def test_enveloped_voice_stops_when_the_envelope_reaches_idle():
    r = Rig()
    m = r.add_mixer()
    kw = dict(attack_s=0.01, hold_s=0.0, decay_s=0.01, sustain_level=0.5, release_s=0.02)
    pcm = workloads.tone_buffer(0, SR, 40000 / SR)
    v = r.g.add_voice(m, pcm, 2, SR)
    r.g.set_voice_envelope(v, **kw)
    r.g.set_voice_status(v, 0.02, True)
    p, env = am.Params(SR, **kw), am.Envelope()
    env.note_on(p)
    s = sm.Sender(v, SR, 0.02, True, 2, SR, r.raw)

    def run(n):   # voice.rs:469-486
        if env.stage not in (am.SUSTAIN, am.IDLE):
            for _ in range(n):
                env.run(p)
        return env.stage == am.IDLE

    voice = sm.SamplerVoice(s, source=sm.FileSource(s, pcm.size // 2, 2, SR, SR), envelope_run=run)
    r.add_sampler_voice(m, v, voice)
    r.g.release_voice(v, 2500)
    r.event(v, 2500, lambda: env.note_off(p))
    r.run([1024] * 6)
    got = r.check()
    assert got[-1] == ("stopped", v, 3072, False)   # released at 2500, 960 frames of release: Idle inside the write that begins at 3072


# ---- granular voices -------------------------------------------------------------------------------------------------------------------
def _granular(r, mixer, kw, matrix=None, emit=0.03, buffer=None, stop_at=None):
    buf = gm.make_buffer(2048)
    p = gm.Params(**kw)
    if matrix is None:
        pool = gm.GrainPool(SR, buf, p, RNG, 1.0, 1.0, 0.0)
    else:
        pool = mm.ModGrainPool(SR, buf, p, mm.make_matrix(SR, **matrix), RNG, 1.0, 1.0, 0.0)
    gp = _capi.granular_params(loop_range=p.loop_range, rng_state=RNG, overlap_mode=p.overlap_mode, window=p.window, size=p.size, density=p.density, variation=p.variation,
                               spray=p.spray, pan_spread=p.pan_spread, playback_direction=p.playback_direction, position=p.position, step=p.step)
    v = r.g.add_granular_voice(mixer, buf, gp)
    if matrix is not None:
        r.g.set_voice_modulation_matrix(v, **matrix)
    r.g.set_voice_status(v, emit, True)
    s = sm.Sender(v, SR, emit, True, 1, SR, r.raw)
    voice = sm.SamplerVoice(s, pool=pool, buffer_len=buf.size)
    r.add_sampler_voice(mixer, v, voice)
    return v


GRANULAR = {
    "step0": (dict(position=0.3, size=20.0, density=40.0), None),
    "step": (dict(position=0.2, step=1.5, size=20.0, density=40.0), None),
    "loop": (dict(position=0.1, step=2.0, size=20.0, density=40.0, loop_range=(0.25, 0.5)), None),
    "lfo_position": (dict(position=0.4, step=0.5, size=20.0, density=40.0), dict(rates=(7.0, 2.0), routes=[(0, 5, 0.3, True)])),
}


@pytest.mark.parametrize("case", sorted(GRANULAR))
def test_granular_voice(case):
    kw, matrix = GRANULAR[case]
    r = Rig()
    m = r.add_mixer()
    v = _granular(r, m, kw, matrix)
    r.write(1024, 0)
    r.stop(v, 2000)
    r.volume(v, 0.7, 1500)   # an event of the voice's mixer: one more process call
    r.run([1024] * 5, 1024)
    got = r.check()
    assert got[0][:3] == ("position", v, 0)                                   # the start event, at the first write
    assert got[-2:] == [("stopped", v, got[-1][2], False)] * 2                # the two Stopped records
    assert len({e[3] for e in got if e[0] == "position"}) > (1 if case != "step0" else 0)


# ---- order, capacity, audio -------------------------------------------------------------------------------------------------------------
def test_order_over_sub_mixers_and_nested_sub_mixers():
    r = Rig()
    a = r.add_mixer()
    b = r.add_mixer(a)
    c = r.add_mixer()
    for mixer in (0, c, b, a, 0, b):
        r.add_file(mixer, 5000, emit=1e-9)
    r.volume(list(r.sources)[2], 0.5, 700)    # an event of the nested mixer ...
    r.volume(list(r.sources)[3], 0.5, 2100)   # ... and one of its parent: a call boundary for the nested one
    r.run([1024] * 6)
    got = r.check()
    assert [e[1] for e in got if e[2] == 0] == [5, 2, 3, 1, 4, 0]   # nested b (5 in front of 2: the same start time), a, c, then the main mixer's own


def test_64_voices_with_mixed_emit_rates_over_two_mixers():
    r = Rig()
    mixers = [r.add_mixer(), r.add_mixer()]
    for i in range(64):
        r.add_file(mixers[i % 2], 3000 + 37 * i, emit=[0.01, 0.02, 0.035, None][i % 4], stopped=i % 8 != 7, start_time=(i % 5) * 300)
    r.run([1024] * 7)
    assert len(r.check()) > 200


def test_capacity_four_counts_what_it_drops_and_goes_on():
    r = Rig(capacity=4)
    v = r.add_file(0, 100000, emit=1e-9)
    for k in range(7):
        r.write(1024, 1024 * k)
    assert r.g.status_dropped() == 3
    assert r.g.poll_status(3) == r.ev[:3]            # a poll smaller than what waits ...
    assert r.g.poll_status(16) == r.ev[3:4]          # ... the next one goes on; records 4, 5 and 6 were dropped
    r.write(1024, 7168)
    r.write(1024, 8192)
    assert r.g.poll_status(16) == r.ev[7:9] and r.g.status_dropped() == 3
    assert r.ev[8] == ("position", v, 8192, 9216, 9216 / 48000)


def test_status_enabled_but_nobody_opted_in():
    r = Rig()
    r.add_file(0, 3000, status=False)
    r.add_file(r.add_mixer(), 3000, status=False)
    r.run([1024] * 4)
    assert r.g.poll_status(16) == [] and r.ev == []


def test_errors():
    g = Graph(SR, 2, MF, 0)
    lib, pcm = g._lib, workloads.tone_buffer(0, SR, 0.1)
    v = g.add_voice(0, pcm, 2, SR)
    assert lib.pg_graph_set_voice_status(g._h, v, 0.05, 1) == _capi.PG_ERR_STATE          # not enabled
    assert lib.pg_graph_enable_status(g._h, 0) == _capi.PG_ERR_PARAMETER
    g.enable_status(64)
    assert lib.pg_graph_enable_status(g._h, 64) == _capi.PG_ERR_STATE                      # once
    assert lib.pg_graph_set_voice_status(g._h, 99, 0.05, 1) == _capi.PG_ERR_NOT_FOUND
    assert lib.pg_graph_set_voice_status(g._h, v, float("nan"), 1) == _capi.PG_ERR_PARAMETER
    conv = g.add_voice(0, pcm, 2, SR, source_rate=44100)
    assert lib.pg_graph_set_voice_status(g._h, conv, 0.05, 1) == _capi.PG_ERR_PARAMETER    # rate-converted
    fed = g.add_stream_voice(0, 2, SR, 4096)
    assert lib.pg_graph_set_voice_status(g._h, fed, 0.05, 1) == _capi.PG_ERR_PARAMETER     # host-fed
    g.set_voice_status(v, 0.05, True)
    g.write(np.zeros(2048, np.float32), 0)
    assert lib.pg_graph_set_voice_status(g._h, v, 0.05, 1) == _capi.PG_ERR_STATE           # has rendered
    late = Graph(SR, 2, MF, 0)
    late.add_voice(0, pcm, 2, SR)
    late.write(np.zeros(2048, np.float32), 0)
    assert lib.pg_graph_enable_status(late._h, 64) == _capi.PG_ERR_STATE                    # before the first write


def _headline_like(status, blocks):
    g = Graph(SR, 2, MF, 0)
    g.set_max_blocks_per_launch(blocks)
    if status is not None:
        g.enable_status(1 << 16)
    workloads.build_headline(g, n_voices=12)
    voices = []
    extra = g.add_mixer()
    for i in range(3):
        voices.append(g.add_voice(extra, workloads.tone_buffer(40 + i, SR, 0.4), 2, SR))
    voices.append(g.add_voice(0, workloads.tone_buffer(50, SR, 0.4), 2, SR))
    if status:
        for v in voices:
            g.set_voice_status(v, 0.01, True)
        for v in range(12):
            g.set_voice_status(v, 0.02, True)
    g.set_voice_volume(voices[0], 0.5, 1500)
    g.set_voice_volume(voices[3], 0.25, 5000)
    g.stop_voice(voices[1], 9216)        # at a piece's first frame
    g.stop_voice(2, 6700)                # strictly inside a piece, on units with a Reverb (the staged kernel): a fade-out ...
    g.stop_voice(voices[2], 7001)        # ... on a unit without effects, and on a main-mixer source
    g.stop_voice(voices[3], 11111)
    out = [np.zeros(2 * n, np.float32) for n in (1024, 4096, 8192, 1024)]
    pos = 0
    for o in out:
        g.write(o, pos)
        pos += o.size // 2
    assert g.device_errors() == 0
    return np.concatenate(out), (g.poll_status(1 << 16) if status is not None else None)


def test_audio_is_bit_identical_with_and_without_status():
    plain, _ = _headline_like(None, 8)
    enabled, none = _headline_like(False, 8)
    reporting, records = _headline_like(True, 8)
    assert none == [] and len(records) > 50
    assert np.abs(plain).max() > 1e-3
    assert np.array_equal(plain.view(np.uint32), enabled.view(np.uint32))
    assert np.array_equal(plain.view(np.uint32), reporting.view(np.uint32))


def test_voices_made_from_a_sample_buffer():
    """Position divides by the FILE buffer's channel count and rate, and a granular voice's sample position scales by the file buffer's
    len() — frames x channels, the decoder's extra zero frame included (voice.rs:455-466) — not by the mono buffer's."""
    r = Rig()
    m = r.add_mixer()
    pcm = workloads.tone_buffer(3, 44100, 3000 / 44100, 2)
    b = r.g.add_sample_buffer(pcm, 2, 44100)
    v = r.g.add_voice_from_buffer(m, b)
    r.g.set_voice_status(v, 0.01, True)
    s = sm.Sender(v, SR, 0.01, True, 2, 44100, r.raw)
    r.add_sampler_voice(m, v, sm.FileSource(s, pcm.size // 2, 2, 44100, SR))
    mono = r.g.read_granular_buffer(b)
    p = gm.Params(position=0.2, step=1.5, size=20.0, density=40.0)
    gp = _capi.granular_params(rng_state=RNG, overlap_mode=p.overlap_mode, window=p.window, size=p.size, density=p.density, variation=p.variation, spray=p.spray,
                               pan_spread=p.pan_spread, playback_direction=p.playback_direction, position=p.position, step=p.step)
    gv = r.g.add_granular_voice_from_buffer(m, b, gp)
    r.g.set_voice_status(gv, 0.01, True)
    gs = sm.Sender(gv, SR, 0.01, True, 2, 44100, r.raw)
    r.add_sampler_voice(m, gv, sm.SamplerVoice(gs, pool=gm.GrainPool(SR, mono, p, RNG, 1.0, 1.0, 0.0), buffer_len=pcm.size))
    r.run([1024] * 5)
    got = r.check()
    pos = [e for e in got if e[1] == gv and e[0] == "position"]
    assert len(pos) >= 4 and pos[0][2] == 0 and len({e[3] for e in pos}) > 2
    assert pos[0][4] == pos[0][3] / 44100 and ("stopped", v, 3072, True) in got


def test_sharded_handle_merges_the_shards():
    sh = ShardedGraph([0, 0], SR, 2, MF)
    r = Rig(graph=sh)
    mixers = [r.add_mixer() for _ in range(3)]
    nested = r.add_mixer(mixers[1])
    for mixer in (mixers[2], 0, nested, mixers[0], 0, mixers[1], 0):
        r.add_file(mixer, 5000, emit=0.01)
    assert len({sh.shard_of_mixer(m) for m in mixers}) == 2
    r.volume(list(r.sources)[0], 0.5, 1300)
    r.run([1024, 4096, 1024])
    got = r.check()
    assert len(got) >= 14 and {sh.shard_of_mixer(m) for m in mixers} == {0, 1}
