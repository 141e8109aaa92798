"""Per-voice AHDSR volume envelopes on the GPU (pg_graph_set_voice_envelope / pg_graph_release_voice) against the CPU oracle's render of the
same graph without an envelope, multiplied frame by frame by the independent f32 model of the reference's envelope (tests/ahdsr_model.py,
src/utils/ahdsr.rs). Everything goes through the C ABI (phonic_amd.graph is a ctypes mirror of include/phonic_gpu.h).

Scaled decay curves: after a timed attack the reference leaves target_volume AT the sustain level (ahdsr.rs:456-468), so its scaled decay has
a range of f32::EPSILON and a "progress" far outside [0, 1] (:526-542; a debug build of the reference panics there, a release build hands out
inf or NaN). A decay scaling therefore only meets a zero attack time here — the one configuration in which the reference's curve is defined;
attack and release scalings meet timed attacks."""
import numpy as np
import pytest

import ahdsr_model as M
import oracle
from phonic_amd import _capi, workloads
from phonic_amd.graph import Graph, ShardedGraph

pytestmark = pytest.mark.gpu

SR = 48000
MF = 1024


def _tone(i, frames):
    return workloads.tone_buffer(i, SR, frames / SR)


def _writes(g, sizes, on_write=None):
    out, pos = [], 0
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        pos += n
        out.append(buf)
        if on_write:
            on_write(k, pos)
    return np.concatenate(out)


def _dry(pcm, n_frames):
    o = oracle.OracleGraph(SR, 2, MF)
    o.add_voice(0, pcm, 2, SR)
    return o.render(n_frames // MF, MF)


def _gpu_single(pcm, sizes, env_kw, note_off=None, on_write=None, graph_out=None):
    g = Graph(SR, 2, MF, 0)
    v = g.add_voice(0, pcm, 2, SR)
    g.set_voice_envelope(v, **env_kw)
    if note_off is not None:
        g.release_voice(v, note_off)
    if graph_out is not None:
        graph_out.append((g, v))
    out = _writes(g, sizes, (lambda k, pos: on_write(g, v, k, pos)) if on_write else None)
    assert g.device_errors() == 0
    return out


def _expected(dry, env_kw, n_frames, note_off=None):
    gains, _, _ = M.render(M.Params(SR, **env_kw), n_frames, note_off_at=note_off)
    return (dry.reshape(-1, 2) * gains[:, None]).astype(np.float32).reshape(-1), gains


N_LONG = 144 * MF    # 3.07 s: the default envelope reaches Sustain at frame 72480
N = 76 * MF          # 1.62 s

BIT_EXACT = {
    "default": (dict(), N_LONG, None),
    "zero_attack": (dict(attack_s=0.0), N, None),
    "zero_hold": (dict(hold_s=0.0), N, None),
    "zero_decay": (dict(decay_s=0.0), N, None),
    "zero_attack_hold_decay": (dict(attack_s=0.0, hold_s=0.0, decay_s=0.0), N, 30001),
    "sustain_0": (dict(sustain_level=0.0), N, None),
    "sustain_1": (dict(sustain_level=1.0), N, 74003),
    "off_in_attack": (dict(), N, 301),
    "off_in_hold": (dict(), N, 20011),
    "off_in_decay": (dict(), N, 60013),
    "off_in_sustain": (dict(release_s=0.05), N, 74003),
    "off_zero_release": (dict(release_s=0.0), N, 50001),
    "off_at_block_start": (dict(release_s=0.3), N, 30 * MF),
    "off_at_block_end": (dict(release_s=0.3), N, 30 * MF + MF - 1),
    "off_before_first_frame": (dict(), 8 * MF, 0),
}


@pytest.mark.parametrize("name", list(BIT_EXACT))
def test_bit_exact_against_oracle_times_model(name):
    env_kw, n, off = BIT_EXACT[name]
    pcm = _tone(3, n + 64)
    exp, gains = _expected(_dry(pcm, n), env_kw, n, off)
    got = _gpu_single(pcm, [MF] * (n // MF), env_kw, off)
    assert np.abs(exp).max() > 1e-3 or name == "off_before_first_frame"
    assert np.array_equal(got, exp), (name, int(np.flatnonzero(got != exp)[0]) // 2, float(np.abs(got - exp).max()))


@pytest.mark.parametrize("name", ["default", "off_in_decay"])
def test_piece_independence_and_stage(name):
    """128-frame writes, 1024-frame writes and one write of the whole length: bit-identical audio, and after every write the envelope's stage
    is the model's."""
    env_kw, n, off = BIT_EXACT[name]
    pcm = _tone(5, n + 64)
    params = M.Params(SR, **env_kw)
    outs = []
    for sizes in ([128] * (n // 128), [MF] * (n // MF), [n]):
        _, stages, idle_call = M.render(params, n, note_off_at=off, pieces=sizes)
        stage_at = dict(stages)
        seen = []

        def check(g, v, k, pos, stage_at=stage_at, seen=seen):   # after EVERY write
            seen.append((pos, g.voice_envelope_stage(v), stage_at[pos]))

        outs.append(_gpu_single(pcm, sizes, env_kw, off, on_write=check))
        assert all(a == b for _, a, b in seen), [s for s in seen if s[1] != s[2]][:5]
        assert len(seen) == len(sizes)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    exp, _ = _expected(_dry(pcm, n), env_kw, n, off)
    assert np.array_equal(outs[1], exp)


SCALED = [
    # timed attack: attack and release scalings from {-1, -0.5, 0.5, 1}, note-off inside the attack or later
    (dict(attack_s=0.2, attack_scaling=-1.0, release_s=0.2, release_scaling=0.5), 40 * MF, 30011),
    (dict(attack_s=0.2, attack_scaling=-0.5, release_s=0.2, release_scaling=1.0), 40 * MF, 5003),
    (dict(attack_s=0.2, attack_scaling=0.5, release_s=0.2, release_scaling=-1.0), 40 * MF, 30011),
    (dict(attack_s=0.2, attack_scaling=1.0, release_s=0.2, release_scaling=-0.5), 40 * MF, 7001),
    # zero attack: the decay scaling works on [sustain, 1]
    (dict(attack_s=0.0, hold_s=0.05, decay_s=0.4, decay_scaling=-1.0, attack_scaling=0.5, release_s=0.2, release_scaling=0.5), 40 * MF, 30011),
    (dict(attack_s=0.0, hold_s=0.0, decay_s=0.4, decay_scaling=-0.5, attack_scaling=-1.0, release_s=0.2, release_scaling=1.0), 40 * MF, 9001),
    (dict(attack_s=0.0, hold_s=0.05, decay_s=0.4, decay_scaling=0.5, attack_scaling=1.0, sustain_level=0.2, release_s=0.2, release_scaling=-1.0), 40 * MF, 30011),
    (dict(attack_s=0.0, hold_s=0.0, decay_s=0.4, decay_scaling=1.0, attack_scaling=-0.5, sustain_level=0.0, release_s=0.2, release_scaling=-0.5), 40 * MF, None),
]


@pytest.mark.parametrize("case", range(len(SCALED)))
def test_scaled_curves(case):
    """The project's standing tolerance against the oracle (tests/test_gpu_fullsize.py): <= 1e-5 RMS, <= 1e-4 max. The device's powf and
    numpy's are both within a few ulp for values <= 1."""
    env_kw, n, off = SCALED[case]
    pcm = _tone(7, n + 64)
    exp, gains = _expected(_dry(pcm, n), env_kw, n, off)
    assert np.isfinite(gains).all() and gains.max() <= 1.0 and gains.min() >= 0.0
    got = _gpu_single(pcm, [MF] * (n // MF), env_kw, off)
    d = got.astype(np.float64) - exp.astype(np.float64)
    rms, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"scaled case {case}: rms {rms:.3e} max {mx:.3e} (signal peak {np.abs(exp).max():.3f})")
    assert rms <= 1e-5 and mx <= 1e-4


def test_end_of_the_voice():
    """A release that reaches Idle: the voice is not playing once that write has ended, everything behind the Idle frame is exactly 0, and the
    unit goes back to the time-parallel kernels: the write after the end carries the topology change, which every unit sits out on the exact
    kernel once, and from the write behind that one no unit is deferred."""
    n = 40 * MF
    g = Graph(SR, 2, MF, 0)
    m = g.add_mixer()
    g.add_effect(m, _capi.FX_GAIN)
    plain = g.add_voice(m, _tone(1, n + 64), 2, SR)
    v = g.add_voice(m, _tone(2, n + 64), 2, SR)
    env_kw = dict(attack_s=0.01, hold_s=0.05, decay_s=0.05, release_s=0.05)
    g.set_voice_envelope(v, **env_kw)
    off = 10 * MF + 77
    g.release_voice(v, off)
    gains, stages, idle_call = M.render(M.Params(SR, **env_kw), n, note_off_at=off, pieces=[MF] * 40)
    idle_frame = int(np.flatnonzero(gains[off:] == 0.0)[0]) + off
    end_write = idle_frame // MF   # the write in which the envelope became Idle
    deferred, playing, stage = [], [], []
    for k in range(40):
        buf = np.zeros(2 * MF, dtype=np.float32)
        g.write(buf, k * MF)
        deferred.append(g.deferred_units())
        playing.append(g.is_voice_playing(v))
        stage.append(g.voice_envelope_stage(v))
    assert all(playing[:end_write]) and not any(playing[end_write:]), (end_write, playing)
    assert stage[end_write - 1] == M.RELEASE and stage[end_write] == M.IDLE
    print(f"end of the voice: envelope Idle in write {end_write}, deferred units per write {deferred}")
    assert all(d == 1 for d in deferred[2:end_write + 1]), deferred     # the one unit with the living envelope
    # the next write reads the voice's `ended` word, clears static_defer and uploads the topology: that round sends every unit (here: the one)
    # through the exact kernel, as any topology change does; from the write behind it nothing is deferred
    assert deferred[end_write + 1] == 1, deferred
    assert all(d == 0 for d in deferred[end_write + 2:]), deferred      # static_defer is gone
    assert g.is_voice_playing(plain)
    # the enveloped voice alone: exactly 0 behind the Idle frame
    pcm = _tone(2, n + 64)
    solo = _gpu_single(pcm, [MF] * 40, env_kw, off)
    assert np.abs(solo[2 * idle_frame:]).max() == 0.0 and np.abs(solo[2 * (idle_frame - 200):2 * idle_frame]).max() > 0.0
    assert g.device_errors() == 0


def test_release_without_envelope_is_a_stop():
    """SamplerVoice::stop without envelope parameters stops the file source (voice.rs:207-208): the same audio as pg_graph_stop_voice."""
    n = 16 * MF
    outs = []
    for how in ("release", "stop"):
        g = Graph(SR, 2, MF, 0)
        v = g.add_voice(0, _tone(4, n + 64), 2, SR)
        (g.release_voice if how == "release" else g.stop_voice)(v, 5 * MF + 13)
        outs.append(_writes(g, [MF] * 16))
        assert g.voice_envelope_stage(v) == -1
    assert np.array_equal(outs[0], outs[1]) and np.abs(outs[0][2 * 5 * MF:2 * 5 * MF + 20]).max() > 0


def test_attach_after_the_first_frame_is_an_error():
    g = Graph(SR, 2, MF, 0)
    v = g.add_voice(0, _tone(4, 8 * MF), 2, SR)
    late = g.add_voice(0, _tone(5, 8 * MF), 2, SR, start_time=4 * MF)
    _writes(g, [MF])
    with pytest.raises(Exception) as e:
        g.set_voice_envelope(v)
    assert e.value.code == _capi.PG_ERR_STATE
    g.set_voice_envelope(late)   # has not rendered a frame yet
    assert g.voice_envelope_stage(late) == M.ATTACK and g.voice_envelope_stage(v) == -1


def test_live_note_on_after_the_graph_has_rendered():
    """The live case: a voice added with start_time 0 ("now") after several writes has rendered nothing, so it takes an envelope; it starts with
    the next write's first frame, and the audio from there is the oracle's dry render times the model, bit for bit, with the note-off at its
    frame. Attaching is refused only once a write issued after the voice was added has ended behind its start time — also when the host has
    moved the position backwards in between."""
    n, t0, off = 12 * MF, 3 * MF, 5 * MF + 37
    env_kw = dict(attack_s=0.02, hold_s=0.03, decay_s=0.04, release_s=0.05)
    bed, pcm = _tone(6, t0 + n + 64), _tone(3, n + 64)
    g = Graph(SR, 2, MF, 0)
    b = g.add_voice(0, bed, 2, SR)
    head = _writes(g, [MF] * 3)
    v = g.add_voice(0, pcm, 2, SR)               # start_time 0: plays from the next write on
    g.set_voice_envelope(v, **env_kw)
    assert g.voice_envelope_stage(v) == M.ATTACK
    g.release_voice(v, t0 + off)
    g.remove_voice(b)
    got = []
    for k in range(n // MF):
        buf = np.zeros(2 * MF, dtype=np.float32)
        g.write(buf, t0 + k * MF)
        got.append(buf)
    got = np.concatenate(got)
    exp, _ = _expected(_dry(pcm, n), env_kw, n, off)
    assert np.abs(head).max() > 1e-3 and np.abs(exp).max() > 1e-3
    assert np.array_equal(got, exp), (int(np.flatnonzero(got != exp)[0]) // 2, float(np.abs(got - exp).max()))
    assert g.voice_envelope_stage(v) == M.IDLE and g.device_errors() == 0
    # ... and refused once the voice has rendered: one write behind the add is enough, wherever the earlier writes stood
    h = Graph(SR, 2, MF, 0)
    h.add_voice(0, bed, 2, SR)
    buf = np.zeros(2 * MF, dtype=np.float32)
    for k in range(4):
        h.write(buf, k * MF)
    w = h.add_voice(0, pcm, 2, SR)
    h.write(buf, 0)                              # the host went back to frame 0: the new voice renders there
    with pytest.raises(Exception) as e:
        h.set_voice_envelope(w, **env_kw)
    assert e.value.code == _capi.PG_ERR_STATE
    x = h.add_voice(0, pcm, 2, SR)               # added behind the rewind, nothing rendered since: accepted
    h.set_voice_envelope(x, **env_kw)
    assert h.voice_envelope_stage(x) == M.ATTACK and h.voice_envelope_stage(w) == -1


def test_a_kept_source_leaves_the_exact_kernel_when_its_envelope_ends():
    """non_transient: the mixer keeps the exhausted source in its list (mixed.rs:612-620), but its envelope is Idle for good — the unit goes
    back to the time-parallel kernels like a transient voice's."""
    g = Graph(SR, 2, MF, 0)
    m = g.add_mixer()
    g.add_effect(m, _capi.FX_GAIN)
    g.add_voice(m, _tone(1, 24 * MF + 64), 2, SR)
    v = g.add_voice(m, _tone(2, 24 * MF + 64), 2, SR, non_transient=1)
    g.set_voice_envelope(v, attack_s=0.01, hold_s=0.02, decay_s=0.02, release_s=0.03)
    g.release_voice(v, 6 * MF + 5)
    deferred, stage = [], []
    _writes(g, [MF] * 24, lambda k, pos: (deferred.append(g.deferred_units()), stage.append(g.voice_envelope_stage(v))))
    end_write = stage.index(M.IDLE)
    print(f"kept source: envelope Idle in write {end_write}, deferred units per write {deferred}")
    assert 6 <= end_write <= 9 and all(d == 1 for d in deferred[2:end_write + 1]), (end_write, deferred)
    assert all(d == 0 for d in deferred[end_write + 2:]), deferred
    assert g.device_errors() == 0


def _many_graph(g, is_oracle, n, rng_seed=77):
    """64 voices over 8 mixers (Gain -> Reverb each), seeded envelope parameters and note-off times. The oracle gets file x model envelope, cut
    at the end of the write in which the envelope went Idle (voice.rs:488-495: the voice is reset in the process call in which the stage
    became Idle — the cut the device makes too), and a same-value volume event where the GPU graph has its note-off: both mixers split their
    chunk at that frame."""
    rng = np.random.default_rng(rng_seed)
    for mi in range(8):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_GAIN, {"gain": 0.8})
        g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(mi))
        for k in range(8):
            i = mi * 8 + k
            env_kw = dict(attack_s=float(rng.choice([0.0, 0.005, 0.03])), hold_s=float(rng.choice([0.0, 0.02, 0.1])), decay_s=float(rng.choice([0.0, 0.05, 0.15])),
                          sustain_level=float(rng.choice([0.0, 0.4, 0.75, 1.0])), release_s=float(rng.choice([0.0, 0.03, 0.12])))
            off = int(rng.integers(1, n - 1)) if rng.random() < 0.8 else None
            vol, pan = float(np.float32(0.3 + 0.1 * (i % 5))), float(np.float32(workloads.voice_pan(i)))
            pcm = _tone(i, n + 64)
            if not is_oracle:
                v = g.add_voice(m, pcm, 2, SR, volume=vol, panning=pan)
                g.set_voice_envelope(v, **env_kw)
                if off is not None:
                    g.release_voice(v, off)
            else:
                gains, _, idle_call = M.render(M.Params(SR, **env_kw), n, note_off_at=off, pieces=[MF] * (n // MF))
                f = pcm.reshape(-1, 2).copy()
                f[:n] *= gains[:, None]
                if idle_call is not None:
                    bounds = sorted(set(range(0, n + 1, MF)) | ({off} if off is not None else set()))
                    end = -(-bounds[idle_call + 1] // MF) * MF   # the end of the WRITE that holds that call
                    f = f[:end]
                v = g.add_voice(m, f.reshape(-1), 2, SR, volume=vol, panning=pan)
                if off is not None:
                    g.set_voice_volume(v, vol, off)


def test_many_voices_with_effects():
    n = 24 * MF
    g, o = Graph(SR, 2, MF, 0), oracle.OracleGraph(SR, 2, MF)
    _many_graph(g, False, n)
    _many_graph(o, True, n)
    got, exp = _writes(g, [MF] * 24), o.render(24, MF)
    d = got.astype(np.float64) - exp.astype(np.float64)
    rms, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"many voices: rms {rms:.3e} max {mx:.3e} (signal peak {np.abs(exp).max():.3f})")
    assert np.abs(exp).max() > 0.05
    assert rms <= 1e-5 and mx <= 1e-4
    assert g.device_errors() == 0


def test_untouched_graph_beside_an_enveloped_unit():
    """The headline graph at 64 voices with one extra unit that holds an enveloped voice = the graph without it + that unit's own render
    (within 1e-6 max in f64), and exactly one unit is deferred to the exact kernel while the envelope lives."""
    blocks = 12
    pcm = _tone(9, blocks * MF + 64)

    def extra(g):
        m = g.add_mixer()
        v = g.add_voice(m, pcm, 2, SR, volume=0.5)
        g.set_voice_envelope(v, attack_s=0.05, hold_s=0.02, decay_s=0.05)
        return v

    a, b, c = Graph(SR, 2, MF, 0), Graph(SR, 2, MF, 0), Graph(SR, 2, MF, 0)
    workloads.build_headline(a, n_voices=64)
    extra(a)
    workloads.build_headline(b, n_voices=64)
    extra(c)
    deferred = []
    ya = _writes(a, [MF] * blocks, lambda k, pos: deferred.append(a.deferred_units()))
    yb, yc = _writes(b, [MF] * blocks), _writes(c, [MF] * blocks)
    assert deferred[2:] == [1] * (blocks - 2), deferred
    d = np.abs(ya.astype(np.float64) - yb.astype(np.float64) - yc.astype(np.float64)).max()
    print(f"untouched graph: max difference {d:.3e}")
    assert np.abs(yc).max() > 0.01 and d <= 1e-6
    assert a.device_errors() == 0


def test_sharded_equals_single():
    """Enveloped voices on both shards of ShardedGraph([0, 0]) = the single graph, bit for bit. One sub-mixer per shard, two enveloped voices
    each: the single graph's mixer sum adds the sub-mixers in unit order, (0 + m1) + m2, the sharded handle adds the shards' partial buses,
    (0 + m1) + (0 + m2) — the same f32 sum. (With several sub-mixers per shard the two orders differ, (m1 + m3) + (m2 + m4) against
    ((m1 + m2) + m3) + m4, by a rounding of the bus sum with or without envelopes: tests/test_gpu_graph.py holds such graphs to 2e-5.)"""
    n = 16 * MF

    def build(g):
        ids = []
        for mi in range(2):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_GAIN, {"gain": 0.9})
            for k in range(2):
                i = 2 * mi + k
                v = g.add_voice(m, _tone(i, n + 64), 2, SR, volume=0.5, panning=float(np.float32(workloads.voice_pan(i))))
                g.set_voice_envelope(v, attack_s=0.01 * (i + 1), hold_s=0.02, decay_s=0.05, sustain_level=0.5, release_s=0.04)
                g.release_voice(v, 5 * MF + 101 * i + 7)
                ids.append(v)
        return g, ids

    single, _ = build(Graph(SR, 2, MF, 0))
    sharded, ids = build(ShardedGraph([0, 0], SR, 2, MF))
    assert sharded.shard_of_mixer(1) != sharded.shard_of_mixer(2)
    stages = []
    ys, yh = _writes(single, [MF] * 16), _writes(sharded, [MF] * 16, lambda k, pos: stages.append([sharded.voice_envelope_stage(v) for v in ids]))
    assert np.abs(ys).max() > 0.01
    assert np.array_equal(ys, yh), (int(np.flatnonzero(ys != yh)[0]) // 2, float(np.abs(ys - yh).max()))
    assert all(s in (M.ATTACK, M.HOLD, M.DECAY) for s in stages[0]) and stages[-1] == [M.IDLE] * 4   # forwarded to the voices' shards
    assert not any(sharded.is_voice_playing(v) for v in ids) and sharded.device_errors() == 0
