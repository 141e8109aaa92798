"""Granular-mode samplers on the device (pg_graph_add_granular_sampler: pg_gsampler_kernel between the pg_grain_kernel launches of the spans of
the sampler's source-write grid) against the independent model tests/granular_sampler_model.py. Everything goes through the C ABI.

48 kHz, a 3000-frame mono buffer (at the graph's rate it is its own granular buffer), max_frames 256, writes of mixed lengths — one below a tile
(< 32 frames), one across a chunk (> 4096) and one of 1 frame — and grains of a few milliseconds, so that pools run dry inside a write. After EVERY
write (tests/granular_sampler_rig.py: run) the slot table equals the model's field by field, every slot's grain state, every slot's matrix state
and the parameters equal the model's bit for bit, and the audio equals the model's as values (an all-zero frame may carry the other zero's sign).
Every case asserts on the model that what it is about happened, so none passes vacuously."""
import numpy as np
import pytest

import granular_model as gm
import granular_sampler_rig as R
import modulation_model as mm
from phonic_amd import _capi
from phonic_amd.graph import Graph

pytestmark = pytest.mark.gpu

SR, MF = R.SR, R.MF
SIZES = [300, 20, 4300, 1, 499]     # 5120 frames: a write across a chunk, one below a tile, one of 1 frame
MOD = dict(rates=(7.0, 13.0), waveforms=(mm.SINE, mm.RANDOM), rng_states=R.LFO_RNG,
           routes=[(mm.LFO1, mm.SIZE, 0.5, True), (mm.LFO2, mm.POSITION, 0.3, False), (mm.VELOCITY, mm.DENSITY, -0.4, False), (mm.KEYTRACK, mm.SPRAY, 0.6, True),
                   (mm.LFO2, mm.PAN_SPREAD, 0.5, True)])


def _single(voice_count, **kw):
    g = Graph(SR, 2, MF, 0)
    return g, R.Rig(g, g.add_mixer(), [0], voice_count, **kw)


def _peak(audio):
    return float(np.abs(audio).max())


# ---- 1: differential — a 1-voice sampler's one note against a lone granular voice ----
def test_one_note_equals_a_lone_granular_voice():
    """speed_from_note(60) is exactly 1.0 (utils.rs:67-70): a 1-voice sampler without an envelope whose one note_on(60, 1.0, 0.0) comes at its
    start time renders what a lone pg_graph_add_granular_voice_from_buffer voice with the same parameters, seeds and matrix renders in a twin
    sub-mixer of a second graph: state and bus are bit-equal over 3 writes."""
    start = 100
    states = [(R.POOL_RNG, R.LFO_RNG[0], R.LFO_RNG[1])]
    g, r = _single(1, modulation=MOD, rng_states=states, start_time=start)
    r.on(start, 60, 1.0, 0.0)
    h = Graph(SR, 2, MF, 0)
    hb = h.add_sample_buffer(R.BUF, 1, SR)
    v = h.add_granular_voice_from_buffer(h.add_mixer(), hb, R.capi_params(R.SHORT, rng_state=R.POOL_RNG), start_time=start)
    h.set_voice_modulation_matrix(v, rates=MOD["rates"], waveforms=MOD["waveforms"], rng_states=MOD["rng_states"], velocity=1.0, note=60, routes=MOD["routes"])
    pos, peak = 0, 0.0
    for n in (300, 17, 4300):
        a, b = np.zeros(2 * n, np.float32), np.zeros(2 * n, np.float32)
        g.write(a, pos)
        h.write(b, pos)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ("bus", pos)
        assert gm.states_equal(h.voice_grain_state(v), g.sampler_voice_grain_state(r.s, 0)) == [], ("grain state", pos)
        assert gm.states_equal(h.voice_modulation_state(v), g.sampler_voice_modulation_state(r.s, 0)) == [], ("matrix state", pos)
        r.m.write(n, pos)
        r.check_state(pos)
        peak = max(peak, _peak(a))
        pos += n
    assert peak > 0.02 and g.device_errors() == 0 and h.device_errors() == 0


# ---- 2: note placement ----
def test_note_placement_inside_pieces_and_on_edges():
    """Notes at frames 0, 1, 31, 32, 33, 63, 64 and 255 of a piece, one on a piece edge and one on a chunk edge, two on one frame in both sending
    orders, and a note-on with its note-off on the same frame."""
    g, r = _single(8, modulation=None)
    w2 = SIZES[0] + SIZES[1]                 # the third write begins here: pieces at w2 + 256 k, its first chunk ends at w2 + 4096
    piece = w2 + 2 * MF
    for k, f in enumerate((0, 1, 31, 32, 33, 63, 64, 255)):
        i = r.on(piece + f, 55 + k, 0.8, 0.1 * k - 0.3)
        if k % 2:
            r.off(piece + f + 40, i)
    r.on(w2 + 5 * MF, 70)                    # a piece edge
    r.on(w2 + 4096, 71, 0.9, -0.5)           # a chunk edge
    a = r.on(50, 60, 0.5, 0.0)
    b = r.on(50, 62, 0.7, 0.2)               # two on one frame ...
    r.off(120, a)
    r.off(120, b)
    t = w2 + 7 * MF + 5
    c = r.on(t, 64)
    d = r.on(t, 65)                          # ... and again, the note-offs in the other order
    r.off(t + 60, d)
    r.off(t + 60, c)
    e = r.on(w2 + 9 * MF + 17, 66)
    r.off(w2 + 9 * MF + 17, e)               # a note-on and its note-off on the same frame
    got, exp = R.run(g, [r], SIZES)
    assert _peak(exp[0]) > 0.02 and r.slot_of(a) != r.slot_of(b) and r.slot_of(c) != r.slot_of(d)


# ---- 3: stealing ----
@pytest.mark.parametrize("envelope", [False, True], ids=["no_envelope", "envelope"])
@pytest.mark.parametrize("voice_count", [1, 2, 3, 8, 33, 64])
def test_stealing(voice_count, envelope):
    """The pool is filled, then more notes come than it has slots: without an envelope the oldest id goes; with one, the earliest release, ties to the
    lower slot (two notes released on one frame). Then everything is released and runs out, and one more note takes slot 0: its third note, so
    the generator the slot carries from note to note shows. With 33 slots the decision lies beyond lane 31; with 64 every lane of the wave holds a slot (no lane carries the "no slot" index 64)."""
    n = voice_count
    g, r = _single(n, envelope=R.ENV if envelope else None)
    for k in range(n):
        r.on(5 + 3 * k, 48 + k % 24, 0.6 + 0.01 * (k % 7), 0.0)
    t = 5 + 3 * n + 20
    if envelope and n >= 3:
        r.off(t, n - 1)                      # the last slot releases first ...
        r.off(t + 4, 0)
        r.off(t + 4, 1)                      # ... then two on one frame: a tie, the lower slot goes first
    for k in range(4):
        r.on(t + 10 + 7 * k, 72 + k, 0.9, -0.2)
    r.all_off(t + 60)                        # grains of at most 3 ms * 1.8, a release of 5 ms: every slot is free 300 frames later
    last = r.on(t + 400, 80)
    sizes = [t + 30, 19, 1, 420]
    R.run(g, [r], sizes)
    m = r.m
    assert m.steals == 4 and r.slot_of(last) == 0 and sum(1 for a in m.allocations if a[2] == 0) >= 3
    if envelope and n >= 3:
        stolen_slots = [a[2] for a in m.allocations if a[3] is not None]
        assert stolen_slots[:3] == [n - 1, 0, 1], stolen_slots
    elif n >= 2:
        assert [a[2] for a in m.allocations if a[3] is not None][:2] == [0, 1]   # the oldest ids sit in the lowest slots


# ---- 4: the two end-of-span cases, with and without other events of the mixer chain ----
def _fx_events(g, mixer, times):
    fx = g.add_effect(mixer, _capi.FX_GAIN)
    for t in times:
        g.schedule_param(fx, "gain", 1.0, t)     # unity gain: an event of the mixer that changes no sample


@pytest.mark.parametrize("chain", ["plain", "own_event", "parent_events"])
@pytest.mark.parametrize("probe", [0, 1], ids=["one_frame_early", "at_the_end"])
@pytest.mark.parametrize("kind", ["dry", "idle"])
def test_slot_is_free_at_the_end_of_its_span(kind, probe, chain):
    """tests/test_granular_sampler_model.py's two hand-derived scenarios on the device: the pool runs dry (the envelope goes Idle) with frame x;
    a note at x finds the slot active, a note at x + 1 finds it free. An event of the owning sub-mixer or of its parent moves span ends in
    between and changes neither."""
    x = R.GRAIN_FRAMES - 1 if kind == "dry" else 10 + R.RELEASE_FRAMES - 1
    g = Graph(SR, 2, MF, 0)
    cuts = []
    if chain == "parent_events":
        parent = g.add_mixer()
        mixer = g.add_mixer(parent)
        cuts = [7, x - 20, x + 30]
        _fx_events(g, parent, cuts)
    else:
        mixer = g.add_mixer()
        if chain == "own_event":
            cuts = [40, x + 50]
            _fx_events(g, mixer, cuts)
    r = R.Rig(g, mixer, [0], 3, kw=R.ONE_GRAIN, envelope=R.FLAT_ENV if kind == "idle" else None)
    c = (R.dry_scenario if kind == "dry" else R.idle_scenario)(r, x + probe)
    got, exp = R.run(g, [r], [64, 29, 300], cuts=cuts)   # (a unity gain in the chain: the same values)
    assert r.slot_of(c) == (2 if probe == 0 else 0)


# ---- 5: the envelope across span edges ----
def test_envelope_stages_across_span_edges():
    """Attack, Hold, Decay and Sustain across span edges (the sampler's messages and the pieces cut them), a note-off during Attack, a release that
    reaches Idle inside a span, and a releasing slot retriggered."""
    env = dict(attack_s=0.004, hold_s=0.003, decay_s=0.004, sustain_level=0.5, release_s=0.004)   # 192 / 144 / 192 / 192 frames
    g, r = _single(3, envelope=env, kw=dict(R.SHORT, size=6.0))
    a = r.on(10, 60)
    b = r.on(100, 64, 0.8, 0.3)              # A is in Attack here
    r.off(160, b)                            # B: a note-off during Attack
    r.on(250, 67)                            # A in Hold; B releases
    r.off(700, a)                            # A in Sustain since frame 538
    for t in (420, 600):                     # cuts inside Decay and Sustain
        r.vol(t, a, 0.9)
    d = r.on(720, 70)                        # B's release (192 frames from 160) reached Idle inside the span [250, 420): slot 1 is free
    e = r.on(730, 72)                        # every slot is taken: A releases since 700 and is retriggered
    got, exp = R.run(g, [r], [300, 20, 4300, 1])
    assert r.slot_of(d) == 1 and r.slot_of(e) == 0 and r.m.frees()[1] >= 1 and _peak(exp[0]) > 0.02


# ---- 6: setters and parameters ----
@pytest.mark.parametrize("envelope", [False, True], ids=["no_envelope", "envelope"])
def test_setters_and_parameters(envelope):
    """set_note_speed / _volume / _panning, STRN, SFTN, SVOL and SPAN in the middle of a note and on a free pool; three set_granular_parameter calls
    in the middle of a note — overlap mode and window among them — and one on a pool with no note; a setter in front of the start time."""
    g, r = _single(2, envelope=R.ENV if envelope else None, kw=dict(R.SHORT, size=10.0), start_time=64)
    r.param(5, "volume", 0.8)                # in front of the start time: held to frame 64
    r.gparam(20, "GSIZ", 5.0)                # on a pool with no note
    r.param(30, "transpose", 3)
    a = r.on(64, 60, 0.9, 0.1)
    r.speed(150, a, 1.5, glide=12.0)
    r.vol(200, a, 0.4)
    r.pan(260, a, -0.7)
    r.gparam(330, "GOVM", 1.0)
    r.gparam(400, "GWND", 0.4, True)
    r.gparam(470, "GDEN", 0.9, True)
    r.param(520, "finetune", 0.7, True)
    r.param(560, "panning", 0.5)
    r.param(600, "volume", 0.5, True)
    r.param(640, "transpose", -5)
    r.off(900, a)
    r.param(4000, "volume", 1.2)             # the pool is free by now
    r.param(4010, "finetune", -20)
    r.speed(4020, a, 2.0)
    r.gparam(4030, "GPOS", 0.6)
    r.vol(4040, a, 0.3)                      # the note has ended: set_note_volume / _panning find no slot and change nothing
    r.pan(4050, a, 0.9)
    r.param(4060, "panning", -0.4)           # SPAN on a free pool: the base panning the next note starts from
    r.param(4070, "transpose", 2)
    b = r.on(4100, 62, 1.0, 0.0)             # ... and a later note takes what they left
    r.off(4500, b)
    got, exp = R.run(g, [r], [300, 20, 4300, 1, 499])
    assert r.m.p.overlap_mode == gm.SEQUENTIAL and r.m.transpose == 2 and _peak(exp[0]) > 0.02
    assert float(r.m.base_panning) == float(np.float32(-0.4))   # (what the late per-note setters left alone shows in the slot table of every write)


# ---- 7: stop and remove ----
def test_stop_on_a_transient_sampler_and_remove_with_notes_sounding():
    """pg_graph_sampler_stop on a transient sampler: all notes off, it stops with the write in which its last slot ends and leaves the mixer;
    messages sent after the stop are dropped. pg_graph_remove_sampler with notes sounding: silence from the next write on."""
    g = Graph(SR, 2, MF, 0)
    mixer = g.add_mixer()
    r = R.Rig(g, mixer, [0], 2, transient=True)
    a = r.on(10, 60)
    r.on(40, 64)
    r.stop(200)
    r.on(230, 67)                            # dropped: the sampler is stopping
    r.gparam(240, "GSIZ", 50.0)
    got, exp = R.run(g, [r], [300, 20, 1000])
    st = r.m.state()
    assert st["stopping"] and st["stopped"] and st["active_voices"] == 0 and len(r.m.allocations) == 2
    buf = np.zeros(2 * 64, np.float32)
    g.write(buf, 1320)                       # the host sees the word at the top of this write: the pool leaves the mixer
    assert not buf.any()
    with pytest.raises(Exception):
        g.sampler_note_on(r.s, 60, 1.0, 0.0, 0)
    q = R.Rig(g, mixer, r.m.note_ids, 2, buffer_id=r.buf)
    q.on(1400, 60)
    q.on(1410, 65)
    R.run(g, [q], [200], pos=1384)
    assert q.m.state()["active_voices"] == 2
    g.remove_sampler(q.s)
    buf = np.zeros(2 * 300, np.float32)
    g.write(buf, 1584)
    assert not buf.any() and g.device_errors() == 0


# ---- 8: a matrix ----
def test_matrix_with_all_sources_and_notes_of_different_pitch_and_velocity():
    """All four sources routed, one LFO with a random shape; notes of different pitch and velocity into ONE slot, one after the other: every
    note_on resets both LFOs (the random one draws again) and sets velocity and keytracking."""
    g, r = _single(1, modulation=MOD, kw=dict(R.SHORT, size=8.0))
    for k, (note, vel) in enumerate(((40, 0.3), (90, 1.0), (64, 0.6))):
        i = r.on(50 + 700 * k, note, vel, 0.0)
        r.off(400 + 700 * k, i)
    seen = []
    pos = 0
    for n in (300, 500, 20, 700, 1, 900):
        R.run(g, [r], [n], pos=pos)
        pos += n
        ms = r.m.modulation_state(0)
        seen.append((float(ms["velocity"]), float(ms["note_pitch"])))
    assert len(set(seen)) == 3 and len(r.m.allocations) == 3 and all(a[2] == 0 for a in r.m.allocations)


# ---- 9: seeded random scripts ----
SCRIPT_FRAMES = 24000      # 0.5 s
SCRIPT_SIZES = [300, 20, 4300, 1, 5000, 777, 4096, 3000, 6506]
assert sum(SCRIPT_SIZES) == SCRIPT_FRAMES
SCRIPT_CASES = [(1, False, 1), (1, True, 1), (2, False, 1), (2, True, 1), (5, False, 1), (5, True, 1), (8, False, 1), (8, True, 1)]   # (slots, envelope, seed)


def random_script(r, rng, n_slots):
    """About 100 messages in bursts: each burst sends three more note-ons than the pool has slots within a few frames of each other (several on
    one frame), then note-offs, setters and parameters; the pool drains before the next burst."""
    bursts = max(6, round(100 / (n_slots + 8)))
    t0 = 0
    for b in range(bursts):
        t = t0 = max(t0, b * SCRIPT_FRAMES // bursts + int(rng.integers(0, 200))) + 1
        for _ in range(n_slots + 3):
            r.on(t, int(rng.integers(48, 84)), float(np.float32(rng.uniform(0.3, 1.0))), float(np.float32(rng.uniform(-1.0, 1.0))))
            t += int(rng.integers(0, 9))
        for _ in range(5):
            t += int(rng.integers(1, 40))
            k = int(rng.integers(0, len(r.ids))) if rng.random() < 0.9 else None
            u = rng.random()
            if u < 0.3:
                r.off(t, k)
            elif u < 0.4:
                r.vol(t, k, float(np.float32(rng.uniform(0.0, 1.2))))
            elif u < 0.5:
                r.pan(t, k, float(np.float32(rng.uniform(-1.0, 1.0))))
            elif u < 0.6:
                r.speed(t, k, float(rng.uniform(0.5, 2.0)))
            elif u < 0.75:
                name = ("transpose", "finetune", "volume", "panning")[int(rng.integers(0, 4))]
                raw = dict(transpose=int(rng.integers(-12, 13)), finetune=int(rng.integers(-100, 101)), volume=float(np.float32(rng.uniform(0.1, 1.5))),
                           panning=float(np.float32(rng.uniform(-1.0, 1.0))))[name]
                r.param(t, name, raw)
            elif u < 0.9:
                fourcc = ("GSIZ", "GDEN", "GVAR", "GSPY", "GPAN", "GPOS", "GWND", "GDIR")[int(rng.integers(0, 8))]
                r.gparam(t, fourcc, float(np.float32(rng.uniform(0.0, 0.12) if fourcc in ("GSIZ",) else rng.uniform(0.0, 1.0))), True)
            else:
                r.all_off(t)
        t += int(rng.integers(1, 30))
        r.all_off(t)
        t0 = t + 400


def script_rng(n_slots, envelope, seed):
    return np.random.default_rng(9000 * seed + 10 * n_slots + int(envelope))


def script_qualifies(m):
    """From the model alone: at least 10 steals, 5 slots freed by exhaustion or Idle, 3 messages inside a span's first tile."""
    return m.steals >= 10 and sum(m.frees()) >= 5 and m.first_tile_messages >= 3


@pytest.mark.parametrize("n_slots,envelope,seed", SCRIPT_CASES)
def test_seeded_random_scripts(n_slots, envelope, seed):
    g, r = _single(n_slots, envelope=R.ENV if envelope else None, modulation=MOD if n_slots == 2 else None)
    random_script(r, script_rng(n_slots, envelope, seed), n_slots)
    got, exp = R.run(g, [r], SCRIPT_SIZES)
    assert script_qualifies(r.m), (r.m.steals, r.m.frees(), r.m.first_tile_messages)
    assert _peak(exp[0]) > 0.02


# ---- 10: two granular samplers in one sub-mixer, and one beside a file voice ----
def _assert_mixed(got, exp, what):
    """The project's bound for re-associated mixer sums."""
    d = got.astype(np.float64) - exp.astype(np.float64)
    rms, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"{what}: rms {rms:.3e} max {mx:.3e}")
    assert rms <= 1e-5 and mx <= 1e-4, (what, rms, mx)


def test_two_granular_samplers_in_one_sub_mixer():
    """Each sampler's messages are events of the shared mixer: they cut the other's spans too. Slot tables and states exact; the audio is the
    sum of the two models' within the bound for re-associated mixer sums."""
    g = Graph(SR, 2, MF, 0)
    mixer = g.add_mixer()
    ids = [0]
    r = R.Rig(g, mixer, ids, 2)
    q = R.Rig(g, mixer, ids, 3, envelope=R.ENV, kw=dict(R.SHORT, size=6.0, position=0.7), buffer_id=r.buf)
    a = r.on(10, 60)
    b = q.on(25, 64, 0.8, 0.2)
    r.on(40, 67)
    q.on(300, 70)
    r.off(310, a)
    r.on(500, 72)
    r.on(505, 74)
    q.off(600, b)
    q.on(650, 50)
    q.on(660, 52)
    q.on(670, 54)
    got, exp = R.run(g, [r, q], [300, 20, 4300, 1])
    assert r.m.steals >= 1 and q.m.steals >= 1
    _assert_mixed(got, (exp[0] + exp[1]).astype(np.float32), "two granular samplers")


def test_granular_sampler_beside_a_file_voice():
    g = Graph(SR, 2, MF, 0)
    o = Graph(SR, 2, MF, 0)
    voice_pcm = np.repeat(gm.make_buffer(6000, 9), 2)
    mixers = []
    for x in (g, o):
        mixers.append(x.add_mixer())
        v = x.add_voice(mixers[-1], voice_pcm, 2, SR, volume=0.5, start_time=40)
        x.set_voice_volume(v, 0.25, 333)       # an event of the shared mixer: a cut of the sampler's spans
    r = R.Rig(g, mixers[0], [0], 2)
    a = r.on(10, 60)
    r.on(200, 64)
    r.off(400, a)
    r.on(900, 67)
    got, exp = R.run(g, [r], [300, 20, 4300, 1], cuts=[333], audio=False)
    alone = np.zeros(2 * 4621, np.float32)
    pos = 0
    for n in (300, 20, 4300, 1):
        buf = np.zeros(2 * n, np.float32)
        o.write(buf, pos)
        alone[2 * pos:2 * (pos + n)] = buf
        pos += n
    _assert_mixed(got, (exp[0] + alone.reshape(-1, 2)).astype(np.float32), "granular sampler beside a file voice")
