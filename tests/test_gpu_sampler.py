"""The Sampler's note layer on the GPU (pg_graph_add_sampler and the pg_graph_sampler_* messages) against tests/sampler_model.py and the CPU
oracle. 48 kHz, pieces of 1024 frames, the sampler alone in an effect-less sub-mixer unless a case says otherwise.

Expected audio: every note of the model is rendered as one ordinary voice of an OracleGraph that starts at the model's start frame with the
smoother values the slot handed down (the set-targets follow at its start), gets the model's speed, volume, panning and stop events, is cut at
the frame the model says it was stolen or freed at, and is multiplied by the model's envelope gains in f32; the notes are then added in slot
order in f32 — the reference's own order (sampler.rs:989-1006). Compared with np.array_equal. The slot table of pg_graph_sampler_state after
EVERY write equals the model's, field by field. Where a sampler shares its mixer or sits in front of an effect (case 10) the bound is the one
tests/test_gpu_ahdsr.py uses against the oracle: RMS <= 1e-5, max <= 1e-4.

Scripts keep every message of a sampler on a frame of its own unless the case is about messages that share one: two volume set-targets of one
source at one frame reach an oracle voice through a one-slot queue (mixed.rs:810-845), which a sampler's direct calls do not have."""
import numpy as np
import pytest

import oracle
from phonic_amd import _capi, workloads
from phonic_amd._wrap import PhonicError
from phonic_amd.graph import Graph
from sampler_rig import ENV, LONG, MF, SHORT, SR, UNKNOWN, Rig, _assert_equal, _note_audio, _run, _single, expected_audio, resolve  # noqa: F401

pytestmark = pytest.mark.gpu


def _slots(r):
    return [s["note_id"] for s in r.m.state()["slots"]]


def test_01_first_free_order_and_reuse():
    g, r = _single(SHORT, 4)
    a, b, c, d = r.on(0, 60), r.on(300, 62), r.on(1024, 57), r.on(2047, 64)
    e = r.on(7000, 65)     # behind the write in which note a (6001 frames at speed 1) ended: slot 0 again
    n = 14
    got = _run(g, [r], [MF] * n)
    notes = r.m.notes
    assert [notes[r.ids[k]].slot for k in (a, b, c, d, e)] == [0, 1, 2, 3, 0]
    assert notes[r.ids[a]].end == 6 * MF and not notes[r.ids[a]].stolen
    _assert_equal(got, expected_audio(r.m, SHORT, n * MF))


def test_02_third_note_steals_the_lowest_id():
    g, r = _single(LONG, 2)
    a, b, c = r.on(0, 60, 0.9, -0.2), r.on(500, 64, 0.8, 0.3), r.on(1500, 67, 0.7, 0.1)
    got = _run(g, [r], [MF] * 6)
    rec = r.m.notes[r.ids[a]]
    assert rec.stolen and rec.end == 1500 and r.m.notes[r.ids[c]].slot == 0
    _assert_equal(got, expected_audio(r.m, LONG, 6 * MF))


def test_03_envelope_stealing_and_idle():
    g, r = _single(LONG, 3, envelope=ENV)
    a, b, c = r.on(0, 60), r.on(10, 62), r.on(20, 64)
    r.off(1000, b)
    r.off(1500, a)
    d = r.on(2000, 65)      # the earliest release (b, slot 1), not the oldest id
    e = r.on(8000, 67)      # a's release (0.1 s from 1500) reached Idle: slot 0 is free, nothing is stolen
    r.off(9000, c)
    r.all_off(9200)         # c moves from 9000 to 9200 and ties with d and e
    r.off(9300, d)
    f = r.on(9500, 69)      # c (slot 2) and e (slot 0) tie at 9200: the lower slot goes; without the all_notes_off it would have been c
    n = 16
    got = _run(g, [r], [MF] * n)
    notes = r.m.notes
    assert [notes[r.ids[k]].slot for k in (d, e, f)] == [1, 0, 0]
    assert notes[r.ids[b]].stolen and not notes[r.ids[a]].stolen and notes[r.ids[e]].stolen and notes[r.ids[e]].end == 9500
    _assert_equal(got, expected_audio(r.m, LONG, n * MF))


def test_04_fade_out_without_envelope():
    g, r = _single(LONG, 2)
    a, b = r.on(0, 60), r.on(100, 62)
    r.off(1000, b)          # the 50 ms fade-out
    c = r.on(3000, 64)      # during the fade, both slots busy: a goes (lowest id), the fading voice is not "releasing"
    d = r.on(8000, 65)      # b's fader has arrived: slot 1 is free
    n = 12
    got = _run(g, [r], [MF] * n)
    notes = r.m.notes
    assert notes[r.ids[a]].stolen and notes[r.ids[a]].end == 3000 and notes[r.ids[c]].slot == 0
    assert not notes[r.ids[b]].stolen and 1000 + 2400 < notes[r.ids[b]].end < 8000 and notes[r.ids[d]].slot == 1
    _assert_equal(got, expected_audio(r.m, LONG, n * MF))


def test_05_base_parameters():
    g, r = _single(LONG, 3)
    a, b = r.on(0, 60, 0.8, 0.3), r.on(200, 64, 1.0, -0.5)
    r.speed(500, a, 1.5, glide=12.0)
    r.param(1500, "transpose", 12)          # retunes a and b at that frame and ends a's glide
    r.param(2500, "finetune", -30)
    r.param(3300, "volume", 0.5)
    r.param(4100, "panning", 0.9)           # a: 0.3 + 0.9 clamps to 1.0
    r.param(5000, "volume", 0.8, normalized=True)
    r.param(5500, "transpose", 0.25, normalized=True)
    r.param(5700, "finetune", 0.5, normalized=True)
    r.param(6000, "panning", 0.5, normalized=True)
    c = r.on(6500, 55, 0.6, 0.2)            # a new note composes with the base values of that frame
    n = 10
    got = _run(g, [r], [MF] * n)
    st = r.m.state()
    assert (st["transpose"], st["finetune"]) == (-24, 0) and float(st["panning"]) == 0.0 and 2.0 < float(st["volume"]) < 2.6
    assert [x[1] for x in r.m.notes[r.ids[a]].panning_events][:2] == [np.float32(0.3), np.float32(1.0)]
    assert r.m.notes[r.ids[a]].speed_events[2] == (1500, 2.0, None)
    _assert_equal(got, expected_audio(r.m, LONG, n * MF))


def test_06_per_note_setters_live_ended_unknown():
    g, r = _single(SHORT, 3)
    a, b = r.on(0, 48), r.on(100, 60)       # a at half speed: 12000 frames; b ends at 6101, inside the sixth write
    r.speed(1000, a, 0.8, glide=24.0)
    r.vol(2000, a, 0.5)
    r.pan(3000, a, -0.7)
    for t, k in ((7000, b), (7600, None)):  # an ended note, then an id nobody has: all ignored
        r.vol(t, k, 0.1)
        r.pan(t + 100, k, 0.9)
        r.speed(t + 200, k, 2.0)
        r.off(t + 300, k)
    n = 14
    got = _run(g, [r], [MF] * n)
    assert len(r.m.notes[r.ids[b]].volume_events) == 1 and r.m.notes[r.ids[b]].end == 6 * MF
    assert r.m.notes[r.ids[a]].end is not None
    _assert_equal(got, expected_audio(r.m, SHORT, n * MF))


def test_07_reused_slot_inherits_the_smoothers():
    g, r = _single(LONG, 1)
    a = r.on(0, 60, 0.2, -0.8)
    b = r.on(3000, 62, 0.9, 0.6)            # a's ramps are done: from 0.2 / -0.8
    c = r.on(3200, 64, 0.4, -0.1)           # b's ramps are under way
    got = _run(g, [r], [MF] * 6)
    na, nb, nc = (r.m.notes[r.ids[k]] for k in (a, b, c))
    assert (float(na.inherited_volume), float(na.inherited_panning)) == (1.0, 0.0)      # a fresh slot: AmplifiedSource(1.0), PannedSource(0.0)
    # (an exponential smoother rests where its step falls to 100 f32 epsilons, smoothing.rs:198-206: within 100 * eps * 256 * 48000 / 44100 of its target)
    rest = 100 * 1.1920929e-07 * 256 * 48000 / 44100 * 1.001
    assert abs(float(nb.inherited_volume) - 0.2) <= rest and abs(float(nb.inherited_panning) + 0.8) <= rest
    assert 0.25 < float(nc.inherited_volume) < 0.85 and -0.75 < float(nc.inherited_panning) < 0.55
    _assert_equal(got, expected_audio(r.m, LONG, 6 * MF))


@pytest.mark.parametrize("transient", [True, False])
def test_08_stop(transient):
    g, r = _single(LONG, 2, envelope=ENV, transient=transient)
    a, b = r.on(0, 60), r.on(100, 64)
    r.stop(2000)
    c = r.on(2500, 67)                      # dropped by a transient sampler that is stopping
    n = 8
    got = _run(g, [r], [MF] * n)
    st = r.m.state()
    if transient:
        assert r.ids[c] not in r.m.notes and st["stopping"] and st["stopped"] and st["active_voices"] == 0
        g.write(np.zeros(2 * MF, np.float32), n * MF)        # the host has seen `stopped`: the pool has left the mixer
        with pytest.raises(PhonicError) as e:
            g.sampler_note_on(r.s, 60)
        assert e.value.code == _capi.PG_ERR_NOT_FOUND
        g.add_mixer()                                         # a graph-changing call: the retired voices' buffer references return
        assert g.sample_buffer_info(r.buf)["use_count"] == 0
        late = np.zeros(2 * MF, np.float32)
        g.write(late, (n + 1) * MF)
        assert not late.any()
    else:
        assert r.m.notes[r.ids[c]].slot == 0 and not st["stopping"] and not st["stopped"] and st["active_voices"] == 1
        assert g.sample_buffer_info(r.buf)["use_count"] == 2
    _assert_equal(got, expected_audio(r.m, LONG, n * MF))


def test_09_piece_independence():
    """128-frame writes, 1024-frame writes and one write of the whole length: bit-identical audio and the same final state. (Envelope releases
    and ends of file only: where a 50 ms fade-out's last, inaudible frames end depends on the chunk it arrives in — by the reference's rule.)"""
    n = 12 * MF
    outs, finals = [], []
    for sizes in ([128] * (n // 128), [MF] * (n // MF), [n]):
        g, r = _single(SHORT, 3, envelope=ENV)
        a, b, c = r.on(0, 60), r.on(700, 55), r.on(1300, 67)
        r.off(2100, a)
        d = r.on(2500, 62)
        r.off(3000, c)
        e = r.on(4200, 58)
        r.param(5000, "transpose", 3)
        f = r.on(9000, 60)
        got = _run(g, [r], sizes)
        _assert_equal(got, expected_audio(r.m, SHORT, n))
        outs.append(got)
        finals.append(g.sampler_state(r.s))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
    assert finals[0] == finals[1] == finals[2]


def test_10_three_samplers_effects_and_shared_frames():
    """Three samplers in three sub-mixers, a reverb behind one, ordinary voices beside another, two messages at one sample time. No stealing and
    no envelope: the whole graph has an oracle twin whose voices are the model's notes. Tolerance bound (shared mixers, an effect)."""
    seeds = (16386, 16386, [0.1 * i for i in range(16)])
    g = Graph(SR, 2, MF, 0)
    o = oracle.OracleGraph(SR, 2, MF)
    ids = [0]
    mixers, gpu_mixers, rigs = [], [], []
    for k in range(3):
        mg, mo = g.add_mixer(), o.add_mixer()
        if k == 1:
            g.add_effect(mg, _capi.FX_REVERB, reverb_seeds=seeds)
            o.add_effect(mo, _capi.FX_REVERB, reverb_seeds=seeds)
        mixers.append(mo)
        gpu_mixers.append(mg)
        rigs.append(Rig(g, mg, SHORT if k != 2 else LONG, ids, 4))
    plain = workloads.tone_buffer(5, SR, 0.2)
    for start in (0, 2000):
        g.add_voice(gpu_mixers[0], plain, 2, SR, start_time=start, volume=0.5)
        o.add_voice(mixers[0], plain, 2, SR, start_time=start, volume=0.5)
    r0, r1, r2 = rigs
    r0.on(0, 60, 0.8, -0.3), r1.on(100, 64, 0.7, 0.4), r2.on(200, 55)
    k = r2.on(1000, 62)
    r2.off(1000, k)                          # same sample time, in this order: the note starts and fades from its first frame
    r1.off(1500, None)
    r1.off(1500, 0)                          # an unknown id, then the live one, at one frame
    r0.param(3000, "volume", 0.5)
    r0.on(3000, 67, 1.0, 0.2)                # the base volume first: the note's first target is 0.5
    r1.on(5000, 60)
    n = 10
    got = _run(g, rigs, [MF] * n)
    assert r2.m.state()["slots"][1]["release_start_frame"] is None and r2.m.notes[r2.ids[k]].stop_frames == [1000]
    assert r0.m.notes[r0.ids[1]].volume_events == [(3000, np.float32(0.5))]
    for rig, mo in zip(rigs, mixers):
        for rec in rig.m.notes.values():
            assert not rec.stolen
            v = o.add_voice(mo, rig.pcm, 2, SR, volume=float(rec.inherited_volume), panning=float(rec.inherited_panning), speed=rec.speed_events[0][1], start_time=rec.start)
            for t, x in rec.volume_events:
                o.set_voice_volume(v, float(x), t)
            for t, x in rec.panning_events:
                o.set_voice_panning(v, float(x), t)
            for t in rec.stop_frames:
                o.stop_voice(v, t)
    exp = o.render(n, MF)
    d = got.astype(np.float64) - exp.astype(np.float64)
    rms, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"three samplers: rms {rms:.3e} max {mx:.3e} (signal peak {np.abs(exp).max():.3f})")
    assert np.abs(exp).max() > 1e-2
    assert rms <= 1e-5 and mx <= 1e-4


def _random_script(r, rng, n_frames, n_messages):
    """About n_messages messages on distinct frames, sent in frame order: note-ons (half of them), note-offs, the per-note setters on living,
    ended and unknown ids, base parameters, all-notes-off."""
    frames = sorted(int(x) for x in rng.choice(np.arange(1, n_frames - 1), size=n_messages, replace=False))
    for t in frames:
        u = rng.random()
        k = int(rng.integers(0, len(r.ids))) if r.ids and rng.random() < 0.9 else None
        if u < 0.5 or not r.ids:
            r.on(t, int(rng.integers(48, 73)), float(np.float32(rng.uniform(0.2, 1.0))), float(np.float32(rng.uniform(-1.0, 1.0))))
        elif u < 0.68:
            r.off(t, k)
        elif u < 0.74:
            r.vol(t, k, float(np.float32(rng.uniform(0.0, 1.2))))
        elif u < 0.80:
            r.pan(t, k, float(np.float32(rng.uniform(-1.0, 1.0))))
        elif u < 0.85:
            r.speed(t, k, float(rng.uniform(0.5, 2.0)), glide=float(rng.uniform(6.0, 48.0)) if rng.random() < 0.5 else None)
        elif u < 0.96:
            name = ("transpose", "finetune", "volume", "panning")[int(rng.integers(0, 4))]
            normalized = bool(rng.random() < 0.5)
            raw = dict(transpose=int(rng.integers(-12, 13)), finetune=int(rng.integers(-100, 101)), volume=float(np.float32(rng.uniform(0.1, 1.5))),
                       panning=float(np.float32(rng.uniform(-1.0, 1.0))))[name]
            r.param(t, name, float(np.float32(rng.uniform(0.3, 0.7))) if normalized else raw, normalized)
        else:
            r.all_off(t)


@pytest.mark.parametrize("envelope", [False, True])
@pytest.mark.parametrize("voice_count", [1, 2, 5, 8])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_11_random_scripts(seed, voice_count, envelope):
    n = 72     # 1.5 s
    g, r = _single(SHORT, voice_count, envelope=ENV if envelope else None)
    _random_script(r, np.random.default_rng(1000 * seed + 10 * voice_count + int(envelope)), n * MF, 200)
    got = _run(g, [r], [MF] * n)
    assert sum(1 for rec in r.m.notes.values() if rec.stolen) > 0 or voice_count == 8
    _assert_equal(got, expected_audio(r.m, SHORT, n * MF))
