"""tests/granular_sampler_model.py pinned by cases derived by hand from the reference (src/generator/sampler.rs, src/generator/sampler/voice.rs,
granular.rs, src/modulation/matrix.rs): none of the expected values comes from the device code. No GPU.

The arithmetic the cases lean on:
  - one grain per note (granular_sampler_rig.ONE_GRAIN): Cloud at 100 Hz fires at the note's first frame (GrainPool::start sets trigger_phase
    to 1.0) and not again within 470 frames (1 / (100 / 48000) = 480); a grain of 2 ms without variation is 96 frames long and sounds at frames
    t .. t + 95 of a note started at t; after GrainPool::stop the pool is exhausted with frame t + 95;
  - a release of 50 frames from level 1.0 (FLAT_ENV): the raw level falls by 0.02 per frame, it is about 0.02 after 49 frames and at most
    rounding noise after 50 — at or below the -60 dB floor of 0.001: Idle with the 50th frame behind the note-off."""
import numpy as np

import ahdsr_model as A
import granular_model as gm
import granular_sampler_model as G
import granular_sampler_rig as R
import modulation_model as mm

F32 = np.float32


def _rig(n, **kw):
    return R.Rig(None, None, [0], n, **kw)


def test_allocation_free_slot_then_earliest_release_then_oldest_id():
    """next_free_voice_index (sampler.rs:826-860)."""
    r = _rig(3, kw=R.ONE_GRAIN, envelope=dict(R.FLAT_ENV, release_s=0.1))
    a, b, c = r.on(0, 60), r.on(0, 62), r.on(0, 64)
    R.run_model([r], [5])
    assert [r.slot_of(k) for k in (a, b, c)] == [0, 1, 2]          # free slots in index order
    r.off(6, c)
    r.off(8, b)                                                    # two slots release: c since 6, b since 8
    d = r.on(10, 65)
    e = r.on(10, 66)
    f = r.on(10, 67)
    R.run_model([r], [20], pos=5)
    assert r.slot_of(d) == 2 and r.slot_of(e) == 1                 # the earliest release first, whatever its note id
    assert r.slot_of(f) == 0                                       # nobody releases any more: the oldest id (a) — d and e are younger
    assert r.m.steals == 3
    # without an envelope a stopped voice is not "releasing": the oldest id goes, and equal keys go to the lower slot
    q = _rig(2, kw=dict(R.ONE_GRAIN, size=20.0))
    a, b = q.on(0, 60), q.on(0, 62)
    q.off(3, b)
    c = q.on(5, 64)
    R.run_model([q], [10])
    assert q.slot_of(c) == 0


def _probe(scenario, probe, **kw):
    r = _rig(3, **kw)
    c = scenario(r, probe)
    R.run_model([r], [64, 29, 300])
    return r, c


def test_a_pool_that_runs_dry_frees_its_slot_at_the_end_of_the_span():
    """A's one grain sounds through frame 95. A note at 95 ends the span [10, 95) in front of that frame: A is active, the note takes slot 2.
    A note at 96 ends the span [10, 96) behind it: A was freed with that span, the note takes slot 0."""
    r, c = _probe(R.dry_scenario, R.GRAIN_FRAMES - 1, kw=R.ONE_GRAIN)
    assert r.slot_of(c) == 2 and r.m.frees()[0] >= 1
    r, c = _probe(R.dry_scenario, R.GRAIN_FRAMES, kw=R.ONE_GRAIN)
    assert r.slot_of(c) == 0
    assert (93, 3) in r.m.span_log                                 # the span that freed it: the writes end at 64 and 93, the note cuts at 96


def test_an_envelope_that_goes_idle_frees_its_slot_at_the_end_of_the_span():
    x = 10 + R.RELEASE_FRAMES - 1                                  # Idle with frame 59
    r, c = _probe(R.idle_scenario, x, kw=R.ONE_GRAIN, envelope=R.FLAT_ENV)
    assert r.slot_of(c) == 2
    r, c = _probe(R.idle_scenario, x + 1, kw=R.ONE_GRAIN, envelope=R.FLAT_ENV)
    assert r.slot_of(c) == 0 and r.m.frees()[1] >= 1
    # the envelope alone, from ahdsr_model: 49 release frames leave about 0.02, the 50th ends the release
    e, p = A.Envelope(), A.Params(R.SR, **R.FLAT_ENV)
    e.note_on(p, 1.0)
    e.run(p)
    e.note_off(p)
    levels = [float(e.run(p)) for _ in range(R.RELEASE_FRAMES)]
    assert e.stage == A.IDLE and 0.015 < levels[-2] < 0.025 and levels[-1] == 0.0


def test_an_unrelated_event_of_the_mixer_moves_the_span_end():
    """A slot that has gone Idle keeps running its scheduler, and drawing from its generator, until the write that resets it (with an envelope
    the pool goes on triggering: a trigger every 480 frames here, each with draws). A is Idle with frame 59. Without another event the span
    [10, 1200) runs on to the next message and slot 0's generator is drawn from at frames 480 and 960. With an event of the mixer at 60 the span
    ends there: the slot is reset at 60 and draws nothing more. The next note takes slot 0 either way — from another generator state, so with
    other grains. (A message is a cut itself, so at a MESSAGE's frame every slot that ended earlier is free whatever else cut the mixer: what an
    unrelated cut moves is when the slot is reset, which shows in the slot table at the end of a write and in everything the slot plays later.)"""
    kw = dict(R.ONE_GRAIN, variation=0.5)

    def one(cuts):
        r = _rig(2, kw=kw, envelope=R.FLAT_ENV)
        a = r.on(0, 60)
        r.off(10, a)
        c = r.on(1200, 67)
        R.run_model([r], [1300], cuts=cuts)
        return r, c
    r0, c0 = one(())
    r1, c1 = one((60,))
    assert r0.slot_of(c0) == 0 and r1.slot_of(c1) == 0
    assert (10, 1190) in r0.m.span_log and (10, 50) in r1.m.span_log and (60, 1140) in r1.m.span_log
    d0, d1 = r0.m.slots[0].pool.rng_draws, r1.m.slots[0].pool.rng_draws
    assert d0 > d1, (d0, d1)                                       # the uncut span went on triggering: more draws
    assert r0.m.grain_state(0)["rng"] != r1.m.grain_state(0)["rng"]
    # the slot table at the end of a write: A's slot is still taken behind frame 58, free behind frame 59
    for frames, taken in ((59, True), (60, False)):
        r = _rig(2, kw=kw, envelope=R.FLAT_ENV)
        a = r.on(0, 60)
        r.off(10, a)
        R.run_model([r], [frames])
        assert (r.m.state()["slots"][0]["note_id"] != 0) == taken


def test_a_stolen_slots_grains_are_gone_at_the_notes_frame_and_its_generator_carries_on():
    r = _rig(1, kw=dict(R.SHORT, size=20.0))
    r.on(0, 60)
    R.run_model([r], [500])
    before = r.m.grain_state(0)
    draws = r.m.slots[0].pool.rng_draws
    assert before["active"].sum() >= 2 and draws > 0
    r.on(500, 72, 0.5, 0.25)
    r.m._write_span(0, 500, np.zeros((0, 2), F32))                 # the messages of frame 500 alone: SamplerVoice::start
    after = r.m.grain_state(0)
    assert after["active"].sum() == 0 and (after["samples_remaining"] == 0).all() and after["primary"] == -1
    assert after["rng"] == before["rng"] and r.m.slots[0].pool.rng_draws == draws            # not reseeded, nothing drawn
    assert after["trigger_phase"] == F32(1.0) and after["playhead"] == F32(R.SHORT["position"]) and after["trigger_new_grains"] == 1
    assert after["volume"] == F32(0.5) and after["panning"] == F32(0.25) and after["speed"] == 2.0   # speed_from_note(72): an octave
    assert r.m.steals == 1


def test_note_on_resets_both_lfos_and_sets_velocity_and_keytracking():
    mod = dict(rates=(5.0, 9.0), waveforms=(mm.SINE, mm.RANDOM), rng_states=R.LFO_RNG, routes=[(mm.LFO1, mm.SIZE, 0.5, True), (mm.LFO2, mm.SPRAY, 0.5, True)])
    r = _rig(1, modulation=mod)
    ms = r.m.modulation_state(0)
    assert ms["velocity"] == F32(0.0) and ms["note_pitch"] == F32(F32(60.0) / F32(127.0))     # no note yet
    r.on(0, 40, 0.3, 0.0)
    R.run_model([r], [1000])
    ms = r.m.modulation_state(0)
    assert ms["velocity"] == F32(0.3) and ms["note_pitch"] == F32(F32(40.0) / F32(127.0))
    assert abs(float(ms["lfo0_phase"]) - 1000 * 5.0 / 48000) < 1e-4      # 1000 f32 additions of 5 / 48000: rounding of about 1e-8 each
    hold, rng = ms["lfo1_sample_hold"], ms["lfo1_rng"]
    r.on(1000, 90, 1.0, 0.0)
    r.m._write_span(0, 1000, np.zeros((0, 2), F32))
    ms = r.m.modulation_state(0)
    assert ms["lfo0_phase"] == F32(0.0) and ms["lfo1_phase"] == F32(0.0)                    # Lfo::reset
    assert ms["lfo1_rng"] != rng and ms["lfo1_sample_hold"] != hold                          # the random shape draws again; its generator carries on
    assert ms["velocity"] == F32(1.0) and ms["note_pitch"] == F32(F32(90.0) / F32(127.0))


def test_a_setter_in_front_of_the_start_time_waits_for_it():
    """The mixer does not call the sampler before its start time: what came due earlier is applied at the top of its first write, in the order of
    the times it was stamped with (mixed.rs:565-576, :902-918)."""
    r = _rig(1, kw=R.ONE_GRAIN, start_time=100)
    a = r.on(20, 60, 1.0, 0.0)                  # held until frame 100
    r.param(10, "volume", 0.5)                  # stamped earlier: applied first
    r.vol(30, a, 0.25)                          # stamped later: applied to the started note
    audio = r.m.write(300)
    assert r.m.span_log[0] == (100, 200) and not audio[:100].any() and audio[100:196].any() and not audio[196:].any()
    st = r.m.grain_state(0)
    assert st["volume"] == F32(F32(0.5) * F32(0.25)) and r.m.state()["slots"][0]["note_volume"] == F32(0.25)
    # the one grain was activated at frame 100, before the per-note volume arrived? No: all three are applied in front of frame 100
    assert (st["volume_g"][0] == F32(0.125))


def test_derive_state_is_distinct_per_slot_and_generator():
    seen = set()
    for given in (None, R.POOL_RNG):
        for k in range(64):
            for j in range(3):
                s = G.derive_state(given, k, j)
                assert any(s) and (s[3] & 0xFF) == 3 * k + j
                seen.add(s)
    assert len(seen) == 2 * 64 * 3
