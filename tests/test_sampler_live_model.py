"""tests/sampler_live_model.py pinned on cases worked out by hand from the reference's lines (src/utils/ahdsr.rs:143-249, :402-470;
src/generator/sampler.rs:184-217, :656-731, :1148-1271; src/modulation/matrix.rs:60-83, :394-408; src/utils/dsp/lfo.rs:89-119;
src/generator/sampler/granular.rs:516-518), and the conditions the GPU tests' seeded random scripts must meet, decided by the model alone.
No GPU."""
import numpy as np
import pytest

import ahdsr_model as A
import granular_sampler_rig as R
import modulation_model as mm
import sampler_live_model as L
import sampler_live_rig as LR

F = np.float32
SR = 48000
ENV = dict(attack_s=0.002, hold_s=0.003, decay_s=0.004, sustain_level=0.6, release_s=0.005)   # 96 / 144 / 192 / 240 frames


def _file_model(**kw):
    return L.LiveSamplerModel(SR, 6001, 2, SR, voice_count=2, envelope=ENV, **kw)


def test_duration_round_trip_edges():
    """from_secs_f32 rounds to the nearest nanosecond: 4e-10 s is a zero Duration (a rate of f32::MAX), 0.6e-9 s is 1 ns; as_secs_f32 is
    `secs as f32 + nanos as f32 / 1e9f32`."""
    assert L.duration_round_trip(4e-10) == (F(0.0), True)
    assert L.duration_round_trip(0.6e-9) == (F(F(1.0) / F(1e9)), False)
    assert L.duration_round_trip(-1.0) == (F(0.0), True)                                # seconds.max(0.0)
    assert L.duration_round_trip(0.008) == (F(F(8000000.0) / F(1e9)), False)            # f32(0.008) = 0.00800000038 s -> 8 000 000 ns
    assert L.duration_round_trip(2.5) == (F(2.5), False)                                # 2 s + 500 000 000 ns
    assert L.duration_round_trip(1.5e-9) == (F(F(2.0) / F(1e9)), False)                 # f32(1.5e-9) lies above 1.5e-9: 2 ns
    p = A.Params(SR, **ENV)
    for fourcc, rate in (("AATK", "attack_rate"), ("ADCY", "decay_rate"), ("AREL", "release_rate")):
        L.apply_envelope_parameter(p, fourcc, F(4e-10))
        assert getattr(p, rate) == A.F32_MAX
    L.apply_envelope_parameter(p, "AATK", F(0.6e-9))
    assert p.attack_rate == F(F(1.0) / F(F(F(1.0) / F(1e9)) * F(SR))) and np.isfinite(p.attack_rate)
    assert L.envelope_state(p)["zero_times"] == L.DECAY_ZERO | L.RELEASE_ZERO


def test_descriptors_and_resolution():
    assert [d[0] for d in L.ENV_DESCRIPTORS] == list(L.ENV_IDS)
    assert L.resolve_envelope("AATK", 12.0, False) == F(10.0) and L.resolve_envelope("AREL", -1.0, False) == F(0.0)
    assert L.resolve_envelope("ASTN", 1.5, False) == F(1.0)
    assert L.resolve_envelope("ADCY", 0.5, True) == F(2.5)            # Exponential(2.0): 0.25 of 0..=10
    assert L.resolve_envelope("ADCY", 1.5, True) == F(10.0)           # clamped to 0..=1 first
    assert L.resolve_envelope("ASTN", 0.25, True) == F(0.25)          # linear
    with pytest.raises(ValueError):
        L.resolve_envelope("SVOL", 1.0, False)
    with pytest.raises(ValueError):
        L.resolve_envelope("AATK", float("nan"), False)


def test_sustain_alone_leaves_the_decay_rate_stale():
    m = _file_model()
    before = m.envelope_state()
    assert before["decay_rate"] == F(F(F(1.0) - F(0.6)) / F(F(0.004) * F(SR)))
    m.set_envelope_parameter("ASTN", 0.2, t=100)
    m.write(300)
    after = m.envelope_state()
    assert after["sustain_level"] == F(0.2) and after["decay_rate"] == before["decay_rate"]
    assert {k for k in after if after[k] != before[k]} == {"sustain_level"}


@pytest.mark.parametrize("order", ["in_time_order", "decay_sent_first"])
def test_decay_behind_sustain_divides_by_the_new_sustain(order):
    """ASTN stamped 100, ADCY stamped 200: whichever is SENT first, the decay setter runs second and sees sustain 0.2."""
    m = _file_model()
    calls = [("ASTN", 0.2, 100), ("ADCY", 0.008, 200)]
    for fourcc, value, t in (calls if order == "in_time_order" else calls[::-1]):
        m.set_envelope_parameter(fourcc, value, t=t)
    m.write(150)
    mid = m.envelope_state()
    assert mid["sustain_level"] == F(0.2) and mid["decay_rate"] == F(F(F(1.0) - F(0.6)) / F(F(0.004) * F(SR)))   # the ADCY is not due yet
    m.write(150)
    assert m.envelope_state()["decay_rate"] == F(F(F(1.0) - F(0.2)) / F(F(F(8000000.0) / F(1e9)) * F(SR)))


def test_decay_in_front_of_sustain_keeps_the_old_sustain():
    m = _file_model()
    m.set_envelope_parameter("ADCY", 0.008, t=100)
    m.set_envelope_parameter("ASTN", 0.2, t=200)
    m.write(300)
    assert m.envelope_state()["decay_rate"] == F(F(F(1.0) - F(0.6)) / F(F(F(8000000.0) / F(1e9)) * F(SR)))


def _run_until(e, p, pred, limit=100000):
    n = 0
    while not pred(e):
        e.run(p)
        n += 1
        assert n < limit
    return n


def test_hold_time_during_hold_does_not_touch_the_running_hold():
    """hold_samples_remaining is set where Attack ends (ahdsr.rs: hold_time * sample_rate = 144) and counted down one per frame: the frame that
    ends the attack and the 143 behind it end in Hold whatever AHLD says in between."""
    p, e = A.Params(SR, **ENV), A.Envelope()
    e.note_on(p, 1.0)
    _run_until(e, p, lambda e: e.stage == A.HOLD)
    in_hold = 1
    for _ in range(50):
        e.run(p)
        in_hold += 1
    L.apply_envelope_parameter(p, "AHLD", F(0.01))
    assert p.hold_samples == F(480.0) and e.hold_samples_remaining == F(144.0 - 50.0)
    in_hold += _run_until(e, p, lambda e: e.stage != A.HOLD) - 1
    assert in_hold == 144 and e.stage == A.DECAY


def test_zero_hold_during_attack_skips_hold():
    p, e = A.Params(SR, **ENV), A.Envelope()
    e.note_on(p, 1.0)
    for _ in range(10):
        e.run(p)
    L.apply_envelope_parameter(p, "AHLD", F(0.0))
    seen = set()
    while e.stage == A.ATTACK:
        e.run(p)
        seen.add(e.stage)
    assert e.stage == A.DECAY and A.HOLD not in seen and e.output == F(1.0)


def test_zero_attack_mid_attack_reaches_the_target_on_the_next_frame():
    p, e = A.Params(SR, **ENV), A.Envelope()
    e.note_on(p, 1.0)
    for _ in range(10):
        e.run(p)
    assert e.stage == A.ATTACK and F(0.0) < e.output < F(0.2)
    L.apply_envelope_parameter(p, "AATK", F(0.0))
    assert p.attack_rate == A.F32_MAX
    e.run(p)
    assert e.output == F(1.0) and e.stage == A.HOLD


def test_zero_release_then_note_off_frees_the_slot_with_that_write():
    m = _file_model()
    nid = m.note_on(60, 1.0, 0.0, t=0)
    m.set_envelope_parameter("AREL", 0.0, t=100)
    m.note_off(nid, t=150)
    st = m.write(300)
    rec = m.notes[nid]
    assert st["active_voices"] == 0 and st["slots"][0]["note_id"] == 0 and st["slots"][0]["envelope_stage"] == A.IDLE
    assert rec.end == 300 and rec.release_frames == [150]
    assert all(g == 0 for g in rec.gains[150:]) and rec.gains[149] > 0      # Idle at once: no release tail
    assert m.envelope_state()["zero_times"] == L.RELEASE_ZERO


MOD = dict(rates=(7.0, 13.0), waveforms=(mm.SINE, mm.TRIANGLE), rng_states=R.LFO_RNG, routes=[])


def _granular_model(voice_count=2, **kw):
    kw.setdefault("modulation", MOD)
    return L.LiveGranularSamplerModel(SR, R.BUF, R.model_params(dict(R.SHORT, size=8.0), kw.pop("loop_range", None)), voice_count=voice_count, **kw)


def test_route_set_while_a_slot_is_free_sounds_in_its_next_note():
    m = _granular_model()
    m.note_on(60, 1.0, 0.0, t=0)                                  # slot 0
    m.set_modulation(mm.VELOCITY, mm.DENSITY, 0.4, False, t=100)    # slot 1 is free
    m.note_on(64, 0.5, 0.0, t=200)                                # slot 1
    m.write(300)
    assert [a[2] for a in m.allocations] == [0, 1]
    for k, velocity in ((0, 1.0), (1, 0.5)):
        st = m.modulation_state(k)
        assert st["amount"][mm.VELOCITY, mm.DENSITY] == F(0.4) and st["bipolar"][mm.VELOCITY, mm.DENSITY] == 0
        assert st["last"][mm.DENSITY] == F(F(velocity) * F(0.4))   # a unipolar source, not bipolar: the value itself
    m.clear_modulation(mm.VELOCITY, mm.DENSITY, t=310)
    m.set_modulation(mm.KEYTRACK, mm.SPRAY, 0.0005, True, t=310)    # below update_target's threshold: no route
    m.write(100)
    for k in (0, 1):
        st = m.modulation_state(k)
        assert not st["amount"].any() and not st["bipolar"].any() and st["last"][mm.DENSITY] == 0


def test_lfo_rate_and_waveform_survive_note_on():
    m = _granular_model()
    m.set_lfo_rate(0, 5.0, t=50)
    m.set_lfo_rate(1, 100.0, t=50)          # clamped to 20 Hz
    m.set_lfo_waveform(1, mm.SQUARE, t=60)
    before = m.modulation_state(1)
    m.note_on(60, 1.0, 0.0, t=100)
    m.write(80)
    st = m.modulation_state(0)
    assert st["lfo0_phase_inc"] == F(float(F(5.0)) / SR) and st["lfo1_phase_inc"] == F(float(F(20.0)) / SR) and st["lfo1_waveform"] == mm.SQUARE
    free = m.modulation_state(1)             # the free slot took them too, and nothing else of it moved: no draw, no phase change
    assert free["lfo0_phase_inc"] == st["lfo0_phase_inc"] and free["lfo1_waveform"] == mm.SQUARE
    for key in ("lfo0_rng", "lfo1_rng", "lfo0_phase", "lfo1_phase", "lfo0_sample_hold", "lfo1_jitter_target"):
        assert free[key] == before[key], key
    m.write(100)                             # the note's reset at frame 100 keeps rate and waveform
    st = m.modulation_state(0)
    assert st["lfo0_phase_inc"] == F(float(F(5.0)) / SR) and st["lfo1_waveform"] == mm.SQUARE and st["lfo0_phase"] > 0


def test_loop_range_none_means_no_loop():
    m = _granular_model(loop_range=(0.2, 0.5))                      # what creation resolved the buffer's embedded loop to
    assert m.params_state()["has_loop_range"] == 1
    m.note_on(60, 1.0, 0.0, t=0)
    m.set_loop_range((300, 1500), t=40)
    m.write(50)
    ps = m.params_state()
    assert ps["has_loop_range"] == 1 and ps["loop_start"] == F(F(300.0) / F(3000.0)) and ps["loop_end"] == F(F(1500.0) / F(3000.0))
    m.set_loop_range(None, t=60)
    m.write(50)
    assert m.params_state()["has_loop_range"] == 0
    for bad in ((3000, 3001), (0, 3001), (5, 5), (9, 4)):
        with pytest.raises(ValueError):
            m.set_loop_range(bad)


def test_messages_while_stopping_change_nothing():
    m = _granular_model(envelope=ENV, transient=True, loop_range=(0.2, 0.5))
    m.note_on(60, 1.0, 0.0, t=0)
    m.stop(t=50)
    m.set_envelope_parameter("ASTN", 0.1, t=60)
    m.set_envelope_parameter("AREL", 0.0, t=60)
    m.set_modulation(mm.LFO1, mm.SIZE, 0.7, True, t=61)
    m.set_lfo_rate(0, 3.0, t=62)
    m.set_lfo_waveform(0, mm.RANDOM, t=63)
    m.set_loop_range(None, t=64)
    m.write(55)
    env, mod, ps = m.envelope_state(), m.modulation_state(1), m.params_state()
    m.write(45)
    assert m.stopping and m.envelope_state() == env and m.params_state() == ps and m.live_log == [] and m.env_log == []
    after = m.modulation_state(1)
    assert all(np.array_equal(after[k], mod[k]) for k in mod)

    f = _file_model(transient=True)
    f.note_on(60, 1.0, 0.0, t=0)
    f.stop(t=50)
    f.set_envelope_parameter("ADCY", 1.0, t=60)
    env = f.envelope_state()
    f.write(100)
    assert f.stopping and f.envelope_state() == env


def test_a_sampler_without_an_envelope_or_a_matrix_refuses():
    with pytest.raises(ValueError):
        L.LiveSamplerModel(SR, 6001, 2, SR, voice_count=2).set_envelope_parameter("AATK", 0.1)
    m = _granular_model(modulation=None)
    for call in (lambda: m.set_modulation(0, 0, 0.5), lambda: m.set_lfo_rate(0, 1.0), lambda: m.set_lfo_waveform(0, 1)):
        with pytest.raises(ValueError):
            call()


# ---- the GPU tests' seeded random scripts: what each must contain, so that the GPU test never skips ----
@pytest.mark.parametrize("n_slots,seed", LR.SCRIPT_CASES)
def test_random_scripts_meet_their_conditions(n_slots, seed):
    r = LR.GRig(None, None, [0], n_slots, envelope=LR.SCRIPT_ENV, modulation=LR.SCRIPT_MOD)
    LR.random_script(r, LR.script_rng(n_slots, seed), n_slots)
    R.run_model([r], LR.SCRIPT_SIZES)
    cond = LR.script_conditions(r.m)
    assert all(cond.values()), cond
    assert max(r.times) < LR.SCRIPT_FRAMES
