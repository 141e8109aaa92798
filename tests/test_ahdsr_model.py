"""tests/ahdsr_model.py — the independent f32 model the GPU envelope tests take their expected values from — pinned against every known
answer the reference's own tests hold (src/utils/ahdsr.rs:599-664) and against analytic facts of the recurrence."""
import math

import numpy as np

import ahdsr_model as M

F = np.float32


def _kat_params():
    # the reference's test set-up: 100 ms attack, no hold, 100 ms decay, sustain 0.5, 100 ms release at 44.1 kHz
    return M.Params(44100, attack_s=0.1, hold_s=0.0, decay_s=0.1, sustain_level=0.5, release_s=0.1)


def test_note_on_enters_attack():
    env = M.Envelope()
    assert env.stage == M.IDLE
    env.note_on(_kat_params(), 1.0)
    assert env.stage == M.ATTACK and env.output == 0.0


def test_run_then_note_off_enters_release():
    p, env = _kat_params(), M.Envelope()
    env.note_on(p, 1.0)
    env.run(p)
    env.note_off(p)
    assert env.stage == M.RELEASE and env.release_output == env.output > 0.0


def test_reset_goes_to_idle():
    p, env = M.Params(M.UNINITIALIZED_SAMPLE_RATE), M.Envelope()
    env.note_on(p, 1.0)
    env.reset()
    assert env.stage == M.IDLE and env.output == 0.0


def test_apply_scaling_known_answers():
    assert abs(float(M.apply_scaling(0.5, 0.0)) - 0.5) < 1e-10
    assert M.apply_scaling(0.5, 0.5) > 0.5    # positive: logarithmic, fast start
    assert M.apply_scaling(0.5, -0.5) < 0.5   # negative: exponential, slow start
    assert M.apply_scaling(0.0, 1.0) == 0.0 and M.apply_scaling(1.0, -1.0) == 1.0 and M.apply_scaling(1.0, 1.0) == 1.0


def test_parameter_set_up_order():
    """The decay rate comes from the SECOND set-up (at the real rate, sustain level known); at the placeholder rate there is no second set-up
    and the rate still divides 1 - 0. A zero time is a rate of f32::MAX."""
    p = M.Params(48000)
    assert p.attack_rate == F(F(1.0) / F(F(0.010) * F(48000.0)))
    assert p.decay_rate == F(F(F(1.0) - F(0.75)) / F(F(0.5) * F(48000.0)))
    assert p.release_rate == F(F(1.0) / F(F(1.0) * F(48000.0)))
    assert p.hold_samples == F(48000.0)
    q = M.Params(M.UNINITIALIZED_SAMPLE_RATE)
    assert q.decay_rate == F(F(1.0) / F(F(0.5) * F(66666.0)))
    z = M.Params(48000, attack_s=0.0, decay_s=0.0, release_s=0.0)
    assert z.attack_rate == z.decay_rate == z.release_rate == M.F32_MAX


def test_attack_reaches_target_at_the_frame_of_a_plain_f32_loop():
    """Zero scaling, with a hold: the attack ends after ceil(1 / attack_rate) frames up to the one-frame slack of f32 accumulation — and at
    exactly the frame a plain f32 accumulation loop gives."""
    for attack_s, sr in ((0.010, 48000), (0.0137, 44100), (0.25, 48000)):
        p = M.Params(sr, attack_s=attack_s)
        acc, k = F(0.0), 0
        while True:
            acc = F(acc + p.attack_rate)
            k += 1
            if acc >= F(1.0):
                break
        assert abs(k - math.ceil(1.0 / float(p.attack_rate))) <= 1
        env = M.Envelope()
        env.note_on(p, 1.0)
        outs = [env.run(p) for _ in range(k + 2)]
        assert env.stage == M.HOLD
        assert all(o < 1.0 for o in outs[:k - 1]) and outs[k - 1] == 1.0 and outs[k] == 1.0
        first_hold = next(i for i, o in enumerate(outs) if o == 1.0)
        assert first_hold == k - 1
        assert env.target_volume == p.sustain_level


def test_zero_attack_skips_to_hold_or_decay():
    env = M.Envelope()
    p = M.Params(48000, attack_s=0.0)
    env.note_on(p, 1.0)
    assert env.stage == M.HOLD and env.output == 1.0 and env.hold_samples_remaining == F(48000.0)
    p = M.Params(48000, attack_s=0.0, hold_s=0.0)
    env.note_on(p, 1.0)
    assert env.stage == M.DECAY and env.output == 1.0
    # ... and from there the decay runs from 1.0 to the sustain level in about decay_s * rate = 24000 frames: every f32 subtraction in
    # [0.5, 1) lands on a multiple of 2^-24, so the step of 1.0417e-5 (174.8 such units) is off by up to half a unit per frame, 0.29 %
    n = 0
    while env.stage == M.DECAY:
        env.run(p)
        n += 1
    slack = math.ceil(24000 * (0.5 * 2.0 ** -24) / float(p.decay_rate)) + 2
    assert env.stage == M.SUSTAIN and env.output == F(0.75) and abs(n - 24000) <= slack


def test_zero_release_goes_to_idle_with_output_zero():
    p, env = M.Params(48000, release_s=0.0), M.Envelope()
    env.note_on(p, 1.0)
    for _ in range(100):
        env.run(p)
    env.note_off(p)
    assert env.stage == M.IDLE and env.output == 0.0 and env.run(p) == 0.0


def test_release_from_a_level_ends_at_silence():
    p, env = M.Params(48000, attack_s=0.0, hold_s=0.0, decay_s=0.0, sustain_level=0.6, release_s=0.05), M.Envelope()
    env.note_on(p, 1.0)
    env.run(p)
    assert env.stage == M.SUSTAIN and env.output == F(0.6)
    env.note_off(p)
    assert env.stage == M.RELEASE and env.release_output == F(0.6)
    last = None
    n = 0
    while env.stage == M.RELEASE:
        last = env.output
        out = env.run(p)
        n += 1
    assert env.stage == M.IDLE and out == 0.0
    step = F(F(0.6) * p.release_rate)
    assert last > M.SILENCE and F(last - step) <= M.SILENCE   # the frame that crossed 0.001 is the one that ended it
    assert abs(n - 0.05 * 48000) <= 6                         # (0.6 - 0.001) / (0.6 / 2400) = 2396 frames


def test_note_off_at_zero_level_goes_straight_to_idle():
    p, env = M.Params(48000), M.Envelope()
    env.note_on(p, 1.0)
    env.note_off(p)   # output is still 0: nothing to release
    assert env.stage == M.IDLE


def test_render_is_independent_of_the_call_pieces():
    p = M.Params(8000, attack_s=0.01, hold_s=0.02, decay_s=0.05, release_s=0.05)
    n = 3000
    a, _, ia = M.render(p, n, note_off_at=777)
    b, _, _ = M.render(p, n, note_off_at=777, pieces=[128] * 23 + [56])
    assert np.array_equal(a, b)
    assert a[:80].max() < 1.0 and a[80] == 1.0 and a[-1] == 0.0
