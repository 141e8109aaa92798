"""tests/granular_model.py pinned against what the reference's code says (src/generator/sampler/granular.rs): the window tables' known
points, the crossfade points, the scheduler's first trigger and trigger spacing, Sequential's two-grain rule, pool exhaustion with the
draws of a failed activation, and independence of how a render is cut into calls. The reference's own tests cover none of this."""
import math

import numpy as np
import pytest

import granular_model as gm

F32 = np.float32


def test_lut_known_points():
    t = gm.lut()
    for w in (0, 2, 3, 4):   # Hann, Triangle, Tukey, Trapezoid peak at phase 0.5
        assert t[w, 1024] == F32(1.0), gm.WINDOWS[w]
    for w in (0, 2, 4, 6, 7):  # Hann, Triangle, Trapezoid, RampUp, RampDown start at 0
        assert t[w, 0] == F32(0.0), gm.WINDOWS[w]
    assert t[5, 0] == F32(math.exp(-3.0))                     # Exponential: exp(-6 * |0 - 0.5|)
    assert t[5, 1024] == F32(1.0)
    assert t[3, 512:1537].min() == F32(1.0) and t[4, 205:1844].min() == F32(1.0)   # Tukey's and Trapezoid's sustain
    assert abs(float(t[1, 1024]) - 1.0) < 1e-6 and abs(float(t[1, 0])) < 1e-6      # Blackman: 0.42 + 0.5 + 0.08, 0.42 - 0.5 + 0.08
    assert np.isfinite(t).all() and t.min() > -1e-6 and t.max() <= 1.0


def test_window_sample_branches():
    t = gm.lut()
    for w in range(8):
        assert gm.window_sample(w, 1.0) == t[w, gm.LUT_N - 1]              # index == N - 1: the last entry, no interpolation
        assert gm.window_sample(w, 0.0) == t[w, 0]
        x = 1000.25 / 2047.0
        idxf = x * 2047.0
        i, fr = int(idxf), F32(idxf - int(idxf))
        assert gm.window_sample(w, x) == F32(t[w, i] * (F32(1.0) - fr) + t[w, i + 1] * fr)


def test_crossfade_points():
    assert [float(gm.crossfade_point(w)) for w in range(8)] == [0.5, 0.5, 0.5, 0.5, float(F32(0.9)), float(F32(0.8)), float(F32(0.8)), float(F32(0.8))]


def test_rng_draws():
    r = gm.Xoshiro256pp([1, 2, 3, 4])
    # xoshiro256++ reference implementation, state {1, 2, 3, 4}: first outputs
    assert [r.next_u64() for _ in range(3)] == [41943041, 58720359, 3588806011781223]
    a, b = gm.Xoshiro256pp([5, 6, 7, 8]), gm.Xoshiro256pp([5, 6, 7, 8])
    u = b.next_u64()
    assert a.f32() == F32(u >> 40) * F32(2.0 ** -24)
    u = b.next_u64()
    assert a.f64() == (u >> 11) * 2.0 ** -53
    u = b.next_u64()
    assert a.boolean() == bool(u >> 63)
    assert gm.Xoshiro256pp(None).s == gm.Xoshiro256pp([0, 0, 0, 0]).s and any(gm.Xoshiro256pp(None).s)


def test_pow2_is_libms_on_these_draws():
    """The model's 2^x is the correctly rounded one; the libm of this machine agrees on the arguments the pitch variation produces."""
    r = gm.Xoshiro256pp([11, 12, 13, 14])
    for _ in range(300):
        x = (r.f64() - 0.5) / 12.0
        assert gm.pow2(x) == math.pow(2.0, x) or abs(gm.pow2(x) - math.pow(2.0, x)) <= 2.3e-16
    assert gm.pow2(0.0) == 1.0 and gm.pow2(1.0) == 2.0 and gm.pow2(-1.0) == 0.5


def test_defaults_at_44100():
    buf = gm.make_buffer(2048)
    m = gm.GrainPool(44100, buf, gm.Params())
    assert m.trigger_phase == F32(1.0)
    out, n, S = m.process(1)
    assert m.activations == [(0, 0)]                                        # trigger_phase starts at 1.0: the first frame triggers
    assert m.samples_remaining[0] == 4410 - 1 and m.window_increment[0] == 1.0 / 4410.0   # 100 ms at 44.1 kHz
    m.process(3 * 4410 + 10)
    frames = [f for f, _ in m.activations]
    assert len(frames) >= 3 and all(abs((b - a) - 4410) <= 1 for a, b in zip(frames, frames[1:]))
    assert m.playhead == F32(0.5) and not m.playing_loop_range            # step == 0: the playhead never moves
    assert m.increment[0] == 1.0 / 2048.0


def test_sequential_two_grains_and_crossfade_trigger():
    buf = gm.make_buffer(2048)
    for window in (0, 4):
        m = gm.GrainPool(8000, buf, gm.Params(overlap_mode=gm.SEQUENTIAL, window=window, size=50.0))
        cp = float(gm.crossfade_point(window))
        prev_primary, prev_phase = -1, 0.0
        for f in range(2500):
            phase_before = m.window_phase[m.primary] if m.primary >= 0 and m.active[m.primary] else None
            n_act = len(m.activations)
            m.process(1)
            assert int(m.active.sum()) <= 2
            if len(m.activations) > n_act and phase_before is not None:
                assert phase_before >= cp                                   # the new grain started at a frame whose primary phase had reached the point ...
                assert phase_before - 1.0 / 400.0 < cp                      # ... and at the FIRST such frame (400 samples per grain)
        assert len(m.activations) >= 5


def test_pool_exhaustion_and_the_draws_of_a_failed_activation():
    """Density 100 at 8000 Hz is a trigger every ~80 frames; 1000 ms grains whose size varies up to x 3 outlive 100 triggers: the pool fills."""
    buf = gm.make_buffer(2048)
    m = gm.GrainPool(8000, buf, gm.Params(density=100.0, size=1000.0, variation=1.0), [9, 8, 7, 6])
    before, acts = None, 0
    while m.failed_activations == 0:
        assert m.frame < 16000
        before, acts = list(m.rng.s), len(m.activations)
        m.process(1)
    assert m.active.all() and len(m.activations) == acts >= 100             # 100 concurrent grains, and activate_new_grain returned None
    probe = gm.Xoshiro256pp(before)
    probe.f64()                                                             # the spray draw happens (:562-571 precedes :821), the others do not
    assert list(m.rng.s) == probe.s
    while m.active.all():                                                   # ... until a slot frees: no activation, one draw per trigger
        fails, before = m.failed_activations, list(m.rng.s)
        m.process(1)
        assert len(m.activations) == acts
        if m.failed_activations > fails:
            probe = gm.Xoshiro256pp(before)
            probe.f64()
            assert list(m.rng.s) == probe.s
        else:
            assert list(m.rng.s) == before
    while len(m.activations) == acts:
        free = int(np.flatnonzero(~m.active)[0])
        m.process(1)
    assert m.activations[-1][1] == free                                     # the first inactive slot takes the next trigger


CLOUD = dict(density=100.0, size=1000.0, variation=1.0, spray=1.0, pan_spread=1.0, playback_direction=gm.RANDOM, step=1.0)


@pytest.mark.parametrize("kw,frames", [(dict(), 2048), (CLOUD, 3072), (dict(overlap_mode=gm.SEQUENTIAL, window=0, size=20.0, variation=0.5), 2048),
                                       (dict(loop_range=(0.25, 0.75), step=2.0, position=0.1, density=50.0, size=40.0), 2048)], ids=["defaults", "cloud", "sequential", "loop"])
def test_call_cutting_changes_no_state(kw, frames):
    buf = gm.make_buffer(2048)
    ref = gm.GrainPool(8000, buf, gm.Params(**kw), [1, 2, 3, 4])
    out, n, S = ref.process(frames)
    bound = 2.0 * n[:, None] * 2.0 ** -23 * S
    for cut in (1, 7, 64, 1024):
        m = gm.GrainPool(8000, buf, gm.Params(**kw), [1, 2, 3, 4])
        parts = [m.process(min(cut, frames - a))[0] for a in range(0, frames, cut)]
        assert gm.states_equal(ref.state(), m.state()) == []
        o = np.concatenate(parts)
        assert (np.abs(o.astype(np.float64) - out.astype(np.float64)) <= bound).all()


def test_commands_reach_new_grains_only():
    buf = gm.make_buffer(2048)
    m = gm.GrainPool(8000, buf, gm.Params(density=50.0, size=100.0))
    m.process(100)
    old = m.volume_g[0], m.panning_g[0], m.increment[0]
    m.set_volume(0.25), m.set_panning(-0.5), m.set_speed(2.0)
    m.process(161 - 100)
    assert (m.volume_g[0], m.panning_g[0], m.increment[0]) == old            # the running grain keeps its values
    assert (m.volume_g[1], m.panning_g[1], m.increment[1]) == (F32(0.25), F32(-0.5), 2.0 / 2048.0)
    m.stop()
    assert not m.is_exhausted()
    m.process(800)
    assert m.is_exhausted() and len(m.activations) == 2
