"""tests/modulation_model.py pinned without a device: the LFO shapes against values written out by hand, sine_approx at its fixed points, the four
polarity transforms and the 0.001 routing threshold of src/modulation/matrix.rs, the redraws of the random shapes on the f32 phase wraps, and the
modulated grain pool against tests/granular_model.py where the two must agree."""
import numpy as np
import pytest

import granular_model as gm
import modulation_model as mm

F32 = np.float32
SR = 8000
RNG = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444)
LFO_RNG = ((0xA5A5A5A5DEADBEEF, 2, 3, 4), (5, 6, 0xC0FFEE1234567890, 8))
CLOUD = dict(density=100.0, size=1000.0, variation=1.0, spray=1.0, pan_spread=1.0, playback_direction=gm.RANDOM, step=1.0)
# the parameters of tests/test_gpu_modulation.py's single-route and all-routes cases
BASE = dict(density=50.0, size=60.0, variation=0.3, spray=0.3, pan_spread=0.3, step=1.0, position=0.2, playback_direction=gm.RANDOM)
LOOPED = dict(BASE, loop_range=(0.25, 0.75))


def bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32).tolist()


@pytest.mark.parametrize("waveform,want", [
    (mm.TRIANGLE, [0.0, 0.5, 1.0, 0.5, 0.0, -0.5, -1.0, -0.5, 0.0, 0.5]),
    (mm.RAMP_UP, [-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, -1.0, -0.75]),
    (mm.RAMP_DOWN, [1.0, 0.75, 0.5, 0.25, 0.0, -0.25, -0.5, -0.75, 1.0, 0.75]),
    (mm.SQUARE, [1.0, 1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0, 1.0, 1.0]),
], ids=["Triangle", "RampUp", "RampDown", "Square"])
def test_shapes_at_an_eighth_of_the_rate(waveform, want):
    """rate = sr / 8: phase_inc = 0.125 exactly, the phases are 0, 1/8 .. 7/8, 0, 1/8 and every value is exact in f32."""
    l = mm.Lfo(SR, SR / 8, waveform, RNG)
    assert l.phase_inc == F32(0.125)
    got = [l.run() for _ in range(10)]
    assert bits(got) == bits(want)


def test_sine_approx_fixed_points():
    """B x + C x |x| is 0 at 0 and +-pi and +-1 at +-pi/2, where the correction term P (y |y| - y) vanishes: within two roundings of f32."""
    assert mm.sine_approx(0.0) == 0.0
    for x, want in ((mm.FRAC_PI_2, 1.0), (-mm.FRAC_PI_2, -1.0), (mm.PI, 0.0), (-mm.PI, 0.0)):
        assert abs(float(mm.sine_approx(x)) - want) <= 2.0 ** -22, (x, mm.sine_approx(x))
    assert bits(mm.sine_approx(F32(0.7))) == bits(-mm.sine_approx(F32(-0.7)))
    l = mm.Lfo(SR, SR / 8, mm.SINE, RNG)       # phases 0, 1/8, 1/4: sin(0), ~sin(pi/4), sin(pi/2)
    v = [float(l.run()) for _ in range(3)]
    assert v[0] == 0.0 and abs(v[1] - 2.0 ** -0.5) < 1.1e-3 and abs(v[2] - 1.0) <= 2.0 ** -22


def test_polarity_transforms():
    for v in (0.0, 0.25, 1.0):       # unipolar sources: velocity, keytracking
        assert mm.unipolar_source(F32(v), False) == F32(v)
        assert mm.unipolar_source(F32(v), True) == F32((v - 0.5) * 2.0)
    for v in (-1.0, 0.0, 1.0):       # bipolar sources: the LFOs
        assert mm.bipolar_source(F32(v), True) == F32(v)
        assert mm.bipolar_source(F32(v), False) == F32((v + 1.0) / 2.0)
    # ... and where they enter the sum: slot order, `+= mod_value * amount`
    mx = mm.make_matrix(SR, rates=(20.0, 20.0), waveforms=(mm.SQUARE, mm.RAMP_UP), velocity=0.25, note=127,
                        routes=[(mm.LFO1, mm.SIZE, 0.5, True), (mm.LFO2, mm.SIZE, 0.25, False), (mm.VELOCITY, mm.SIZE, -1.0, True), (mm.KEYTRACK, mm.SIZE, 0.125, False),
                                (mm.KEYTRACK, mm.STEP, 1.0, True)])
    out = mx.process_frame()
    assert out[mm.SIZE] == F32(1.0 * 0.5 + ((-1.0 + 1.0) / 2.0) * 0.25 + ((0.25 - 0.5) * 2.0) * -1.0 + 1.0 * 0.125) and out[mm.STEP] == F32(1.0)
    assert (out[[mm.DENSITY, mm.VARIATION, mm.SPRAY, mm.PAN_SPREAD, mm.POSITION]] == 0).all() and np.array_equal(mx.last, out)


def test_routing_threshold():
    mx = mm.Matrix(SR)
    mx.set_modulation(mm.LFO1, mm.DENSITY, 0.0009, True)
    assert not mx.has_route(mm.LFO1, mm.DENSITY)                      # not added
    mx.set_modulation(mm.LFO1, mm.DENSITY, 0.001, True)
    assert mx.has_route(mm.LFO1, mm.DENSITY) and mx.bipolar[mm.LFO1, mm.DENSITY] == 1
    mx.set_modulation(mm.LFO1, mm.DENSITY, -0.5, False)               # one route per slot and target: updated in place
    assert mx.amount[mm.LFO1, mm.DENSITY] == F32(-0.5) and mx.bipolar[mm.LFO1, mm.DENSITY] == 0
    mx.set_modulation(mm.LFO1, mm.DENSITY, -0.0009, True)
    assert not mx.has_route(mm.LFO1, mm.DENSITY) and mx.bipolar[mm.LFO1, mm.DENSITY] == 0   # removed
    mx.set_modulation(mm.VELOCITY, mm.STEP, 1.0, False)
    mx.clear_modulation(mm.VELOCITY, mm.STEP)
    assert not mx.amount.any()
    for bad in (1.5, -1.001, float("nan")):
        with pytest.raises(ValueError):
            mx.set_modulation(mm.LFO1, mm.SIZE, bad, True)
    with pytest.raises(ValueError):
        mx.set_modulation(4, mm.SIZE, 0.5, True)
    with pytest.raises(ValueError):
        mx.set_modulation(mm.LFO1, 7, 0.5, True)


@pytest.mark.parametrize("waveform", [mm.RANDOM, mm.SMOOTH_RANDOM], ids=["Random", "SmoothRandom"])
def test_random_shapes_redraw_exactly_on_the_wraps(waveform):
    l = mm.Lfo(SR, 1.0, mm.SINE, LFO_RNG[0])
    assert l.draws == 3
    l.set_rate(19.7)
    l.set_waveform(waveform)
    assert l.draws == 3                                    # set_waveform / set_rate draw nothing
    l.reset()
    assert l.draws == 5 and l.phase == 0
    inc, ph, wraps = F32(19.7 / SR), F32(0.0), []
    for f in range(2000):                                  # the f32 recurrence on its own
        ph = F32(ph + inc)
        if ph >= F32(1.0):
            ph = F32(ph - F32(1.0))
            wraps.append(f)
    got, values = [], []
    for f in range(2000):
        before = l.draws
        held = (l.sample_hold, l.jitter_current, l.jitter_target)
        values.append(l.run())
        if l.draws != before:
            assert l.draws == before + 2 and l.jitter_current == held[2]
            got.append(f)
        else:
            assert (l.sample_hold, l.jitter_current, l.jitter_target) == held
    assert got == wraps and len(wraps) == 4 and l.phase == ph
    if waveform == mm.RANDOM:
        assert len(set(bits(values))) == 5                 # one held value per period
    else:
        assert len(set(bits(values))) > 1500 and max(abs(float(v)) for v in values) <= 1.0


def test_a_deterministic_shape_never_draws():
    l = mm.Lfo(SR, 20.0, mm.TRIANGLE, LFO_RNG[1])
    l.reset()
    for _ in range(1000):
        l.run()
    assert l.draws == 3


def test_matrix_without_routes_is_the_plain_pool():
    """`x + 0.0` and `x * (1.0 + 0.0)`: bit for bit tests/granular_model.py over 4096 frames of the cloud that fills the pool."""
    buf = gm.make_buffer(2048)
    a = gm.GrainPool(SR, buf, gm.Params(**CLOUD), RNG)
    b = mm.ModGrainPool(SR, buf, gm.Params(**CLOUD), mm.make_matrix(SR, rng_states=LFO_RNG), RNG)
    oa, ca, sa = a.process(4096)
    ob, cb, sb = b.process(4096)
    assert gm.states_equal(a.state(), b.state()) == [] and np.array_equal(oa.view(np.uint32), ob.view(np.uint32)) and np.array_equal(ca, cb)
    assert ca.max() >= 40 and not b.matrix.last.any() and b.matrix.lfos[0].phase != 0


ALL_ROUTES = [(s, t, [1.0, -1.0, 0.37][(s + t) % 3], (s * 7 + t) % 2 == 0) for s in range(4) for t in range(7)]


def _pool(kw, zero=(), **mkw):
    mkw.setdefault("rates", (20.0, 13.0))
    mkw.setdefault("velocity", 0.8)
    mkw.setdefault("note", 72)
    return mm.ModGrainPool(SR, gm.make_buffer(2048), gm.Params(**kw), mm.make_matrix(SR, rng_states=LFO_RNG, **mkw), RNG, zero=zero)


def test_cutting_a_render_changes_nothing():
    a = _pool(LOOPED, routes=ALL_ROUTES, waveforms=(mm.SMOOTH_RANDOM, mm.SINE))
    b = _pool(LOOPED, routes=ALL_ROUTES, waveforms=(mm.SMOOTH_RANDOM, mm.SINE))
    oa, _, _ = a.process(1500)
    ob = np.concatenate([b.process(n)[0] for n in (1, 31, 32, 33, 64, 700, 639)])
    assert gm.states_equal(a.state(), b.state()) == [] and gm.states_equal(a.matrix.state(), b.matrix.state()) == []
    assert np.array_equal(oa.view(np.uint32), ob.view(np.uint32)) and a.playing_loop_range


@pytest.mark.parametrize("target", range(mm.N_TARGETS), ids=["size", "density", "variation", "spray", "pan_spread", "position", "step"])
def test_every_input_shows_in_the_state(target):
    """What tests/test_gpu_modulation.py relies on: with its parameters, amounts and lengths, a pool that is fed 0.0 for ONE target ends in another
    state than the full model - for every source routed alone to that target in either polarity, and with all 28 routes at once."""
    configs = [[(s, target, [1.0, -1.0, 0.37][(s + target + b) % 3], bool(b))] for s in range(4) for b in (0, 1)] + [ALL_ROUTES]
    for routes in configs:
        kw = BASE if len(routes) == 1 else LOOPED
        full, cut = _pool(kw, routes=routes, rates=(20.0, 20.0)), _pool(kw, zero=(target,), routes=routes, rates=(20.0, 20.0))
        full.process(2048), cut.process(2048)
        assert gm.states_equal(full.state(), cut.state()) != [], routes
