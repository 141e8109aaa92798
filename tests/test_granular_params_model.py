"""tests/granular_params_model.py on the CPU: with no command it is the grain pool the other models are; each thing a parameter change makes live
shows in it (the activation spacing, the cleared primary, a position that moves nothing while the playhead runs); the descriptor table is
Sampler::granular_parameters() (reference src/generator/sampler.rs:219-296, hand-copied into tests/golden/granular_params.json) and the
normalized mappings are the formulas of src/parameter/float.rs:137-141 and src/parameter/enum.rs:154."""
import json
import math
import os

import numpy as np
import pytest

import granular_model as gm
import granular_params_model as gpm
import modulation_model as mm

F32 = np.float32
SR = 8000
RNG = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "granular_params.json")
BASE = dict(density=50.0, size=60.0, variation=0.3, spray=0.3, pan_spread=0.3, step=1.0, position=0.2, playback_direction=gm.RANDOM, loop_range=(0.25, 0.75))


def _pool(cls, kw, **extra):
    return cls(SR, gm.make_buffer(2048), gm.Params(**kw), rng_state=RNG, **extra)


@pytest.mark.parametrize("overlap", [gm.CLOUD, gm.SEQUENTIAL], ids=["cloud", "sequential"])
def test_without_commands_it_is_the_grain_pool(overlap):
    kw = dict(BASE, overlap_mode=overlap)
    plain, mod, par = _pool(gm.GrainPool, kw), _pool(mm.ModGrainPool, kw, matrix=mm.Matrix(SR)), _pool(gpm.ParamGrainPool, kw)
    for n in (1, 31, 700, 1316):
        a, b, c = plain.process(n), mod.process(n), par.process(n)
        for x, y, z in zip(a, b, c):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        st = par.state()
        assert st.pop("overlap_mode") == overlap
        assert gm.states_equal(plain.state(), st) == [] and gm.states_equal(mod.state(), st) == []
    assert len(par.activations) >= 5 and par.activations == plain.activations
    assert par.cleared_primaries == 0 and (overlap == gm.CLOUD or par.blocked_frames > 0)


def test_overlap_mode_is_cloud_until_the_first_frame():
    par = _pool(gpm.ParamGrainPool, dict(BASE, overlap_mode=gm.SEQUENTIAL))
    assert par.state()["overlap_mode"] == gm.CLOUD
    par.process(1)
    assert par.state()["overlap_mode"] == gm.SEQUENTIAL and par.primary == 0


def test_density_change_moves_the_activation_spacing():
    """No variation: the trigger phase is the only clock. sr / d frames between two activations, give or take the f32 phase's rounding."""
    d1, d2 = 50.0, 20.0
    par = _pool(gpm.ParamGrainPool, dict(density=d1, size=20.0))
    par.process(1000)
    par.set_parameter("GDEN", d2)
    par.process(3000)
    frames = np.array([f for f, _ in par.activations])
    before, after = np.diff(frames[frames < 1000]), np.diff(frames[frames >= 1000 + SR / d2])
    assert len(before) >= 5 and len(after) >= 5
    assert np.all(np.abs(before - SR / d1) <= 1) and np.all(np.abs(after - SR / d2) <= 1)


def test_mode_change_clears_an_active_primary():
    par = _pool(gpm.ParamGrainPool, dict(overlap_mode=gm.SEQUENTIAL, size=100.0, window=0))
    par.process(300)
    assert par.primary >= 0 and par.active[par.primary] and par.cleared_primaries == 0
    par.set_parameter("GOVM", gm.CLOUD)
    assert par.primary >= 0                      # the parameters changed; the pool follows at its next frame
    par.process(1)
    assert par.primary == -1 and par.cleared_primaries == 1 and par.state()["overlap_mode"] == gm.CLOUD
    par.set_parameter("GOVM", 1.0, normalized=True)
    par.process(300)
    assert par.primary >= 0 and par.state()["overlap_mode"] == gm.SEQUENTIAL


def test_position_moves_nothing_while_the_playhead_runs():
    kw = dict(density=50.0, size=20.0, step=1.0, position=0.2)
    a, b = _pool(gpm.ParamGrainPool, kw), _pool(gpm.ParamGrainPool, kw)
    a.process(500), b.process(500)
    b.set_parameter("GPOS", 0.9)
    oa, ob = a.process(1500), b.process(1500)
    assert oa[0].tobytes() == ob[0].tobytes() and gm.states_equal(a.state(), b.state()) == [] and b.params_state()["position"] == F32(0.9)
    a.set_parameter("GSTP", 0.0), b.set_parameter("GSTP", 0.0)        # step 0: the position counts again, the playhead keeps its value
    ph = b.playhead
    oa, ob = a.process(500), b.process(500)
    assert oa[0].tobytes() != ob[0].tobytes() and b.playhead == ph == a.playhead


def test_position_in_front_of_the_note_is_the_playheads():
    par = _pool(gpm.ParamGrainPool, dict(step=1.0, position=0.2))
    par.set_parameter("GPOS", 0.6, started=False)
    assert par.playhead == F32(0.6)
    par.set_parameter("GPOS", 0.1)
    assert par.playhead == F32(0.6)


def test_a_grain_keeps_its_window_and_loop_range():
    par = _pool(gpm.ParamGrainPool, dict(BASE, density=100.0, size=100.0, variation=0.0))
    par.process(1200)
    assert par.playing_loop_range and par.has_loop[par.active].any()
    par.set_parameter("GWND", 4), par.set_loop_range(None)
    still = par.active & (par.samples_remaining > 100)     # (a slot that runs out inside the 100 frames may be taken again)
    par.process(100)
    assert still.any() and np.all(par.window_mode[still] == 2) and par.has_loop[still].any()
    new = par.active & ~still
    assert new.any() and np.all(par.window_mode[new] == 4) and not par.has_loop[new].any() and par.playing_loop_range
    assert len(par.windows_above_threshold()) == 2


def test_descriptors_equal_the_fixture():
    golden = json.load(open(GOLDEN))
    assert [g["id"] for g in golden] == gpm.IDS == ["GOVM", "GWND", "GSIZ", "GDEN", "GVAR", "GSPY", "GPAN", "GDIR", "GPOS", "GSTP"]
    for g, d in zip(golden, gpm.DESCRIPTORS):
        assert (g["id"], g["name"], g["type"]) == d[:3]
        if g["type"] == "enum":
            assert (len(g["values"]), g["default"]) == d[3:]
        else:
            assert (g["min"], g["max"], g["default"], g["scaling"], g.get("factor")) == d[3:]


def test_normalized_mappings():
    r = gpm.resolve
    assert r("GSIZ", 0.5, True) == F32(F32(1.0) + F32(F32(0.25) * F32(999.0)))
    assert r("GDEN", 0.5, True) == F32(F32(1.0) + F32(F32(0.25) * F32(99.0)))
    assert r("GSIZ", 0.0, True) == F32(1.0) and r("GSIZ", 1.0, True) == F32(1000.0) and r("GSIZ", 7.0, True) == F32(1000.0) and r("GDEN", -1.0, True) == F32(1.0)
    assert r("GSTP", 0.75, True) == F32(2.0) and r("GPOS", 0.3, True) == F32(0.3) and r("GVAR", 2.0, True) == F32(1.0)
    assert r("GWND", 0.5, True) == 4 and math.floor(3.5 + 0.5) == 4                 # round(3.5): halves away from zero
    assert r("GWND", 0.0, True) == 0 and r("GWND", 1.0, True) == 7 and r("GOVM", 0.5, True) == 1 and r("GOVM", 0.49, True) == 0
    assert r("GDIR", 0.25, True) == 1 and r("GDIR", 0.24, True) == 0 and r("GDIR", 0.8, True) == 2
    # raw: clamped floats, enum indices (out of range: ignored)
    assert r("GSIZ", 5000.0, False) == F32(1000.0) and r("GSIZ", 0.0, False) == F32(1.0) and r("GSTP", -9.0, False) == F32(-4.0) and r("GSPY", 0.37, False) == F32(0.37)
    assert r("GWND", 7.0, False) == 7 and r("GWND", 8.0, False) is None and r("GOVM", -1.0, False) is None and r("GDIR", 2.9, False) == 2
    with pytest.raises(ValueError):
        r("GXYZ", 0.5, False)
    with pytest.raises(ValueError):
        r("GSIZ", math.nan, True)
