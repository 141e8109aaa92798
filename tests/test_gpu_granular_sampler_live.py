"""Granular-mode samplers on the device taking the messages that change EVERY voice while notes sound — envelope parameters, routes, LFO rate and
waveform, the loop range (pg_gsampler_kernel's gs_open) — against the independent model tests/sampler_live_model.py. Everything goes through
the C ABI.

The shapes and the bars are tests/test_gpu_granular_sampler.py's: 48 kHz, the 3000-frame mono buffer, max_frames 256, writes of 300, 20, 4300, 1
and 499 frames; after EVERY write (tests/granular_sampler_rig.py: run, tests/sampler_live_rig.py: GRig) the slot table, every slot's grain state
and matrix state, the parameters and — new — the envelope parameters read back on every slot equal the model's field by field, and the audio
equals the model's as values. Every case asserts on the model that what it is about happened."""
import numpy as np
import pytest

import ahdsr_model as A
import granular_sampler_rig as R
import modulation_model as mm
import sampler_live_rig as LR
from phonic_amd import _capi
from phonic_amd.graph import Graph

pytestmark = pytest.mark.gpu

SR, MF = R.SR, R.MF
SIZES = LR.SIZES
MOD = dict(rates=(7.0, 13.0), waveforms=(mm.SINE, mm.RANDOM), rng_states=R.LFO_RNG,
           routes=[(mm.LFO1, mm.SIZE, 0.5, True), (mm.LFO2, mm.POSITION, 0.3, False), (mm.VELOCITY, mm.DENSITY, -0.4, False)])
KW = dict(R.SHORT, size=6.0)


def _single(voice_count, **kw):
    g = Graph(SR, 2, MF, 0)
    mixer = g.add_mixer()
    g.add_effect(mixer, _capi.FX_GAIN)   # unity: it changes no sample
    return g, LR.GRig(g, mixer, [0], voice_count, **kw)


def _peak(audio):
    return float(np.abs(audio).max())


# ---- 1: every envelope parameter, found by notes in every stage ----
# R.ENV: attack 96, hold 144, decay 192 frames, release 240. A starts at 10 (Attack to 106, Hold to 250, Decay to 442), B at 150 (Hold 246..390),
# C at 330 (Attack to 426). Frame 350 finds C in Attack, B in Hold, A in Decay; A's note-off is at 760 (Sustain); frame 800 finds A in Release
# and B in Sustain, whatever the message at 350 did to the decay.
ENV_VALUES = {"AATK": (0.004, 0.0), "AHLD": (0.001, 0.0), "ADCY": (0.001, 0.0), "ASTN": (0.3, 0.9), "AREL": (0.002, 0.0)}


@pytest.mark.parametrize("fourcc", LR.ENV_IDS)
def test_envelope_parameter_in_every_stage(fourcc):
    g, r = _single(3, envelope=R.ENV, kw=KW)
    a = r.on(10, 60)
    r.on(150, 64, 0.8, 0.3)
    r.on(330, 67, 0.9, -0.2)
    first, second = ENV_VALUES[fourcc]
    r.env(350, fourcc, first)
    r.off(760, a)
    r.env(800, fourcc, second)
    d = r.on(1500, 70)                       # a later note starts under the parameters as they are now
    r.env(4416, fourcc, 0.5, True)           # normalized, on a chunk edge inside the third write
    r.off(4700, d)
    got, exp = R.run(g, [r], SIZES)
    stages = {t: s for t, _, s in r.m.env_log}
    assert sorted(stages[350]) == [A.ATTACK, A.HOLD, A.DECAY] and A.RELEASE in stages[800] and A.SUSTAIN in stages[800]
    assert len(r.m.env_log) == 3 and _peak(exp[0]) > 0.02


def test_sustain_and_decay_out_of_time_order_and_on_one_frame():
    """ADCY sent first but due behind ASTN divides by the new sustain; the two on ONE frame apply in sending order: ADCY, then ASTN leaves the rate stale."""
    g, r = _single(2, envelope=R.ENV, kw=KW)
    r.on(10, 60)
    r.env(300, "ADCY", 0.006)
    r.env(200, "ASTN", 0.2)
    r.on(400, 64)
    r.env(900, "ADCY", 0.002)                # one frame, ADCY first: (1 - 0.2) / ...
    r.env(900, "ASTN", 0.8)                  # ... and the sustain moves under it
    got, exp = R.run(g, [r], [300, 20, 700])
    st = r.m.envelope_state()
    assert st["sustain_level"] == np.float32(0.8) and st["decay_rate"] == np.float32(np.float32(np.float32(1.0) - np.float32(0.2)) / np.float32(np.float32(0.002) * np.float32(SR)))
    assert _peak(exp[0]) > 0.02


# ---- 2: the matrix: routes, LFO rate and waveform — 2 slots sounding, 1 free, then a note into the free slot ----
def test_routes_and_lfos_inside_pieces_and_on_edges():
    """Writes begin at 0, 300, 320, 4620, 4621; the third one's second chunk at 4416; pieces of 256 frames from each chunk's start."""
    g, r = _single(3, modulation=MOD, kw=KW)
    a = r.on(10, 60, 0.7, 0.0)
    b = r.on(40, 72, 1.0, 0.2)
    r.route(100, mm.VELOCITY, mm.POSITION, 0.3, False)         # set, inside a piece
    r.route(320, mm.VELOCITY, mm.POSITION, -0.6, False)        # changed, on a write's edge
    r.route(576, mm.VELOCITY, mm.POSITION, -0.6, True)         # made bipolar, on a piece edge
    r.lfo_waveform(640, 0, mm.SQUARE)
    r.unroute(700, mm.VELOCITY, mm.POSITION)                   # cleared
    r.lfo_rate(900, 1, 19.0)
    r.route(4416, mm.KEYTRACK, mm.SPRAY, 0.6, True)            # on a chunk edge inside a write
    r.lfo_rate(4416, 0, 0.001)                                 # clamped to 0.01 Hz
    r.lfo_waveform(4416, 1, mm.SMOOTH_RANDOM)
    c = r.on(4500, 50, 0.4, 0.0)                               # into the free slot: it sounds under what the messages left in its matrix
    r.route(4620, mm.LFO1, mm.SIZE, 0.0005, True)              # below the threshold: the route creation gave goes
    r.all_off(4900)
    got, exp = R.run(g, [r], SIZES)
    assert r.slot_of(a) == 0 and r.slot_of(b) == 1 and r.slot_of(c) == 2
    log = r.m.live_log
    assert all(active == 2 and free == (2,) for now, _, active, _, free in log if now < 4500) and len(log) == 10
    ms = r.m.modulation_state(2)
    assert ms["amount"][mm.KEYTRACK, mm.SPRAY] == np.float32(0.6) and ms["amount"][mm.LFO1, mm.SIZE] == 0 and ms["lfo0_waveform"] == mm.SQUARE
    assert ms["lfo0_phase_inc"] == np.float32(float(np.float32(0.01)) / SR) and ms["velocity"] == np.float32(0.4)
    assert _peak(exp[0]) > 0.02


def test_route_and_lfo_on_one_frame_in_both_orders():
    outs = []
    for order in (0, 1):
        g, r = _single(2, modulation=MOD, envelope=R.ENV, kw=KW)
        r.on(10, 60)
        calls = [lambda: r.route(200, mm.LFO1, mm.POSITION, 0.5, True), lambda: r.lfo_rate(200, 0, 15.0), lambda: r.env(200, "ASTN", 0.3), lambda: r.loop(200, (500, 2500))]
        for c in (calls if order == 0 else calls[::-1]):
            c()
        got, exp = R.run(g, [r], [300, 20, 500])
        outs.append(got)
        assert [k for _, k, _, _, _ in r.m.live_log] == (["route", "lfo", "loop"] if order == 0 else ["loop", "lfo", "route"])
    assert np.array_equal(outs[0], outs[1]) and _peak(outs[0]) > 0.02      # four different fields: the order does not show


# ---- 3: the loop range while a cloud plays ----
def test_loop_range_set_changed_and_removed_while_grains_live():
    g, r = _single(2, kw=dict(KW, step=1.0, position=0.1), loop_range=(0.05, 0.9))
    r.on(10, 60)
    r.on(30, 67, 0.8, -0.5)
    r.loop(100, (300, 1500))                 # set, inside a piece
    r.loop(320, (1000, 1200))                # changed, on a write's edge
    r.loop(2000, None)                       # removed: no loop at all
    r.loop(4416, (0, 3000))                  # the whole buffer, on a chunk edge
    r.on(4500, 72)
    r.all_off(4800)
    got, exp = R.run(g, [r], SIZES)
    assert [now for now, *_ in r.m.live_log] == [100, 320, 2000, 4416] and all(living >= 1 for _, _, _, living, _ in r.m.live_log)
    ps = r.m.params_state()
    assert ps["has_loop_range"] == 1 and ps["loop_start"] == 0 and ps["loop_end"] == np.float32(1.0) and _peak(exp[0]) > 0.02


# ---- 4: in front of the start time; while stopping ----
def test_messages_stamped_before_the_start_time_act_at_it():
    g, r = _single(2, envelope=R.ENV, modulation=MOD, kw=KW, start_time=64)
    r.env(20, "ADCY", 0.002)                 # stamped later than the ASTN below: it sees sustain 0.3
    r.env(5, "ASTN", 0.3)
    r.route(6, mm.VELOCITY, mm.SIZE, 0.5, False)
    r.lfo_rate(7, 1, 3.0)
    r.loop(8, (100, 2000))
    r.on(64, 60, 0.8, 0.0)
    r.env(500, "AREL", 0.001)
    r.all_off(600)
    got, exp = R.run(g, [r], [300, 20, 700])
    assert [t for t, _, _ in r.m.env_log] == [64, 64, 500] and [now for now, *_ in r.m.live_log] == [64, 64, 64]
    assert r.m.envelope_state()["decay_rate"] == np.float32(np.float32(np.float32(1.0) - np.float32(0.3)) / np.float32(np.float32(0.002) * np.float32(SR)))
    assert not got[:64].any() and _peak(exp[0]) > 0.02


def test_messages_while_stopping_are_dropped():
    g, r = _single(2, envelope=R.ENV, modulation=MOD, kw=KW, transient=True)
    r.on(10, 60)
    r.on(40, 64)
    r.stop(200)
    r.env(230, "ASTN", 0.1)
    r.env(231, "AREL", 0.0)
    r.route(232, mm.LFO1, mm.SIZE, -1.0, False)
    r.lfo_rate(233, 0, 1.0)
    r.lfo_waveform(234, 1, mm.SINE)
    r.loop(235, (10, 20))
    got, exp = R.run(g, [r], [300, 20, 1000])
    st = r.m.state()
    assert st["stopping"] and st["stopped"] and not r.m.env_log and r.m.live_log == []
    assert r.m.envelope_state()["sustain_level"] == np.float32(0.6) and _peak(exp[0]) > 0.02


# ---- 5: seeded random scripts (tests/test_sampler_live_model.py asserts their conditions on the model alone) ----
@pytest.mark.parametrize("n_slots,seed", LR.SCRIPT_CASES)
def test_seeded_random_scripts(n_slots, seed):
    g, r = _single(n_slots, envelope=LR.SCRIPT_ENV, modulation=LR.SCRIPT_MOD)
    LR.random_script(r, LR.script_rng(n_slots, seed), n_slots)
    got, exp = R.run(g, [r], LR.SCRIPT_SIZES)
    cond = LR.script_conditions(r.m)
    assert all(cond.values()), cond
    assert _peak(exp[0]) > 0.02
