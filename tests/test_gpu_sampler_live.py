"""File samplers on the device taking AMP_* envelope parameters while notes sound (pg_unit_kernel's sampler_command), against
tests/sampler_live_model.py through tests/sampler_rig.py's audio path: every note rendered as an ordinary voice of the CPU oracle, times the
model's envelope gains, summed in slot order. The bar is the rig's: alone in its mixer the sampler's audio is bit for bit the expected one;
after every write the slot table and — on every slot, playing or free — the envelope parameters read back equal the model's.

48 kHz, the 3000-frame mono buffer of the granular rigs, max_frames 256, writes of 300, 20, 4300, 1 and 499 frames, an envelope of
milliseconds (attack 96, hold 144, decay 192, release 240 frames) so that every stage lies inside them."""
import numpy as np
import pytest

import ahdsr_model as A
import granular_sampler_rig as GR
import sampler_live_rig as LR
import sampler_rig as FR
from phonic_amd import _capi
from phonic_amd.graph import Graph

pytestmark = pytest.mark.gpu

SR, MF = FR.SR, 256
PCM = GR.BUF                 # 3000 frames, mono
ENV = GR.ENV
SIZES = LR.SIZES


def _single(voice_count, envelope=ENV, **kw):
    g = Graph(SR, 2, MF, 0)
    mixer = g.add_mixer()
    g.add_effect(mixer, _capi.FX_GAIN)   # unity: it changes no sample
    return g, LR.FRig(g, mixer, PCM, [0], voice_count, envelope=envelope, channels=1, rate=SR, **kw)


def _check_audio(got, r, n):
    FR._assert_equal(got, r.expected(n))


# A starts at 10 (Attack to 106, Hold to 250, Decay to 442), B at 150 (Hold 246..390), C at 330 (Attack to 426): frame 350 finds C in Attack, B in
# Hold, A in Decay; A's note-off is at 760 (Sustain); frame 800 finds A in Release and B in Sustain, whatever the message at 350 did to the decay.
ENV_VALUES = {"AATK": (0.004, 0.0), "AHLD": (0.001, 0.0), "ADCY": (0.001, 0.0), "ASTN": (0.3, 0.9), "AREL": (0.002, 0.0)}


@pytest.mark.parametrize("fourcc", LR.ENV_IDS)
def test_envelope_parameter_in_every_stage(fourcc):
    g, r = _single(3)
    a = r.on(10, 60)
    r.on(150, 57, 0.8, 0.3)
    r.on(330, 55, 0.9, -0.2)
    first, second = ENV_VALUES[fourcc]
    r.env(350, fourcc, first)
    r.off(760, a)
    r.env(800, fourcc, second)
    d = r.on(1500, 53)                       # a later note starts under the parameters as they are now
    r.env(1856, fourcc, 0.5, True)           # normalized, on a piece edge of the third write (320 + 6 * 256)
    r.off(2400, d)
    got = FR._run(g, [r], SIZES)
    stages = {t: s for t, _, s in r.m.env_log}
    assert sorted(stages[350]) == [A.ATTACK, A.HOLD, A.DECAY] and A.RELEASE in stages[800] and A.SUSTAIN in stages[800]
    assert len(r.m.env_log) == 3
    _check_audio(got, r, sum(SIZES))


@pytest.mark.parametrize("order", ["in_time_order", "decay_sent_first", "one_frame_decay_first", "one_frame_sustain_first"])
def test_sustain_and_decay_orders(order):
    """Stamped 200 / 300: whichever is sent first, ADCY divides by the new sustain. On one frame the sending order decides."""
    g, r = _single(2)
    r.on(10, 60)
    one_frame = order.startswith("one_frame")
    calls = [("ASTN", 0.2, 200), ("ADCY", 0.006, 200 if one_frame else 300)]
    if order in ("decay_sent_first", "one_frame_decay_first"):
        calls = calls[::-1]
    for fourcc, value, t in calls:
        r.env(t, fourcc, value)
    r.on(400, 57)
    r.all_off(1200)
    got = FR._run(g, [r], [300, 20, 1500])
    sustain_then = 0.6 if order == "one_frame_decay_first" else 0.2
    st = r.m.envelope_state()
    f = np.float32
    assert st["sustain_level"] == f(0.2) and st["decay_rate"] == f(f(f(1.0) - f(sustain_then)) / f(f(6000000.0) / f(1e9) * f(SR)))
    _check_audio(got, r, 1820)


def test_pool_of_33_takes_the_parameters_beyond_lane_32():
    g, r = _single(33)
    for k in range(33):
        r.on(5 + k, 36 + k, 0.5, 0.0)       # slot k
    r.env(60, "AATK", 0.003)                  # every note is in Attack
    r.env(200, "ASTN", 0.25)
    r.env(200, "ADCY", 0.002)
    r.off(600, 32)
    r.env(640, "AREL", 0.001)                 # slot 32 releases
    got = FR._run(g, [r], [300, 20, 800])
    rec = r.m.notes[r.ids[32]]
    assert rec.slot == 32 and rec.end is not None and rec.end <= 1120 and len(r.m.env_log) == 4     # the short release freed it
    assert r.m.state()["active_voices"] == 32
    _check_audio(got, r, 1120)


def test_read_back_on_free_slots_and_zero_times():
    """No note at all: every slot is free, the parameters move all the same; the Duration edges; a zero release frees the slot with the write of the note-off."""
    g, r = _single(4)
    r.env(10, "AATK", 4e-10)                  # a zero Duration: f32::MAX
    r.env(20, "AREL", 0.6e-9)                 # 1 ns
    r.env(30, "AHLD", 0.0)
    r.env(40, "ADCY", 0.0)
    FR._run(g, [r], [300])
    st = r.m.envelope_state()
    assert st["attack_rate"] == A.F32_MAX and st["decay_rate"] == A.F32_MAX and np.isfinite(st["release_rate"]) and st["zero_times"] == 1 | 2
    a = r.on(310, 60)                         # no attack, no hold, no decay: at the sustain level with its second frame
    r.env(400, "AREL", 0.0)
    r.off(500, a)
    got = FR._run(g, [r], [20, 700], pos=300)
    assert r.m.state()["active_voices"] == 0 and r.m.notes[r.ids[a]].end == 1020 and r.m.envelope_state()["zero_times"] == 1 | 2 | 4
    FR._assert_equal(got, r.expected(720, origin=300))


def test_in_front_of_the_start_time_and_while_stopping():
    g, r = _single(2, transient=True, start_time=64)
    r.env(30, "ADCY", 0.002)                  # stamped later than the ASTN: it sees 0.3
    r.env(5, "ASTN", 0.3)
    r.on(64, 60)
    r.stop(700)
    r.env(720, "ASTN", 0.9)                   # dropped
    got = FR._run(g, [r], [300, 20, 1000])
    f = np.float32
    st = r.m.envelope_state()
    assert [t for t, _, _ in r.m.env_log] == [64, 64] and st["sustain_level"] == f(0.3) and st["decay_rate"] == f(f(f(1.0) - f(0.3)) / f(f(2000000.0) / f(1e9) * f(SR)))
    assert r.m.state()["stopped"]
    _check_audio(got, r, 1320)
