"""The rig the granular samplers' tests share (tests/test_gpu_granular_sampler.py on the device, tests/test_granular_sampler_model.py for the
scenarios both run): one granular-mode sampler on the GPU and its model (tests/granular_sampler_model.py) driven by the same calls; after every
write the slot table, every slot's grain state and matrix state and the parameters are compared bit for bit, and the audio as values.
A plain module: no test lives here."""
import numpy as np

import granular_model as gm
import granular_params_model as gpm
import granular_sampler_model as G
from phonic_amd import _capi

SR = 48000
MF = 256
BUF = gm.make_buffer(3000, 5)        # mono at the graph's rate: it IS its granular buffer
POOL_RNG = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111222233334444, 0x5555666677778888)
LFO_RNG = ((11, 12, 13, 14), (21, 22, 23, 24))
ENV = dict(attack_s=0.002, hold_s=0.003, decay_s=0.004, sustain_level=0.6, release_s=0.005)
# grains of a few milliseconds, so that pools run dry inside a write
SHORT = dict(size=3.0, density=100.0, variation=0.4, spray=0.3, pan_spread=0.5, position=0.3, step=1.0, playback_direction=gm.RANDOM)
UNKNOWN = 999999
PARAM_ID = dict(transpose="STRN", finetune="SFTN", volume="SVOL", panning="SPAN")


def resolve(name, value, normalized):
    """tests/sampler_rig.py's: the raw value a base-parameter update resolves to (it asks the CPU oracle for the decibel scaling)."""
    import sampler_rig

    return sampler_rig.resolve(name, value, normalized)


def model_params(kw, loop_range=None, rng_state=POOL_RNG):
    p = gm.Params(**kw)
    p.loop_range = loop_range
    p.rng_state = rng_state          # (the base state the slots' pool states are derived from)
    return p


def capi_params(kw, loop_range=None, rng_state=POOL_RNG):
    return _capi.granular_params(loop_range=loop_range, rng_state=rng_state, **kw)


def capi_modulation(mod):
    if mod is None:
        return None
    return _capi.modulation_params(rates=mod.get("rates"), waveforms=mod.get("waveforms"), rng_states=mod.get("rng_states"), routes=mod.get("routes", ()))


class ModelOnly:
    """Stands where a rig has no graph: note_on answers with the id the model is about to hand out, everything else does nothing."""

    def __init__(self, m):
        self._m = m

    def sampler_note_on(self, *a):
        return self._m.note_ids[0] + 1

    def __getattr__(self, name):
        return lambda *a, **kw: None


class Rig:
    """g None: the model alone (what a script does can be asserted without a GPU)."""

    def __init__(self, g, mixer, note_ids, voice_count, kw=SHORT, envelope=None, modulation=None, rng_states=None, transient=False, start_time=0, loop_range=None,
                 buf=BUF, buffer_id=None):
        self.m = G.GranularSamplerModel(SR, buf, model_params(kw, loop_range), voice_count=voice_count, envelope=envelope, modulation=modulation, rng_states=rng_states,
                                        transient=transient, note_ids=note_ids, start_time=start_time)
        self.n, self.modulation = voice_count, modulation
        self.ids, self.times = [], []
        if g is None:
            self.g, self.s = ModelOnly(self.m), None
            return
        self.g = g
        self.buf = buffer_id if buffer_id is not None else g.add_sample_buffer(buf, 1, SR)
        self.s = g.add_granular_sampler(mixer, self.buf, capi_params(kw, loop_range), capi_modulation(modulation), rng_states, voice_count=voice_count, envelope=envelope,
                                        transient=transient, start_time=start_time)

    def _id(self, k):
        return UNKNOWN if k is None else self.ids[k]

    def on(self, t, note, volume=1.0, panning=0.0):
        self.times.append(t)
        a, b = self.g.sampler_note_on(self.s, note, volume, panning, t), self.m.note_on(note, volume, panning, t)
        assert a == b, (a, b)
        self.ids.append(a)
        return len(self.ids) - 1

    def off(self, t, k):
        self.times.append(t)
        self.g.sampler_note_off(self.s, self._id(k), t)
        self.m.note_off(self._id(k), t)

    def all_off(self, t):
        self.times.append(t)
        self.g.sampler_all_notes_off(self.s, t)
        self.m.all_notes_off(t)

    def speed(self, t, k, speed, glide=None):
        self.times.append(t)
        self.g.sampler_set_note_speed(self.s, self._id(k), speed, t, glide)
        self.m.set_note_speed(self._id(k), speed, t, glide)

    def vol(self, t, k, v):
        self.times.append(t)
        self.g.sampler_set_note_volume(self.s, self._id(k), v, t)
        self.m.set_note_volume(self._id(k), v, t)

    def pan(self, t, k, p):
        self.times.append(t)
        self.g.sampler_set_note_panning(self.s, self._id(k), p, t)
        self.m.set_note_panning(self._id(k), p, t)

    def param(self, t, name, value, normalized=False):
        self.times.append(t)
        self.g.sampler_set_parameter(self.s, PARAM_ID[name], value, t, normalized)
        self.m.set_parameter(name, resolve(name, value, normalized), t)

    def gparam(self, t, fourcc, value, normalized=False):
        self.times.append(t)
        self.g.sampler_set_granular_parameter(self.s, fourcc, value, t, normalized)
        self.m.set_granular_parameter(fourcc, value, t, normalized)

    def stop(self, t):
        self.times.append(t)
        self.g.sampler_stop(self.s, t)
        self.m.stop(t)

    def slot_of(self, k):
        """The slot note k was started in (the model's record)."""
        return [a[2] for a in self.m.allocations if a[1] == self.ids[k]][0]

    def check_state(self, where):
        got, exp = self.g.sampler_state(self.s), self.m.state()
        slots_g, slots_e = got.pop("slots"), exp.pop("slots")
        assert got == exp, (where, got, exp)
        for i, (a, b) in enumerate(zip(slots_g, slots_e)):
            assert a == b, (where, "slot", i, a, b)
        for k in range(self.n):
            bad = gm.states_equal(self.m.grain_state(k), self.g.sampler_voice_grain_state(self.s, k))
            assert bad == [], (where, "grain state of slot", k, bad)
            if self.modulation is not None:
                bad = gm.states_equal(self.m.modulation_state(k), self.g.sampler_voice_modulation_state(self.s, k))
                assert bad == [], (where, "matrix state of slot", k, bad)
        bad = gm.states_equal(self.m.params_state(), self.g.sampler_granular_params(self.s))
        assert bad == [], (where, "parameters", bad)


def assert_audio(got, exp, where=None):
    """Equal as values: an all-zero frame may carry the other zero's sign."""
    got, exp = np.asarray(got, np.float32).reshape(-1, 2), np.asarray(exp, np.float32).reshape(-1, 2)
    same = got == exp
    assert same.all(), (where, "first differing frame", int(np.flatnonzero(~same.all(axis=1))[0]), float(np.abs(got - exp).max()))


def run(g, rigs, sizes, pos=0, cuts=(), audio=True):
    """The writes, from frame `pos` on; after every one every sampler's read-backs against its model and (one sampler: exactly) the audio.
    cuts: sample times of the owning mixer chain's events that are no message of the rigs' samplers. Returns (device audio, model audio of each rig)."""
    out, exp = [], [[] for _ in rigs]
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        for i, r in enumerate(rigs):
            others = set(cuts) | set(t for q in rigs if q is not r for t in q.times)   # a mixer's events cut every source's call
            exp[i].append(r.m.write(n, pos, cuts=others))
            r.check_state((k, pos + n))
        if audio and len(rigs) == 1:
            assert_audio(buf, exp[0][-1], (k, pos))
        pos += n
        out.append(buf)
    assert g.device_errors() == 0
    return np.concatenate(out).reshape(-1, 2), [np.concatenate(e) for e in exp]


def run_model(rigs, sizes, pos=0, cuts=()):
    for n in sizes:
        for r in rigs:
            r.m.write(n, pos, cuts=cuts)
        pos += n


# ---- scenarios the CPU test derives by hand and the GPU test repeats on the device ----
# One grain per note and nothing random in its length: Cloud at 100 Hz triggers at the note's first frame (trigger_phase starts at 1.0) and again
# 480 frames later at the earliest; size 2 ms at 48 kHz without variation is 96 frames: the grain born at frame t sounds at frames t .. t + 95.
ONE_GRAIN = dict(size=2.0, density=100.0, variation=0.0, spray=0.0, pan_spread=0.0, position=0.3, step=0.0)
GRAIN_FRAMES = 96
# attack, hold and decay of zero length, sustain 1.0: the note is at full level at once; a release of 50 frames: the raw level falls by 1 / 50 of
# the level at note-off per frame — far above SILENCE (0.001) after 49 frames, at or below it after 50: Idle with the 50th frame behind the note-off
FLAT_ENV = dict(attack_s=0.0, hold_s=0.0, decay_s=0.0, sustain_level=1.0, release_s=50.0 / SR)
RELEASE_FRAMES = 50


def dry_scenario(r, probe):
    """Three slots, no envelope. A and B start at frame 0 in slots 0 and 1; A's note-off at frame 10 stops its pool, whose one grain sounds through
    frame 95: the pool is exhausted behind frame 95. The probe note C at frame `probe`: 95 -> the span [10, 95) ends with A's grain still alive,
    A is active, C takes the free slot 2; 96 -> the span [10, 96) holds frame 95, A is freed at its end, C takes slot 0. Returns C's index."""
    a = r.on(0, 60)
    r.on(0, 64)
    r.off(10, a)
    return r.on(probe, 67)


def idle_scenario(r, probe):
    """The same with FLAT_ENV: A's note-off at frame 10 starts a release of 50 frames; the envelope is Idle behind frame 59. C at 59 -> slot 2,
    at 60 -> slot 0."""
    a = r.on(0, 60)
    r.on(0, 64)
    r.off(10, a)
    return r.on(probe, 67)
