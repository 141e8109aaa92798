"""Independent restatement of the reference Sampler's messages that change EVERY voice of the pool while notes sound
(Sampler::process_playback_messages, src/generator/sampler.rs:656-731), on top of tests/sampler_model.py and tests/granular_sampler_model.py:

  SetParameter(AMP_*)      -> set_envelope_parameter (sampler.rs:184-217, :1122-1131) on the sampler's ONE AhdsrParameters, setter by setter
                              (src/utils/ahdsr.rs:143-249): set_sustain_level stores the level and leaves decay_rate as it is; set_decay_time
                              divides (1 - sustain_level) as it holds then; a zero time is a rate of f32::MAX; hold_time > 0, decay_time.is_zero()
                              and release_time > 0 are read where the envelope changes stage; a Hold in progress keeps hold_samples_remaining.
  SetModulation / ClearModulation, SetParameter(ML1R | ML2R | ML1W | ML2W)   (:704-720, :1148-1186, :1210-1244): the matrix of every voice.
  SamplerMessage::SetLoopRange   (:1246-1271, voice.rs:312-339): every voice's pool; None is no loop at all.

Written from the reference, not from the device code. Every message goes through the models' queues: applied at the top of the Sampler::write
whose first frame is its sample time (or the start time), in (sample_time, sending order), dropped while the sampler stops (:663-664).

Duration::from_secs_f32(s).as_secs_f32() is restated as the standard library's documentation describes it (nanoseconds rounded to nearest, ties
to even; then `secs as f32 + nanos as f32 / 1e9f32`): no copy of the library's source is at hand to check the rounding rule against."""
from fractions import Fraction

import numpy as np

import ahdsr_model as A
import granular_sampler_model as G
import sampler_model as sm

F32 = np.float32
ENV_IDS = ("AATK", "AHLD", "ADCY", "ASTN", "AREL")   # Sampler::envelope_parameters() (sampler.rs:173-181)
# (id, name, min, max, default, exponent of ParameterScaling::Exponential or None) — sampler.rs:130-170
ENV_DESCRIPTORS = (("AATK", "Attack", 0.0, 10.0, 0.001, 2.0), ("AHLD", "Hold", 0.0, 10.0, 0.75, 2.0), ("ADCY", "Decay", 0.0, 10.0, 0.5, 2.0),
                   ("ASTN", "Sustain", 0.0, 1.0, 0.75, None), ("AREL", "Release", 0.0, 10.0, 1.0, 2.0))
HOLD_ZERO, DECAY_ZERO, RELEASE_ZERO = 1, 2, 4


def duration_round_trip(seconds):
    """(Duration::from_secs_f32(seconds.max(0.0)).as_secs_f32(), Duration::is_zero())"""
    s = max(F32(seconds), F32(0.0))
    total_ns = round(Fraction(float(s)) * 10**9)          # exact product, half to even
    secs, nanos = divmod(int(total_ns), 10**9)
    return F32(F32(secs) + F32(F32(nanos) / F32(1e9))), total_ns == 0


def resolve_envelope(fourcc, value, normalized):
    """Sampler::parameter_update_value (sampler.rs:862-883): a raw value clamped, a normalized one clamped to 0..=1 and denormalized."""
    d = [d for d in ENV_DESCRIPTORS if d[0] == fourcc]
    if not d:
        raise ValueError("Invalid/unknown envelope parameter '%s'" % fourcc)
    _, _, lo, hi, _, exponent = d[0]
    value, lo, hi = F32(value), F32(lo), F32(hi)
    if value != value:
        raise ValueError("not a number")
    if not normalized:
        return F32(min(max(value, lo), hi))
    n = F32(min(max(value, F32(0.0)), F32(1.0)))
    if exponent is not None:
        n = F32(float(n) ** exponent)                      # f32::powf(2.0): the exact square fits a double, rounded once
    return F32(lo + F32(n * F32(hi - lo)))


def apply_envelope_parameter(p, fourcc, raw):
    """One setter of AhdsrParameters on an ahdsr_model.Params (ahdsr.rs:143-249), after sampler.rs:189-209."""
    sr = F32(p.sample_rate)
    if fourcc == "ASTN":
        p.sustain_level = F32(raw)                         # decay_rate stays as it is
        return
    secs, zero = duration_round_trip(raw)
    if fourcc == "AATK":
        p.attack_s = secs
        p.attack_rate = A.F32_MAX if secs == 0 else F32(F32(1.0) / F32(secs * sr))
    elif fourcc == "AHLD":
        p.hold_s = secs
        p.hold_samples = F32(secs * sr)
    elif fourcc == "ADCY":
        p.decay_s = secs
        p.decay_rate = A.F32_MAX if zero else F32(F32(F32(1.0) - p.sustain_level) / F32(secs * sr))
    elif fourcc == "AREL":
        p.release_s = secs
        p.release_rate = A.F32_MAX if secs == 0 else F32(F32(1.0) / F32(secs * sr))
    else:
        raise ValueError(fourcc)


def envelope_state(p):
    """What pg_graph_sampler_envelope_params reports (_capi.sampler_envelope_state_dict)."""
    zero = (HOLD_ZERO if p.hold_s == 0 else 0) | (DECAY_ZERO if p.decay_s == 0 else 0) | (RELEASE_ZERO if p.release_s == 0 else 0)
    return dict(attack_rate=F32(p.attack_rate), decay_rate=F32(p.decay_rate), release_rate=F32(p.release_rate), sustain_level=F32(p.sustain_level),
                hold_samples=F32(p.hold_samples), attack_scaling=F32(p.attack_scaling), decay_scaling=F32(p.decay_scaling), release_scaling=F32(p.release_scaling),
                zero_times=zero)


class _EnvelopeMessages:
    """set_envelope_parameter for both models: they share the queue, _trigger and the one env_params."""

    env_log = None   # (frame, id, stage of every active slot's envelope) of every envelope message as it was applied

    def set_envelope_parameter(self, fourcc, value, t=0, normalized=False):
        if self.env_params is None:
            raise ValueError("Invalid or unknown sampler parameter")   # sampler.rs:1128-1131, :1189
        raw = resolve_envelope(fourcc, value, normalized)
        if self.env_log is None:
            self.env_log = []

        def fn(now):
            self.env_log.append((now, fourcc, self.envelope_stages()))
            apply_envelope_parameter(self.env_params, fourcc, raw)
        self._send(t, lambda now: self._trigger(lambda: fn(now)))

    def envelope_state(self):
        return envelope_state(self.env_params)


class LiveSamplerModel(_EnvelopeMessages, sm.SamplerModel):
    """A file sampler that takes AMP_* while notes sound."""

    def envelope_stages(self):
        """Stage of every ACTIVE slot's envelope (what a message finds)."""
        return [int(v.env.stage) for v in self.voices if v.is_active()]


class LiveGranularSamplerModel(_EnvelopeMessages, G.GranularSamplerModel):
    """A granular sampler that takes AMP_*, the matrix's messages and SetLoopRange while notes sound. file_frames: the frame count of the FILE
    buffer a loop range is normalised by (default: the granular buffer's — a mono buffer at the graph's rate is its own granular buffer)."""

    def __init__(self, *a, file_frames=None, **kw):
        super().__init__(*a, **kw)
        self.file_frames = int(file_frames) if file_frames is not None else len(self.buf)
        self.live_log = []   # (frame, kind, active slots, slots with living grains, the free slots) of every matrix / loop message as it was applied

    def envelope_stages(self):
        return [int(v.env.stage) for v in self.slots if v.is_active()]

    def _matrices(self):
        if self.modulation is None:
            raise ValueError("only available when granular playback is enabled with a matrix")
        return [v.pool.matrix for v in self.slots]   # every voice, playing or free

    def _log(self, now, kind):
        self.live_log.append((now, kind, sum(1 for v in self.slots if v.is_active()), sum(1 for v in self.slots if v.pool.active.any()),
                              tuple(i for i, v in enumerate(self.slots) if not v.is_active())))

    def _matrix_message(self, t, kind, fn):
        matrices = self._matrices()

        def run(now):
            self._log(now, kind)
            for m in matrices:
                fn(m)
        self._send(t, lambda now: self._trigger(lambda: run(now)))

    def set_modulation(self, source, target, amount, bipolar=False, t=0):
        if not (0 <= source < 4 and 0 <= target < 7) or not (-1.0 <= float(F32(amount)) <= 1.0):
            raise ValueError("ParameterError")
        self._matrix_message(t, "route", lambda m: m.set_modulation(source, target, amount, bipolar))

    def clear_modulation(self, source, target, t=0):
        self.set_modulation(source, target, 0.0, False, t)

    def set_lfo_rate(self, lfo, rate, t=0):     # Lfo::set_rate: no draw, no phase change
        self._matrix_message(t, "lfo", lambda m: m.set_lfo_rate(lfo, rate))

    def set_lfo_waveform(self, lfo, waveform, t=0):
        self._matrix_message(t, "lfo", lambda m: m.set_lfo_waveform(lfo, waveform))

    def set_loop_range(self, loop_range, t=0):
        """loop_range: (start, end) in source frames of the file buffer, or None (sampler.rs:1246-1271): `start as f32 / frame_count as f32`."""
        if loop_range is not None:
            start, end = int(loop_range[0]), int(loop_range[1])
            if start >= self.file_frames or end > self.file_frames or start >= end:
                raise ValueError("Invalid loop range")
            total = F32(self.file_frames)
            norm = (F32(F32(start) / total), F32(F32(end) / total))
        else:
            norm = None

        def run(now):
            self._log(now, "loop")
            for v in self.slots:   # GrainPool::set_loop_range (granular.rs:516-518): playing_loop_range, the playhead and living grains stay
                v.pool.set_loop_range(norm)
        self._send(t, lambda now: self._trigger(lambda: run(now)))
