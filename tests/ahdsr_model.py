"""An independent model of the reference's AHDSR envelope (src/utils/ahdsr.rs) in numpy.float32 arithmetic: `run`, `note_on`, `note_off`,
`reset`, `apply_scaling` and the parameter set-up order of `new_with_scaling` + `set_sample_rate`. Written from the envelope's behaviour —
every operation is one rounded f32 operation, in the order the reference performs it — so that the expected output of the GPU tests does not
come from the code under test. Times are f32 seconds (what Duration::as_secs_f32() returns)."""
import numpy as np

F = np.float32
IDLE, ATTACK, HOLD, DECAY, SUSTAIN, RELEASE = range(6)
F32_MAX = np.finfo(np.float32).max
F32_EPS = np.finfo(np.float32).eps
SILENCE = F(0.001)                 # -60 dB: where a release ends
UNINITIALIZED_SAMPLE_RATE = 66666  # the placeholder rate of freshly built parameters
EULER_DIV_2 = F(F(np.e) / F(2.0))

DEFAULTS = dict(attack_s=0.010, attack_scaling=0.0, hold_s=1.0, decay_s=0.5, decay_scaling=0.0, sustain_level=0.75, release_s=1.0, release_scaling=0.0)


def apply_scaling(value, scaling):
    """Curve of a normalised value: 0 linear, > 0 logarithmic (fast start), < 0 exponential (slow start): x^(1 + |s|^(e/2) * 16), mirrored
    for positive scalings."""
    value, scaling = F(value), F(scaling)
    if scaling == 0 or value == 0:
        return value
    s = F(-scaling)
    with np.errstate(all="ignore"):
        if s > 0:
            return F(np.power(value, F(F(1.0) + F(np.power(s, EULER_DIV_2)) * F(16.0))))
        return F(F(1.0) - F(np.power(F(F(1.0) - value), F(F(1.0) + F(np.power(F(-s), EULER_DIV_2)) * F(16.0)))))


class Params:
    """The rates the envelope runs on. Built like the sampler builds them: every setter once at the placeholder rate (the sustain level is
    still 0 when the decay rate is first computed), then once more at the real rate unless that IS the placeholder."""

    def __init__(self, sample_rate, **kw):
        a = dict(DEFAULTS)
        a.update(kw)
        for k in a:
            if k not in DEFAULTS:
                raise AttributeError(k)
        self.attack_s, self.hold_s, self.decay_s, self.release_s = F(a["attack_s"]), F(a["hold_s"]), F(a["decay_s"]), F(a["release_s"])
        self.attack_scaling, self.decay_scaling, self.release_scaling = F(a["attack_scaling"]), F(a["decay_scaling"]), F(a["release_scaling"])
        self.sample_rate = UNINITIALIZED_SAMPLE_RATE
        self.sustain_level = F(0.0)
        self._rates()
        self.sustain_level = F(a["sustain_level"])
        if sample_rate != self.sample_rate:
            self.sample_rate = int(sample_rate)
            self._rates()
        self.hold_samples = F(self.hold_s * F(self.sample_rate))

    def _rates(self):
        sr = F(self.sample_rate)
        self.attack_rate = F32_MAX if self.attack_s == 0 else F(F(1.0) / F(self.attack_s * sr))
        self.decay_rate = F32_MAX if self.decay_s == 0 else F(F(F(1.0) - self.sustain_level) / F(self.decay_s * sr))
        self.release_rate = F32_MAX if self.release_s == 0 else F(F(1.0) / F(self.release_s * sr))


class Envelope:
    def __init__(self):
        self.stage = IDLE
        self.target_volume = self.hold_samples_remaining = self.release_output = self.output = F(0.0)

    def note_on(self, p, volume=1.0):
        self.target_volume = F(volume)
        if p.attack_rate == F32_MAX:   # no attack: straight to hold or decay, at full level
            self.output = F(volume)
            if p.hold_s > 0:
                self.stage, self.hold_samples_remaining = HOLD, p.hold_samples
            else:
                self.stage = DECAY
        else:
            self.output, self.stage = F(0.0), ATTACK

    def note_off(self, p):
        if p.release_s > 0:
            self.target_volume = F(0.0)
            self.release_output = self.output
            self.stage = RELEASE if self.release_output > F32_EPS else IDLE
        else:
            self.output = self.release_output = F(0.0)
            self.stage = IDLE

    def reset(self):
        self.output, self.stage = F(0.0), IDLE

    def run(self, p):
        """One frame: advance the state machine, then hand out the (curve-scaled) level."""
        with np.errstate(all="ignore"):
            if self.stage == ATTACK:
                self.output = F(self.output + p.attack_rate)
                if self.output >= self.target_volume:
                    self.output = self.target_volume
                    self.target_volume = p.sustain_level
                    if p.hold_s > 0:
                        self.stage, self.hold_samples_remaining = HOLD, p.hold_samples
                    else:
                        self.stage = DECAY
            elif self.stage == HOLD:
                self.hold_samples_remaining = F(self.hold_samples_remaining - F(1.0))
                if self.hold_samples_remaining <= 0:
                    self.stage = SUSTAIN if p.decay_s == 0 else DECAY
            elif self.stage == DECAY:
                if self.output > p.sustain_level:
                    self.output = F(self.output - p.decay_rate)
                    if self.output <= p.sustain_level:
                        self.output, self.stage = p.sustain_level, SUSTAIN
                else:
                    self.output = F(self.output + p.decay_rate)
                    if self.output >= p.sustain_level:
                        self.output, self.stage = p.sustain_level, SUSTAIN
            elif self.stage == RELEASE:
                self.output = F(self.output - F(self.release_output * p.release_rate))
                if self.output <= SILENCE:
                    self.output, self.stage = F(0.0), IDLE
            # the stage the frame ends in decides the curve (Hold, Sustain and Idle have none)
            if self.stage == ATTACK and p.attack_scaling != 0:
                progress = F(self.output / max(self.target_volume, F32_EPS))
                return F(apply_scaling(progress, p.attack_scaling) * self.target_volume)
            if self.stage == DECAY and p.decay_scaling != 0:
                tv, sus = self.target_volume, p.sustain_level
                rng = max(F(abs(F(tv - sus))), F32_EPS)
                progress = F(F(tv - self.output) / rng) if tv > sus else F(F(self.output - tv) / rng)
                sp = apply_scaling(progress, p.decay_scaling)
                return F(tv - F(sp * rng)) if tv > sus else F(tv + F(sp * rng))
            if self.stage == RELEASE and p.release_scaling != 0:
                initial = max(self.output, F32_EPS)
                progress = F(F(1.0) - F(self.output / initial))
                return F(initial * F(F(1.0) - apply_scaling(progress, p.release_scaling)))
            return self.output


def render(params, n_frames, note_off_at=None, pieces=None):
    """The gain of every frame of a voice that starts at frame 0, as the sampler applies the envelope: per process call (`pieces`: their
    lengths; default one call), a call that begins in Sustain or Idle multiplies by the current output, any other runs frame by frame; the
    note-off lands in front of frame `note_off_at` (a call boundary). Returns (gains[n_frames] f32, [(end frame, stage) of every call], the
    index of the call in which the envelope became Idle or None)."""
    env = Envelope()
    env.note_on(params, 1.0)
    gains = np.zeros(n_frames, dtype=np.float32)
    bounds = [0]
    for n in (pieces or [n_frames]):
        bounds.append(bounds[-1] + n)
    assert bounds[-1] == n_frames
    if note_off_at is not None and note_off_at not in bounds:
        bounds = sorted(set(bounds) | {note_off_at})
    stages, idle_call = [], None
    for ci in range(len(bounds) - 1):
        a, b = bounds[ci], bounds[ci + 1]
        if note_off_at is not None and a == note_off_at:
            env.note_off(params)
        if idle_call is not None:
            gains[a:b] = 0.0   # the voice has been reset: it renders nothing any more
        elif env.stage in (SUSTAIN, IDLE):
            gains[a:b] = env.output
        else:
            for i in range(a, b):
                gains[i] = env.run(params)
        if idle_call is None and env.stage == IDLE:
            idle_call = ci
        stages.append((b, env.stage))
    return gains, stages, idle_call
