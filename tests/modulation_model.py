"""Independent numpy model of the modulation matrix of a granular sampler voice: Lfo (reference src/utils/dsp/lfo.rs), ModulationMatrix
(src/modulation/matrix.rs) with the sampler's four sources and seven targets (src/generator/sampler.rs:362-427,
src/generator/sampler/modulation.rs), and the grain pool of tests/granular_model.py fed with the frame's seven sums where
src/generator/sampler/granular.rs takes its `*_mod` arguments (:446-472, :524-640, :788-857). Everything is f32 where the reference has f32,
every operation rounded on its own (no fused multiply-add).

The reference runs the matrix in blocks of 64 frames in front of GrainPool::process (voice.rs:412-427). The blocks do not show in any value: the
LFOs are walked frame by frame, velocity and keytracking are constants, and the sums are formed per frame - so the model (like the device) forms
frame f's sums in front of frame f's scheduler step.

Random draws: tests/granular_model.py's Xoshiro256pp, random::<f32>() as defined there (unverified against the crate)."""
import math

import numpy as np

import granular_model as gm

F32 = np.float32
PI = F32(math.pi)
TAU = F32(2.0 * math.pi)
FRAC_PI_2 = F32(math.pi / 2.0)
SINE, TRIANGLE, RAMP_UP, RAMP_DOWN, SQUARE, RANDOM, SMOOTH_RANDOM = range(7)
LFO1, LFO2, VELOCITY, KEYTRACK = range(4)
SIZE, DENSITY, VARIATION, SPRAY, PAN_SPREAD, POSITION, STEP = range(7)
N_SOURCES, N_TARGETS = 4, 7
THRESHOLD = F32(0.001)   # ModulationMatrixSlot::update_target (matrix.rs:61)
ONE, TWO, HALF = F32(1.0), F32(2.0), F32(0.5)


def sine_approx(x):  # lfo.rs:9-19
    x = F32(x)
    B = F32(4.0) / PI
    C = F32(-4.0) / (PI * PI)
    P = F32(0.225)
    y = F32(F32(B * x) + F32(F32(C * x) * abs(x)))
    return F32(F32(P * F32(F32(y * abs(y)) - y)) + y)


class Lfo:
    def __init__(self, sample_rate, rate, waveform, rng_state=None):  # Lfo::new (lfo.rs:70-86)
        self.sr = int(sample_rate)
        self.phase = F32(0.0)
        self.phase_inc = F32(float(F32(rate)) / float(self.sr))
        self.waveform = int(waveform)
        self.rng = gm.Xoshiro256pp(rng_state)
        self.draws = 0
        self.sample_hold = self._bipolar()
        self.jitter_current = self._bipolar()
        self.jitter_target = self._bipolar()

    def _bipolar(self):  # rng.random::<f32>() * 2.0 - 1.0
        self.draws += 1
        return F32(F32(self.rng.f32() * TWO) - ONE)

    def _redraw(self):
        self.sample_hold = self._bipolar()
        self.jitter_current = self.jitter_target
        self.jitter_target = self._bipolar()

    def reset(self):  # lfo.rs:89-99
        self.phase = F32(0.0)
        if self.waveform in (RANDOM, SMOOTH_RANDOM):
            self._redraw()

    def set_rate(self, rate):  # lfo.rs:102-104
        self.phase_inc = F32(float(F32(rate)) / float(self.sr))

    def set_waveform(self, waveform):  # lfo.rs:117-119
        self.waveform = int(waveform)

    def run(self):  # one frame of Lfo::process (lfo.rs:172-252)
        ph, w = self.phase, self.waveform
        if w == SINE:
            p = F32(ph * TAU) if ph < HALF else F32(F32(ph - ONE) * TAU)
            v = sine_approx(p)
        elif w == TRIANGLE:
            if ph < F32(0.25):
                v = F32(ph * F32(4.0))
            elif ph < F32(0.75):
                v = F32(TWO - F32(ph * F32(4.0)))
            else:
                v = F32(F32(ph * F32(4.0)) - F32(4.0))
        elif w == RAMP_UP:
            v = F32(F32(ph * TWO) - ONE)
        elif w == RAMP_DOWN:
            v = F32(ONE - F32(ph * TWO))
        elif w == SQUARE:
            v = ONE if ph < HALF else F32(-1.0)
        elif w == RANDOM:
            v = self.sample_hold
        else:
            p = F32(FRAC_PI_2 - F32(ph * PI))
            t = F32(F32(ONE - sine_approx(p)) * HALF)
            v = F32(self.jitter_current + F32(t * F32(self.jitter_target - self.jitter_current)))
        self.phase = F32(self.phase + self.phase_inc)
        if self.phase >= ONE:
            self.phase = F32(self.phase - ONE)
            if w in (RANDOM, SMOOTH_RANDOM):
                self._redraw()
        return v


def bipolar_source(v, bipolar):  # matrix.rs:217-231
    return F32(v) if bipolar else F32(F32(v + ONE) / TWO)


def unipolar_source(v, bipolar):  # matrix.rs:201-215
    return F32(F32(v - HALF) * TWO) if bipolar else F32(v)


class Matrix:
    """ModulationState::create_matrix for Sampler::modulation_config (state.rs:91-156, sampler.rs:392-427)."""

    def __init__(self, sample_rate, rng_states=(None, None)):
        self.lfos = [Lfo(sample_rate, 1.0, SINE, rng_states[0]), Lfo(sample_rate, 2.0, TRIANGLE, rng_states[1])]
        self.velocity = F32(0.0)
        self.note_pitch = F32(F32(60.0) / F32(127.0))
        self.amount = np.zeros((N_SOURCES, N_TARGETS), dtype=F32)   # 0: the slot has no target for the parameter
        self.bipolar = np.zeros((N_SOURCES, N_TARGETS), dtype=np.int32)
        self.last = np.zeros(N_TARGETS, dtype=F32)

    def set_modulation(self, source, target, amount, bipolar):  # state.rs:174-220 + update_target (matrix.rs:60-83)
        amount = F32(amount)
        if not (0 <= source < N_SOURCES and 0 <= target < N_TARGETS) or not (F32(-1.0) <= amount <= F32(1.0)):
            raise ValueError("ParameterError")
        if abs(amount) < THRESHOLD:
            self.amount[source, target], self.bipolar[source, target] = F32(0.0), 0
        else:
            self.amount[source, target], self.bipolar[source, target] = amount, 1 if bipolar else 0

    def clear_modulation(self, source, target):
        self.set_modulation(source, target, 0.0, False)

    def has_route(self, source, target):
        return self.amount[source, target] != 0

    def set_lfo_rate(self, lfo, rate):  # the raw parameter update clamps (sampler.rs:870-874, :369-384)
        self.lfos[lfo].set_rate(min(max(F32(rate), F32(0.01)), F32(20.0)))

    def set_lfo_waveform(self, lfo, waveform):
        self.lfos[lfo].set_waveform(waveform)

    def note_on(self, note, volume):  # matrix.rs:394-408
        for l in self.lfos:
            l.reset()
        self.velocity = F32(volume)
        self.note_pitch = F32(F32(note) / F32(127.0))

    def process_frame(self):
        """One frame of every source, then the seven sums (matrix.rs:194-303): slot order LFO 1, LFO 2, velocity, keytracking."""
        raw = [self.lfos[0].run(), self.lfos[1].run(), self.velocity, self.note_pitch]
        out = np.zeros(N_TARGETS, dtype=F32)
        for t in range(N_TARGETS):
            total = F32(0.0)
            for s in range(N_SOURCES):
                a = self.amount[s, t]
                if a == 0:
                    continue
                v = bipolar_source(raw[s], self.bipolar[s, t]) if s < 2 else unipolar_source(raw[s], self.bipolar[s, t])
                total = F32(total + F32(v * a))
            out[t] = total
        self.last = out
        return out

    def state(self):
        """The matrix as pg_graph_voice_modulation_state reports it (_capi.modulation_state_dict)."""
        d = {"velocity": F32(self.velocity), "note_pitch": F32(self.note_pitch), "amount": self.amount.copy(), "bipolar": self.bipolar.copy(), "last": self.last.copy()}
        for i, l in enumerate(self.lfos):
            d[f"lfo{i}_phase"], d[f"lfo{i}_phase_inc"] = F32(l.phase), F32(l.phase_inc)
            d[f"lfo{i}_sample_hold"], d[f"lfo{i}_jitter_current"], d[f"lfo{i}_jitter_target"] = F32(l.sample_hold), F32(l.jitter_current), F32(l.jitter_target)
            d[f"lfo{i}_waveform"] = int(l.waveform)
            d[f"lfo{i}_rng"] = tuple(l.rng.s)
        return d


class ModGrainPool(gm.GrainPool):
    """GrainPool with the matrix in front of every frame. `zero`: targets whose sum is replaced by 0.0 before the pool sees it (what an
    implementation that forgot that input would compute - used to show that the tests' cases tell the difference)."""

    def __init__(self, sample_rate, buffer, params, matrix, rng_state=None, speed=1.0, volume=1.0, panning=0.0, zero=()):
        super().__init__(sample_rate, buffer, params, rng_state, speed, volume, panning)
        self.matrix = matrix
        self.zero = tuple(zero)
        self.m = np.zeros(N_TARGETS, dtype=F32)

    def playback_position(self):  # granular.rs:446-472
        p = self.p
        base = F32(p.position) if F32(p.step) == 0 else self.playhead
        if self.m[POSITION] != 0:
            base = F32(base + self.m[POSITION])
        if self.playing_loop_range and self.loop is not None:
            base = F32(gm.fold_into_loop_range(float(base), float(self.loop[0]), float(self.loop[1])))
        return gm.rem_euclid32(base, ONE)

    def update_trigger_phase(self):  # granular.rs:788-809
        if self.p.overlap_mode == gm.SEQUENTIAL:
            return True
        density_mult = F32(ONE + self.m[DENSITY])
        density = gm.clamp32(F32(F32(self.p.density) * density_mult), 1.0, 100.0)
        self.trigger_phase = F32(self.trigger_phase + F32(density / F32(self.sr)))
        if self.trigger_phase >= ONE:
            self.trigger_phase = F32(self.trigger_phase - ONE)
            return True
        return False

    def try_trigger_grain(self):  # granular.rs:524-603
        p = self.p
        if p.overlap_mode == gm.SEQUENTIAL and self.primary >= 0 and self.active[self.primary]:
            if self.window_phase[self.primary] < float(gm.crossfade_point(p.window)):
                return False
        if not self.trigger_new_grains or not self.update_trigger_phase():
            return False
        file_duration = float(len(self.buf)) / float(self.sr)
        modulated_spray = gm.clamp32(F32(F32(p.spray) + self.m[SPRAY]), 0.0, 1.0)
        spray_seconds = float(modulated_spray) * 2.0 * (self.rng.f64() - 0.5)
        spray_variation = spray_seconds / file_duration
        grain_position = float(self.playback_position()) + spray_variation
        if self.playing_loop_range and self.loop is not None:
            grain_position = gm.fold_into_loop_range(grain_position, float(self.loop[0]), float(self.loop[1]))
        grain_position = gm.rem_euclid64(grain_position, 1.0)
        index = self.activate_new_grain(grain_position)
        if p.overlap_mode == gm.SEQUENTIAL and index is not None:
            self.primary = index
        return index is not None

    def activate_new_grain(self, position):  # granular.rs:813-897 + Grain::activate (:1025-1067)
        p = self.p
        free = np.flatnonzero(~self.active)
        if len(free) == 0:
            self.failed_activations += 1
            return None
        index = int(free[0])
        rng = self.rng
        variation = gm.clamp32(F32(F32(p.variation) + self.m[VARIATION]), 0.0, 1.0)
        volume_scale = F32(ONE - F32(variation * rng.f32()))
        volume = F32(self.volume * volume_scale)
        random_semitones = float(variation) * (rng.f64() - 0.5)
        speed = self.speed * gm.pow2(random_semitones / 12.0) if random_semitones != 0.0 else self.speed
        min_scale = F32(ONE - F32(F32(0.75) * variation))
        max_scale = F32(ONE + F32(TWO * variation))
        size_scale = F32(min_scale + F32(F32(max_scale - min_scale) * rng.f32()))
        size_mult = F32(ONE + self.m[SIZE])
        grain_size_ms = gm.clamp32(F32(F32(p.size) * size_mult), 1.0, 1000.0)
        grain_size = max(int(F32(F32(F32(grain_size_ms * size_scale) * F32(self.sr)) / F32(1000.0))), 2)
        modulated_pan_spread = gm.clamp32(F32(F32(p.pan_spread) + self.m[PAN_SPREAD]), 0.0, 1.0)
        panning_spread = F32(modulated_pan_spread * F32(F32(rng.f32() * TWO) - ONE))
        panning = gm.clamp32(self.panning + panning_spread, -1.0, 1.0)
        pitch_variation_semitones = F32(F32(variation * F32(F32(rng.f32() * TWO) - ONE)) * HALF)
        varied_speed = speed * gm.pow2(float(pitch_variation_semitones) / 12.0)
        if p.playback_direction == gm.FORWARD:
            reverse = False
        elif p.playback_direction == gm.BACKWARD:
            reverse = True
        else:
            reverse = rng.boolean()
        self.active[index] = True
        self.window_mode[index] = p.window
        self.position[index] = min(max(position, 0.0), 1.0)
        self.volume_g[index] = gm.clamp32(volume, 0.0, 100.0)
        self.panning_g[index] = gm.clamp32(panning, -1.0, 1.0)
        self.samples_remaining[index] = grain_size
        if self.playing_loop_range and self.loop is not None:
            self.has_loop[index] = True
            self.loop_start[index] = float(self.loop[0])
            self.loop_end[index] = float(self.loop[1])
        else:
            self.has_loop[index] = False
            self.loop_start[index] = 0.0
            self.loop_end[index] = 0.0
        base_increment = varied_speed / float(len(self.buf))
        self.increment[index] = base_increment * (-1.0 if reverse else 1.0)
        self.window_phase[index] = 0.0
        self.window_increment[index] = 1.0 / float(grain_size)
        self.activations.append((self.frame, index))
        return index

    def advance_playhead(self):  # granular.rs:607-640
        step = F32(self.p.step)
        speed_mult = F32(ONE + self.m[STEP])
        modulated_step = F32(step * speed_mult)
        self.playhead = F32(self.playhead + F32(modulated_step / F32(len(self.buf))))
        if self.loop is not None:
            ls, le = self.loop
            if self.playing_loop_range:
                self.playhead = F32(gm.fold_into_loop_range(float(self.playhead), float(ls), float(le)))
            elif ls <= self.playhead < le:
                self.playing_loop_range = True
            elif self.playhead >= ONE:
                self.playhead = F32(self.playhead - ONE)
            elif self.playhead < F32(0.0):
                self.playhead = F32(self.playhead + ONE)
        elif self.playhead >= ONE:
            self.playhead = F32(self.playhead - ONE)
        elif self.playhead < F32(0.0):
            self.playhead = F32(self.playhead + ONE)

    def process(self, n_frames):
        """n_frames of SamplerVoice::process's granular branch (voice.rs:412-427): the matrix in front of every frame of GrainPool::process.
        Returns what gm.GrainPool.process returns."""
        out = np.zeros((n_frames, 2), dtype=F32)
        cnt = np.zeros(n_frames, dtype=np.int64)
        S = np.zeros((n_frames, 2), dtype=np.float64)
        move_playhead = F32(self.p.step) != 0
        with np.errstate(all="ignore"):
            for f in range(n_frames):
                m = self.matrix.process_frame().copy()
                for t in self.zero:
                    m[t] = F32(0.0)
                self.m = m
                self.try_trigger_grain()
                if move_playhead:
                    self.advance_playhead()
                lt, rt = self._process_grains()
                accl, accr = F32(0.0), F32(0.0)
                for k in range(len(lt)):
                    accl = F32(accl + lt[k])
                    accr = F32(accr + rt[k])
                out[f, 0], out[f, 1] = accl, accr
                cnt[f] = len(lt)
                S[f, 0] = np.abs(lt.astype(np.float64)).sum()
                S[f, 1] = np.abs(rt.astype(np.float64)).sum()
                self.frame += 1
        return out, cnt, S


def make_matrix(sample_rate, rates=(1.0, 2.0), waveforms=(SINE, TRIANGLE), rng_states=(None, None), velocity=1.0, note=60, routes=()):
    """pg_graph_set_voice_modulation_matrix: create_matrix, the parameter and routing updates in front of the note, then start(note, velocity)."""
    mx = Matrix(sample_rate, rng_states)
    for l in range(2):
        mx.set_lfo_rate(l, rates[l])
        mx.set_lfo_waveform(l, waveforms[l])
    for (s, t, amount, bipolar) in routes:
        mx.set_modulation(s, t, amount, bipolar)
    mx.note_on(note, velocity)
    return mx
