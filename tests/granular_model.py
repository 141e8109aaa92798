"""Independent numpy model of the sampler's grain engine: GrainWindow, Grain and GrainPool of the reference's
src/generator/sampler/granular.rs, with the reference's number widths (f32 where it has f32, f64 where f64, `as usize` truncations as
written) and every `*_mod` input 0.0 (a sampler without modulation routings). The per-frame scheduler (try_trigger_grain, update_trigger_phase,
advance_playhead, activate_new_grain) is scalar code; Grain::process and sample_at_position run over all 100 slots at once as numpy arrays,
which changes no value: every slot's arithmetic is its own.

Random draws are rand 0.9's on Xoshiro256++ (SmallRng on 64-bit targets), as rand's documentation describes them (unverified against the
crate's source): random::<f32>() = (next_u64 >> 40) * 2^-24, random::<f64>() = (next_u64 >> 11) * 2^-53, random::<bool>() = top bit of
next_u64.

Transcendentals: the window table's cos / exp are the correctly rounded f32 results (evaluated in f64, rounded once), 2^x of the pitch
variation is the correctly rounded f64 result (decimal arithmetic): what a libm aims at, independent of the libm of the machine at hand.

GrainPool.process(n) returns, per frame: the stereo output (f32, terms added in slot order), the number of contributing grains n, and
S = sum |term| per channel (f64) - the inputs of the sum-order bound |a - b| <= 2 n 2^-23 S between two f32 summation orders of the same terms.
"""
import decimal
import math

import numpy as np

F32 = np.float32
POOL_SIZE = 100
LUT_N = 2048
ENVELOPE_THRESHOLD = F32(0.001)
WINDOWS = ("Hann", "Blackman", "Triangle", "Tukey", "Trapezoid", "Exponential", "RampUp", "RampDown")
CLOUD, SEQUENTIAL = 0, 1
FORWARD, BACKWARD, RANDOM = 0, 1, 2
M64 = (1 << 64) - 1
FIXED_SEED = 0x5EED0000


def crossfade_point(window):  # GrainWindowMode::sequential_crossfade_point (granular.rs:78-94)
    return F32(0.5) if window <= 3 else (F32(0.9) if window == 4 else F32(0.8))


def _cosf(x):  # correctly rounded f32 cosine of an f32
    return F32(math.cos(float(x)))


def _expf(x):
    return F32(math.exp(float(x)))


def build_lut():
    """GrainWindow::<2048>::new (granular.rs:112-196)."""
    lut = np.zeros((8, LUT_N), dtype=F32)
    PI = F32(math.pi)
    one, half, two = F32(1.0), F32(0.5), F32(2.0)
    for i in range(LUT_N):
        phase = F32(i) / F32(LUT_N)
        lut[0, i] = half * (one - _cosf(two * PI * phase))
        pi_phase = PI * phase
        lut[1, i] = F32(0.42) - half * _cosf(two * pi_phase) + F32(0.08) * _cosf(F32(4.0) * pi_phase)
        lut[2, i] = two * phase if phase < half else two * (one - phase)
        width = F32(0.5) / two
        if phase < width:
            lut[3, i] = half * (one - _cosf(PI * (phase / width)))
        elif phase > one - width:
            lut[3, i] = half * (one - _cosf(PI * ((one - phase) / width)))
        else:
            lut[3, i] = one
        rw = F32(0.1)
        if phase < rw:
            lut[4, i] = phase / rw
        elif phase > one - rw:
            lut[4, i] = (one - phase) / rw
        else:
            lut[4, i] = one
        lut[5, i] = _expf(-F32(6.0) * abs(phase - half))
        if phase < F32(0.9):
            lut[6, i] = phase / F32(0.9)
        else:
            lut[6, i] = half * (one + _cosf(PI * ((phase - F32(0.9)) / F32(0.1))))
        if phase < F32(0.1):
            lut[7, i] = half * (one - _cosf(PI * (phase / F32(0.1))))
        else:
            lut[7, i] = one - ((phase - F32(0.1)) / F32(0.9))
    return lut


_LUT = None


def lut():
    global _LUT
    if _LUT is None:
        with np.errstate(all="ignore"):
            _LUT = build_lut()
    return _LUT


def window_sample(mode, phase):
    """GrainWindow::sample (granular.rs:201-215) for one f64 phase."""
    t = lut()[mode]
    index_float = float(phase) * float(LUT_N - 1)
    index = int(index_float) & (LUT_N - 1)
    fraction = F32(index_float - math.trunc(index_float))
    nxt = (index + 1) & (LUT_N - 1)
    if index < LUT_N - 1:
        return F32(t[index] * (F32(1.0) - fraction) + t[nxt] * fraction)
    return t[LUT_N - 1]


class Xoshiro256pp:
    def __init__(self, state=None):
        if state is None or not any(int(x) for x in state):  # SplitMix64 of the fixed seed, as for the Delay's LFO
            z = FIXED_SEED
            state = []
            for _ in range(4):
                z = (z + 0x9E3779B97F4A7C15) & M64
                x = z
                x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
                x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
                state.append(x ^ (x >> 31))
        self.s = [int(x) & M64 for x in state]

    def next_u64(self):
        s = self.s
        a = (s[0] + s[3]) & M64
        r = ((((a << 23) | (a >> 41)) & M64) + s[0]) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = ((s[3] << 45) | (s[3] >> 19)) & M64
        return r

    def f32(self):
        return F32(self.next_u64() >> 40) * F32(1.0 / 16777216.0)

    def f64(self):
        return float(self.next_u64() >> 11) * (1.0 / 9007199254740992.0)

    def boolean(self):
        return (self.next_u64() >> 63) != 0


_DCTX = decimal.Context(prec=60)


def pow2(x):
    """2.0_f64.powf(x), correctly rounded."""
    if x == 0.0:
        return 1.0
    return float(_DCTX.power(decimal.Decimal(2), decimal.Decimal(float(x))))


def rem_euclid64(a, b):  # f64::rem_euclid
    r = math.fmod(a, b)
    return r + abs(b) if r < 0.0 else r


def rem_euclid32(a, b):  # f32::rem_euclid (fmod of two f32 is exact)
    r = F32(math.fmod(float(a), float(b)))
    return F32(r + abs(b)) if r < 0 else r


def fold_into_loop_range(position, loop_start, loop_end):  # granular.rs:433-440, f64
    loop_len = loop_end - loop_start
    if loop_len > 0.0:
        return loop_start + rem_euclid64(position - loop_start, loop_len)
    return loop_start


def clamp32(x, lo, hi):
    return F32(min(max(F32(x), F32(lo)), F32(hi)))


class Params:
    """GranularParameters (granular.rs:241-283) + the optional normalised loop range of the pool."""

    def __init__(self, **kw):
        self.overlap_mode = CLOUD
        self.window = 2
        self.size = 100.0
        self.density = 10.0
        self.variation = 0.0
        self.spray = 0.0
        self.pan_spread = 0.0
        self.playback_direction = FORWARD
        self.position = 0.5
        self.step = 0.0
        self.loop_range = None
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def validate(self):  # granular.rs:291-335
        ok = 1.0 <= self.size <= 1000.0 and 1.0 <= self.density <= 100.0 and 0.0 <= self.spray <= 1.0 and 0.0 <= self.variation <= 1.0
        ok = ok and 0.0 <= self.pan_spread <= 1.0 and 0.0 <= self.position <= 1.0 and -4.0 <= self.step <= 4.0
        if self.loop_range is not None:
            ok = ok and all(0.0 <= x <= 1.0 for x in self.loop_range)
        return ok


class GrainPool:
    def __init__(self, sample_rate, buffer, params, rng_state=None, speed=1.0, volume=1.0, panning=0.0):
        self.sr = int(sample_rate)
        self.buf = np.ascontiguousarray(buffer, dtype=F32)
        assert self.buf.ndim == 1 and len(self.buf) >= 1
        self.p = params
        self.loop = None if params.loop_range is None else (F32(params.loop_range[0]), F32(params.loop_range[1]))
        self.rng = Xoshiro256pp(rng_state)
        n = POOL_SIZE
        self.active = np.zeros(n, dtype=bool)
        self.volume_g = np.ones(n, dtype=F32)
        self.panning_g = np.zeros(n, dtype=F32)
        self.position = np.zeros(n, dtype=np.float64)
        self.increment = np.zeros(n, dtype=np.float64)
        self.samples_remaining = np.zeros(n, dtype=np.int64)
        self.window_phase = np.zeros(n, dtype=np.float64)
        self.window_increment = np.zeros(n, dtype=np.float64)
        self.window_mode = np.full(n, 2, dtype=np.int32)
        self.has_loop = np.zeros(n, dtype=bool)
        self.loop_start = np.zeros(n, dtype=np.float64)
        self.loop_end = np.zeros(n, dtype=np.float64)
        self.primary = -1
        self.activations = []       # (frame, slot) of every activation, frames counted from start()
        self.failed_activations = 0  # triggers that found no free slot
        self.frame = 0
        # GrainPool::start (granular.rs:474-489)
        self.trigger_new_grains = True
        self.trigger_phase = F32(1.0)
        self.speed = float(speed)
        self.volume = F32(volume)
        self.panning = F32(panning)
        self.playhead = F32(params.position)
        self.playing_loop_range = False

    # -- commands --
    def stop(self):
        self.trigger_new_grains = False

    def set_speed(self, speed):
        self.speed = float(speed)

    def set_volume(self, volume):
        self.volume = F32(volume)

    def set_panning(self, panning):
        self.panning = F32(panning)

    def is_exhausted(self):
        return (not self.trigger_new_grains) and not self.active.any()

    # -- scheduler --
    def playback_position(self):  # granular.rs:446-472, position_mod == 0
        p = self.p
        base = F32(p.position) if F32(p.step) == 0 else self.playhead
        if self.playing_loop_range and self.loop is not None:
            base = F32(fold_into_loop_range(float(base), float(self.loop[0]), float(self.loop[1])))
        return rem_euclid32(base, F32(1.0))

    def update_trigger_phase(self):  # granular.rs:788-809
        if self.p.overlap_mode == SEQUENTIAL:
            return True
        density = clamp32(F32(self.p.density) * F32(1.0), 1.0, 100.0)
        self.trigger_phase = F32(self.trigger_phase + density / F32(self.sr))
        if self.trigger_phase >= F32(1.0):
            self.trigger_phase = F32(self.trigger_phase - F32(1.0))
            return True
        return False

    def try_trigger_grain(self):  # granular.rs:524-603
        p = self.p
        if p.overlap_mode == SEQUENTIAL and self.primary >= 0 and self.active[self.primary]:
            if self.window_phase[self.primary] < float(crossfade_point(p.window)):
                return False
        if not self.trigger_new_grains or not self.update_trigger_phase():
            return False
        file_duration = float(len(self.buf)) / float(self.sr)
        modulated_spray = clamp32(F32(p.spray) + F32(0.0), 0.0, 1.0)
        spray_seconds = float(modulated_spray) * 2.0 * (self.rng.f64() - 0.5)
        spray_variation = spray_seconds / file_duration
        grain_position = float(self.playback_position()) + spray_variation
        if self.playing_loop_range and self.loop is not None:
            grain_position = fold_into_loop_range(grain_position, float(self.loop[0]), float(self.loop[1]))
        grain_position = rem_euclid64(grain_position, 1.0)
        index = self.activate_new_grain(grain_position)
        if p.overlap_mode == SEQUENTIAL and index is not None:
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
        variation = clamp32(F32(p.variation) + F32(0.0), 0.0, 1.0)
        volume_scale = F32(F32(1.0) - F32(variation * rng.f32()))
        volume = F32(self.volume * volume_scale)
        random_semitones = float(variation) * (rng.f64() - 0.5)
        speed = self.speed * pow2(random_semitones / 12.0) if random_semitones != 0.0 else self.speed
        min_scale = F32(F32(1.0) - F32(F32(0.75) * variation))
        max_scale = F32(F32(1.0) + F32(F32(2.0) * variation))
        size_scale = F32(min_scale + F32(F32(max_scale - min_scale) * rng.f32()))
        grain_size_ms = clamp32(F32(p.size) * F32(1.0), 1.0, 1000.0)
        grain_size = max(int(F32(F32(F32(grain_size_ms * size_scale) * F32(self.sr)) / F32(1000.0))), 2)
        modulated_pan_spread = clamp32(F32(p.pan_spread) + F32(0.0), 0.0, 1.0)
        panning_spread = F32(modulated_pan_spread * F32(F32(rng.f32() * F32(2.0)) - F32(1.0)))
        panning = clamp32(self.panning + panning_spread, -1.0, 1.0)
        pitch_variation_semitones = F32(F32(variation * F32(F32(rng.f32() * F32(2.0)) - F32(1.0))) * F32(0.5))
        varied_speed = speed * pow2(float(pitch_variation_semitones) / 12.0)
        if p.playback_direction == FORWARD:
            reverse = False
        elif p.playback_direction == BACKWARD:
            reverse = True
        else:
            reverse = rng.boolean()
        # Grain::activate
        self.active[index] = True
        self.window_mode[index] = p.window
        self.position[index] = min(max(position, 0.0), 1.0)
        self.volume_g[index] = clamp32(volume, 0.0, 100.0)
        self.panning_g[index] = clamp32(panning, -1.0, 1.0)
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

    def advance_playhead(self):  # granular.rs:607-640, speed_mod == 0
        step = F32(self.p.step)
        modulated_step = F32(step * F32(1.0))
        self.playhead = F32(self.playhead + modulated_step / F32(len(self.buf)))
        if self.loop is not None:
            ls, le = self.loop
            if self.playing_loop_range:
                self.playhead = F32(fold_into_loop_range(float(self.playhead), float(ls), float(le)))
            elif ls <= self.playhead < le:
                self.playing_loop_range = True
            elif self.playhead >= F32(1.0):
                self.playhead = F32(self.playhead - F32(1.0))
            elif self.playhead < F32(0.0):
                self.playhead = F32(self.playhead + F32(1.0))
        elif self.playhead >= F32(1.0):
            self.playhead = F32(self.playhead - F32(1.0))
        elif self.playhead < F32(0.0):
            self.playhead = F32(self.playhead + F32(1.0))

    # -- grains --
    def _process_grains(self):
        """Grain::process (granular.rs:1081-1120) of every active slot + sample_at_position (:901-933) + the stereo terms (:717-724)."""
        idx = np.flatnonzero(self.active)
        if len(idx) == 0:
            return np.zeros(0, F32), np.zeros(0, F32)
        t = lut()
        wph = self.window_phase[idx]
        index_float = wph * float(LUT_N - 1)
        ti = index_float.astype(np.int64) & (LUT_N - 1)
        fraction = (index_float - np.trunc(index_float)).astype(F32)
        nxt = (ti + 1) & (LUT_N - 1)
        wm = self.window_mode[idx]
        one = F32(1.0)
        env_value = np.where(ti < LUT_N - 1, t[wm, ti] * (one - fraction) + t[wm, nxt] * fraction, t[wm, LUT_N - 1]).astype(F32)
        pos32 = self.position[idx].astype(F32)
        # advance
        pos = self.position[idx] + self.increment[idx]
        self.window_phase[idx] = wph + self.window_increment[idx]
        rem = np.maximum(self.samples_remaining[idx] - 1, 0)
        self.samples_remaining[idx] = rem
        hl = self.has_loop[idx]
        ls, le = self.loop_start[idx], self.loop_end[idx]
        loop_len = le - ls
        safe_len = np.where(loop_len > 0.0, loop_len, 1.0)
        r = np.fmod(pos - ls, safe_len)
        r = np.where(r < 0.0, r + np.abs(safe_len), r)
        looped = np.where(loop_len > 0.0, ls + r, pos)
        plain = np.where(pos < 0.0, pos + 1.0, np.where(pos > 1.0, pos - 1.0, pos))
        self.position[idx] = np.where(hl, looped, plain)
        self.active[idx] = rem != 0
        envelope = (env_value * self.volume_g[idx]).astype(F32)
        pan = self.panning_g[idx]
        keep = envelope > ENVELOPE_THRESHOLD
        if not keep.any():
            return np.zeros(0, F32), np.zeros(0, F32)
        envelope, pan, pos32 = envelope[keep], pan[keep], pos32[keep]
        # sample_at_position
        n = len(self.buf)
        max_index = n - 1
        float_index = (pos32 * F32(max_index)).astype(F32)
        index = np.minimum(np.maximum(float_index, F32(0.0)).astype(np.int64), max_index)
        fr = (float_index - index.astype(F32)).astype(F32)
        i1 = index
        i2 = np.where(i1 < max_index, i1 + 1, 0)
        i0 = np.where(i1 > 0, i1 - 1, max_index)
        i3 = np.where(i2 < max_index, i2 + 1, 0)
        y0, y1, y2, y3 = self.buf[i0], self.buf[i1], self.buf[i2], self.buf[i3]
        h, h15, h25, two = F32(0.5), F32(1.5), F32(2.5), F32(2.0)
        a = ((-h * y0 + h15 * y1) - h15 * y2) + h * y3
        b = ((y0 - h25 * y1) + two * y2) - h * y3
        c = -h * y0 + h * y2
        sample = ((a * fr * fr * fr + b * fr * fr) + c * fr) + y1
        windowed = (sample * envelope).astype(F32)
        left_gain = ((one - pan) * h).astype(F32)
        right_gain = ((one + pan) * h).astype(F32)
        return (windowed * left_gain).astype(F32), (windowed * right_gain).astype(F32)

    def process(self, n_frames):
        """n_frames of GrainPool::process, stereo (granular.rs:693-727). How a render is cut into calls changes no state (the reference's cut only
        reorders active_grain_indices, which holds every active slot exactly once). Returns (out[n, 2] f32, n[n] int, S[n, 2] f64)."""
        out = np.zeros((n_frames, 2), dtype=F32)
        cnt = np.zeros(n_frames, dtype=np.int64)
        S = np.zeros((n_frames, 2), dtype=np.float64)
        move_playhead = F32(self.p.step) != 0
        with np.errstate(all="ignore"):
            for f in range(n_frames):
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

    def state(self):
        """The full state, as pg_graph_voice_grain_state reports it."""
        return {
            "trigger_phase": F32(self.trigger_phase), "playhead": F32(self.playhead), "playing_loop_range": int(self.playing_loop_range),
            "trigger_new_grains": int(self.trigger_new_grains), "primary": int(self.primary), "speed": float(self.speed),
            "volume": F32(self.volume), "panning": F32(self.panning), "rng": tuple(self.rng.s),
            "active": self.active.astype(np.int32).copy(), "samples_remaining": self.samples_remaining.copy(), "position": self.position.copy(),
            "increment": self.increment.copy(), "window_phase": self.window_phase.copy(), "window_increment": self.window_increment.copy(),
            "volume_g": self.volume_g.copy(), "panning_g": self.panning_g.copy(), "window_mode": self.window_mode.copy(),
            "has_loop": self.has_loop.astype(np.int32).copy(),
        }


def states_equal(a, b):
    """Bit-for-bit comparison of two state() dicts; returns the names of the fields that differ."""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            same = x.dtype == y.dtype and x.tobytes() == y.tobytes() if x.dtype.kind == "f" else np.array_equal(x, y)
        elif isinstance(x, (float, np.floating)):
            same = np.asarray(x).tobytes() == np.asarray(y, dtype=np.asarray(x).dtype).tobytes()
        else:
            same = x == y
        if not same:
            bad.append(k)
    return bad


def make_buffer(n=2048, seed=1):
    """The tests' source: a seeded sine plus a ramp, mono f32."""
    rng = np.random.default_rng(seed)
    f = 3.0 + 5.0 * rng.random()
    ph = rng.random()
    t = np.arange(n, dtype=np.float64) / max(n, 1)
    return (0.6 * np.sin(2.0 * np.pi * (f * t + ph)) + 0.3 * (2.0 * t - 1.0)).astype(F32)
