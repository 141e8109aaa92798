"""Independent numpy model of a granular sampler voice whose parameters and loop range change while it plays: tests/modulation_model.py's
ModGrainPool (the grain pool of tests/granular_model.py behind the modulation matrix) plus what the reference keeps apart from the parameters:
  - the pool's own overlap_mode (granular.rs:346), Cloud from GrainPool::new (:399); try_trigger_grain compares it with the parameters' and, on a
    change, takes it and forgets the primary grain (:535-538); update_trigger_phase and the primary bookkeeping read the pool's copy (:794, :596);
  - set_parameter: Sampler::set_granular_parameter (src/generator/sampler.rs:299-360) with the descriptors of :219-296 - a raw float is clamped
    to the range (parameter_update_value, :862-883), a normalized one is min + scaling.scale(n) * (max - min) (src/parameter/float.rs:137-141,
    Exponential(f) = n.powf(f), src/parameter/scaling.rs), a normalized enum (n * (count - 1)).round() (src/parameter/enum.rs:154), a raw enum the
    variant's index (one out of range is ignored);
  - set_loop_range: GrainPool::set_loop_range (granular.rs:516-518) - sample_loop_range alone changes.
Everything else is inherited: a grain keeps the window and loop range it was activated with (:823, :1038-1047), the crossfade point is the current
window's (:547), `position` places grains only while step == 0 (:448-452).

The caller cuts process() at the commands (the reference's calls are cut at its events), so GrainPool.process's `move_playhead`, read once per
call, is the step as of every frame of the call."""
import math

import numpy as np

import granular_model as gm
import modulation_model as mm

F32 = np.float32
ONE = F32(1.0)
ENUM, FLOAT = "enum", "float"
LINEAR, EXPONENTIAL = "linear", "exponential"

# Sampler::granular_parameters() (sampler.rs:219-296): id, name, type, then (min, max, default, scaling, factor) or (variant count, default index)
DESCRIPTORS = [
    ("GOVM", "Overlap Mode", ENUM, 2, 0),
    ("GWND", "Window", ENUM, 8, 0),
    ("GSIZ", "Grain Size", FLOAT, 1.0, 1000.0, 100.0, EXPONENTIAL, 2.0),
    ("GDEN", "Density", FLOAT, 1.0, 100.0, 10.0, EXPONENTIAL, 2.0),
    ("GVAR", "Variation", FLOAT, 0.0, 1.0, 0.0, LINEAR, None),
    ("GSPY", "Spray", FLOAT, 0.0, 1.0, 0.0, LINEAR, None),
    ("GPAN", "Pan Spread", FLOAT, 0.0, 1.0, 0.0, LINEAR, None),
    ("GDIR", "Direction", ENUM, 3, 0),
    ("GPOS", "Position", FLOAT, 0.0, 1.0, 0.5, LINEAR, None),
    ("GSTP", "Step", FLOAT, -4.0, 4.0, 0.0, LINEAR, None),
]
IDS = [d[0] for d in DESCRIPTORS]
FIELD = {"GOVM": "overlap_mode", "GWND": "window", "GSIZ": "size", "GDEN": "density", "GVAR": "variation", "GSPY": "spray", "GPAN": "pan_spread",
         "GDIR": "playback_direction", "GPOS": "position", "GSTP": "step"}


def descriptor(fourcc):
    for d in DESCRIPTORS:
        if d[0] == fourcc:
            return d
    raise ValueError("Invalid/unknown granular playback parameter '%s'" % fourcc)


def resolve(fourcc, value, normalized):
    """The value a ParameterValueUpdate leaves in GranularParameters: an f32 or an int; None when a raw enum index names no variant (ignored)."""
    d = descriptor(fourcc)
    value = F32(value)
    if value != value:
        raise ValueError("not a number")
    if d[2] == FLOAT:
        lo, hi = F32(d[3]), F32(d[4])
        if not normalized:
            return F32(min(max(value, lo), hi))
        n = F32(min(max(value, F32(0.0)), ONE))
        if d[6] == EXPONENTIAL:
            n = F32(float(n) ** float(d[7]))       # f32::powf(factor): for factor 2 the exact square fits a double, rounded once
        return F32(lo + F32(n * F32(hi - lo)))
    count = d[3]
    if not normalized:
        index = int(value)                          # `as usize` of the raw value
        return index if 0 <= index < count else None
    n = F32(min(max(value, F32(0.0)), ONE))
    return int(math.floor(float(F32(n * F32(count - 1))) + 0.5))   # f32::round: halves away from zero


class ParamGrainPool(mm.ModGrainPool):
    """matrix None: a matrix without routes (every sum 0.0: `x + 0.0` and `x * (1.0 + 0.0)` leave every finite x as it is)."""

    def __init__(self, sample_rate, buffer, params, matrix=None, rng_state=None, speed=1.0, volume=1.0, panning=0.0):
        super().__init__(sample_rate, buffer, params, matrix if matrix is not None else mm.Matrix(sample_rate), rng_state, speed, volume, panning)
        self.overlap_mode = gm.CLOUD      # GrainPool::new (granular.rs:399)
        self.cleared_primaries = 0        # mode changes that found an ACTIVE primary grain
        self.blocked_frames = 0           # frames at which Sequential mode held the trigger back (:549-552)
        self.blocked_past_half = 0        # ... of them, frames at which the primary's phase was at or beyond 0.5 (a window whose crossfade point lies later)
        self.rng_draws = 0                # next_u64 calls of the pool's generator
        draw = self.rng.next_u64

        def counted():
            self.rng_draws += 1
            return draw()
        self.rng.next_u64 = counted

    # -- commands --
    def set_parameter(self, fourcc, value, normalized=False, started=True):
        """Sampler::set_granular_parameter. started False: in front of the note - GrainPool::start reads the position then (:487)."""
        v = resolve(fourcc, value, normalized)
        if v is None:
            return
        setattr(self.p, FIELD[fourcc], int(v) if isinstance(v, int) else float(v))
        if fourcc == "GPOS" and not started:
            self.playhead = F32(v)

    def set_loop_range(self, loop_range):  # granular.rs:516-518
        if loop_range is not None and not all(0.0 <= float(F32(x)) <= 1.0 for x in loop_range):
            raise ValueError("Invalid loop points")
        self.p.loop_range = None if loop_range is None else (float(F32(loop_range[0])), float(F32(loop_range[1])))
        self.loop = None if loop_range is None else (F32(loop_range[0]), F32(loop_range[1]))

    # -- scheduler --
    def update_trigger_phase(self):  # granular.rs:788-809: the POOL's mode
        if self.overlap_mode == gm.SEQUENTIAL:
            return True
        density_mult = F32(ONE + self.m[mm.DENSITY])
        density = gm.clamp32(F32(F32(self.p.density) * density_mult), 1.0, 100.0)
        self.trigger_phase = F32(self.trigger_phase + F32(density / F32(self.sr)))
        if self.trigger_phase >= ONE:
            self.trigger_phase = F32(self.trigger_phase - ONE)
            return True
        return False

    def try_trigger_grain(self):  # granular.rs:524-603
        p = self.p
        if self.overlap_mode != p.overlap_mode:  # :535-538
            self.overlap_mode = p.overlap_mode
            if self.primary >= 0 and self.active[self.primary]:
                self.cleared_primaries += 1
            self.primary = -1
        if self.overlap_mode == gm.SEQUENTIAL and self.primary >= 0 and self.active[self.primary]:
            if self.window_phase[self.primary] < float(gm.crossfade_point(p.window)):
                self.blocked_frames += 1
                self.blocked_past_half += int(self.window_phase[self.primary] >= 0.5)
                return False
        if not self.trigger_new_grains or not self.update_trigger_phase():
            return False
        file_duration = float(len(self.buf)) / float(self.sr)
        modulated_spray = gm.clamp32(F32(F32(p.spray) + self.m[mm.SPRAY]), 0.0, 1.0)
        spray_seconds = float(modulated_spray) * 2.0 * (self.rng.f64() - 0.5)
        spray_variation = spray_seconds / file_duration
        grain_position = float(self.playback_position()) + spray_variation
        if self.playing_loop_range and self.loop is not None:
            grain_position = gm.fold_into_loop_range(grain_position, float(self.loop[0]), float(self.loop[1]))
        grain_position = gm.rem_euclid64(grain_position, 1.0)
        index = self.activate_new_grain(grain_position)
        if self.overlap_mode == gm.SEQUENTIAL and index is not None:
            self.primary = index
        return index is not None

    # -- read-back --
    def state(self):
        d = super().state()
        d["overlap_mode"] = int(self.overlap_mode)
        return d

    def params_state(self):
        """The parameters and the loop range as pg_graph_voice_granular_params reports them (_capi.granular_params_dict)."""
        p = self.p
        lr = self.loop
        return {"overlap_mode": int(p.overlap_mode), "window": int(p.window), "size": F32(p.size), "density": F32(p.density), "variation": F32(p.variation),
                "spray": F32(p.spray), "pan_spread": F32(p.pan_spread), "playback_direction": int(p.playback_direction), "position": F32(p.position),
                "step": F32(p.step), "has_loop_range": 0 if lr is None else 1, "loop_start": F32(0.0) if lr is None else F32(lr[0]),
                "loop_end": F32(0.0) if lr is None else F32(lr[1])}

    def windows_above_threshold(self):
        """The window modes of the active grains whose envelope at the coming frame is above ENVELOPE_THRESHOLD (a read: nothing advances)."""
        modes = set()
        for s in np.flatnonzero(self.active):
            env = F32(gm.window_sample(int(self.window_mode[s]), self.window_phase[s]) * self.volume_g[s])
            if env > gm.ENVELOPE_THRESHOLD:
                modes.add(int(self.window_mode[s]))
        return modes
