"""ctypes view of include/phonic_gpu.h: struct layouts, constants and the loader of the HIP library.

The product library (phonic_amd/csrc/libphonic_gpu.so) is built by `__graft_entry__.build()`.
Loading fails loudly when it is missing: there is no CPU fallback for the product path.
"""
import ctypes as C
import os

PG_OK, PG_ERR_PARAMETER, PG_ERR_NOT_FOUND, PG_ERR_QUEUE_FULL, PG_ERR_DEVICE, PG_ERR_STATE = range(6)

FX_GAIN, FX_PANNING, FX_FILTER, FX_EQ5, FX_DELAY, FX_REVERB, FX_CHORUS, FX_COMPRESSOR, FX_GATE, FX_DISTORTION = range(10)
FX_NAMES = ["Gain", "Panning", "Filter", "Eq5", "Delay", "Reverb", "Chorus", "Compressor", "Gate", "Distortion"]

PG_MAX_INIT_PARAMS = 16
MOVE_DIRECTION, MOVE_START, MOVE_END = 0, 1, 2  # EffectMovement (src/player.rs:75-82)
REDUCE_PEER_COPY, REDUCE_RCCL = 0, 1  # pg_sharded_set_reduce
PG_REPEAT_FOREVER = 2**64 - 1
INT64_MAX = 2**63 - 1


def fourcc(s):
    """FourCC(*b"room") -> u32 (big endian, as in include/phonic_gpu.h PG_FOURCC)."""
    b = s.encode() if isinstance(s, str) else bytes(s)
    assert len(b) == 4, s
    return b[0] << 24 | b[1] << 16 | b[2] << 8 | b[3]


class EffectInit(C.Structure):
    _fields_ = [
        ("n_params", C.c_uint32),
        ("fourcc", C.c_uint32 * PG_MAX_INIT_PARAMS),
        ("value", C.c_float * PG_MAX_INIT_PARAMS),
        ("has_reverb_seeds", C.c_uint32),
        ("reverb_fpd_l", C.c_uint32),
        ("reverb_fpd_r", C.c_uint32),
        ("reverb_vib_phase", C.c_double * 16),
        ("has_lfo_seed", C.c_uint32),
        ("reserved_lfo", C.c_uint32),
        ("lfo_rng_state", C.c_uint64 * 4),
    ]


class VoiceOptions(C.Structure):
    _fields_ = [
        ("volume", C.c_float),
        ("panning", C.c_float),
        ("speed", C.c_double),
        ("repeat", C.c_uint64),
        ("has_repeat", C.c_uint32),
        ("has_loop_range", C.c_uint32),
        ("loop_start", C.c_uint64),
        ("loop_end", C.c_uint64),
        ("start_time", C.c_uint64),
        ("fade_in_seconds", C.c_float),
        ("fade_out_seconds", C.c_float),
        ("source_rate", C.c_uint32),
        ("non_transient", C.c_uint32),
    ]


class ParamDesc(C.Structure):
    _fields_ = [
        ("fourcc", C.c_uint32),
        ("type", C.c_int32),
        ("min", C.c_float),
        ("max", C.c_float),
        ("default_value", C.c_float),
        ("scaling", C.c_int32),
        ("scaling_arg0", C.c_float),
        ("scaling_arg1", C.c_float),
        ("n_values", C.c_int32),
        ("name", C.c_char_p),
    ]


class AhdsrParams(C.Structure):
    """pg_ahdsr_params: AhdsrParameters::new_with_scaling's arguments, times as f32 seconds."""
    _fields_ = [(n, C.c_float) for n in ("attack_s", "attack_scaling", "hold_s", "decay_s", "decay_scaling", "sustain_level", "release_s", "release_scaling")]


class AudioLevel(C.Structure):
    """pg_audio_level: AudioLevel (reference src/source/metered.rs), linear peak and RMS per channel."""
    _fields_ = [("peak", C.c_float * 2), ("rms", C.c_float * 2)]


class StatusEvent(C.Structure):
    """pg_status_event: one PlaybackStatusEvent (reference src/source/status.rs) as the device decided it — Position or Stopped { exhausted }."""
    _fields_ = [("kind", C.c_int32), ("voice_id", C.c_int32), ("sample_time", C.c_uint64), ("frame_pos", C.c_uint64), ("position_seconds", C.c_double),
                ("exhausted", C.c_int32), ("reserved", C.c_int32)]


PG_STATUS_POSITION, PG_STATUS_STOPPED = 0, 1


def status_tuple(e):
    """A pg_status_event as a plain tuple: ("position", voice, sample_time, frame_pos, position_seconds) or ("stopped", voice, sample_time, exhausted)."""
    if e.kind == PG_STATUS_POSITION:
        return ("position", int(e.voice_id), int(e.sample_time), int(e.frame_pos), float(e.position_seconds))
    return ("stopped", int(e.voice_id), int(e.sample_time), bool(e.exhausted))


def _db(x):
    import math

    return 20.0 * math.log10(x) if x > 0.0 else float("-inf")


class Level:
    """What Player::audio_level / MixerHandle::audio_level return: per-channel `peak` and `rms` (linear, exactly the f32 values the meter
    published) plus `peak_db` / `rms_db` as AudioLevel::peak_db does: 20 log10, -inf at 0."""

    def __init__(self, raw):
        self.peak = (float(raw.peak[0]), float(raw.peak[1]))
        self.rms = (float(raw.rms[0]), float(raw.rms[1]))
        self.peak_db = tuple(_db(x) for x in self.peak)
        self.rms_db = tuple(_db(x) for x in self.rms)

    def __eq__(self, other):
        return isinstance(other, Level) and self.peak == other.peak and self.rms == other.rms

    def __repr__(self):
        return f"Level(peak={self.peak}, rms={self.rms})"


def ahdsr_params(**kw):
    """AhdsrParameters::default() (reference src/utils/ahdsr.rs:348-359) with overrides."""
    p = AhdsrParams(0.010, 0.0, 1.0, 0.5, 0.0, 0.75, 1.0, 0.0)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, float(v))
    return p


class GranularParams(C.Structure):
    """pg_granular_params: GranularParameters (reference src/generator/sampler/granular.rs:241-266) + the pool's normalised loop range + the
    Xoshiro256++ state of its SmallRng."""
    _fields_ = [("overlap_mode", C.c_int32), ("window", C.c_int32), ("size", C.c_float), ("density", C.c_float), ("variation", C.c_float), ("spray", C.c_float),
                ("pan_spread", C.c_float), ("playback_direction", C.c_int32), ("position", C.c_float), ("step", C.c_float), ("has_loop_range", C.c_int32),
                ("loop_start", C.c_float), ("loop_end", C.c_float), ("reserved", C.c_int32), ("rng_state", C.c_uint64 * 4)]


GRAIN_POOL_SIZE = 100
GRAIN_CLOUD, GRAIN_SEQUENTIAL = 0, 1
GRAIN_FORWARD, GRAIN_BACKWARD, GRAIN_RANDOM = 0, 1, 2
GRAIN_WINDOWS = ("Hann", "Blackman", "Triangle", "Tukey", "Trapezoid", "Exponential", "RampUp", "RampDown")


def granular_params(loop_range=None, rng_state=None, **kw):
    """GranularParameters::default() (granular.rs:268-283) with overrides; loop_range = (start, end) normalised; rng_state = four u64."""
    p = GranularParams()
    load().pg_granular_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in ("overlap_mode", "window", "size", "density", "variation", "spray", "pan_spread", "playback_direction", "position", "step"):
            raise AttributeError(k)
        setattr(p, k, int(v) if k in ("overlap_mode", "window", "playback_direction") else float(v))
    if loop_range is not None:
        p.has_loop_range, p.loop_start, p.loop_end = 1, float(loop_range[0]), float(loop_range[1])
    if rng_state is not None:
        for i in range(4):
            p.rng_state[i] = int(rng_state[i])
    return p


class GrainSlot(C.Structure):
    """pg_grain_slot: Grain (granular.rs:961-985)."""
    _fields_ = [("position", C.c_double), ("increment", C.c_double), ("window_phase", C.c_double), ("window_increment", C.c_double), ("samples_remaining", C.c_uint64),
                ("volume", C.c_float), ("panning", C.c_float), ("active", C.c_int32), ("window_mode", C.c_int32), ("has_loop_range", C.c_int32), ("reserved", C.c_int32)]


class GrainState(C.Structure):
    """pg_grain_state: the GrainPool's scalars and its 100 grains."""
    _fields_ = [("trigger_phase", C.c_float), ("playhead", C.c_float), ("playing_loop_range", C.c_int32), ("trigger_new_grains", C.c_int32), ("primary_slot", C.c_int32),
                ("overlap_mode", C.c_int32), ("speed", C.c_double), ("volume", C.c_float), ("panning", C.c_float), ("rng_state", C.c_uint64 * 4), ("slots", GrainSlot * GRAIN_POOL_SIZE)]


def grain_state_dict(st):
    """A GrainState as numpy arrays / scalars (the layout tests/granular_model.py's GrainPool.state() uses)."""
    import numpy as np

    slots = st.slots
    col = lambda name, dt: np.array([getattr(slots[i], name) for i in range(GRAIN_POOL_SIZE)], dtype=dt)
    return {
        "trigger_phase": np.float32(st.trigger_phase), "playhead": np.float32(st.playhead), "playing_loop_range": int(st.playing_loop_range),
        "trigger_new_grains": int(st.trigger_new_grains), "primary": int(st.primary_slot), "speed": float(st.speed), "volume": np.float32(st.volume),
        "panning": np.float32(st.panning), "rng": tuple(int(x) for x in st.rng_state),
        "active": col("active", np.int32), "samples_remaining": col("samples_remaining", np.int64), "position": col("position", np.float64),
        "increment": col("increment", np.float64), "window_phase": col("window_phase", np.float64), "window_increment": col("window_increment", np.float64),
        "volume_g": col("volume", np.float32), "panning_g": col("panning", np.float32), "window_mode": col("window_mode", np.int32),
        "has_loop": col("has_loop_range", np.int32), "overlap_mode": int(st.overlap_mode),
    }


GRANULAR_PARAM_IDS = ("GOVM", "GWND", "GSIZ", "GDEN", "GVAR", "GSPY", "GPAN", "GDIR", "GPOS", "GSTP")   # Sampler::granular_parameters() (sampler.rs:283-296)


def granular_param_descs():
    """The ten descriptors of pg_granular_param as dicts, in Sampler::granular_parameters() order. No device."""
    lib = load()
    out = []
    for i in range(lib.pg_granular_param_count()):
        d = ParamDesc()
        if lib.pg_granular_param(i, C.byref(d)) != 0:
            raise RuntimeError((lib.pg_last_error_message() or b"").decode())
        out.append({"id": d.fourcc.to_bytes(4, "big").decode(), "name": d.name.decode(), "type": int(d.type), "min": float(d.min), "max": float(d.max),
                    "default": float(d.default_value), "scaling": int(d.scaling), "scaling_arg0": float(d.scaling_arg0), "n_values": int(d.n_values)})
    return out


def granular_params_dict(p):
    """A GranularParams read back with pg_graph_voice_granular_params as numpy scalars (the layout tests/granular_params_model.py's params_state() uses)."""
    import numpy as np

    return {"overlap_mode": int(p.overlap_mode), "window": int(p.window), "size": np.float32(p.size), "density": np.float32(p.density), "variation": np.float32(p.variation),
            "spray": np.float32(p.spray), "pan_spread": np.float32(p.pan_spread), "playback_direction": int(p.playback_direction), "position": np.float32(p.position),
            "step": np.float32(p.step), "has_loop_range": int(p.has_loop_range), "loop_start": np.float32(p.loop_start), "loop_end": np.float32(p.loop_end)}


MOD_SOURCES, MOD_TARGETS = 4, 7
MOD_SOURCE_NAMES = ("LFO1", "LFO2", "VELM", "KEYM")                                         # the matrix's slot order (sampler.rs:362-416)
MOD_TARGET_NAMES = ("size", "density", "variation", "spray", "pan_spread", "position", "step")   # Sampler::modulation_config's order (sampler.rs:417-425)
LFO_WAVEFORMS = ("Sine", "Triangle", "RampUp", "RampDown", "Square", "Random", "SmoothRandom")   # LfoWaveform (utils/dsp/lfo.rs:35-47)


class ModLfo(C.Structure):
    """pg_mod_lfo: rate, waveform and the Xoshiro256++ state of one of the matrix's LFOs."""
    _fields_ = [("rate_hz", C.c_float), ("waveform", C.c_int32), ("rng_state", C.c_uint64 * 4)]


class ModRoute(C.Structure):
    """pg_mod_route: ModulationProcessorTarget's amount and polarity; amount 0 = no route."""
    _fields_ = [("amount", C.c_float), ("bipolar", C.c_int32)]


class ModulationParams(C.Structure):
    """pg_modulation_params: the ModulationMatrix of a granular sampler voice as the note starts (src/generator/sampler/modulation.rs)."""
    _fields_ = [("lfo", ModLfo * 2), ("velocity", C.c_float), ("note", C.c_int32), ("routes", (ModRoute * MOD_TARGETS) * MOD_SOURCES)]


class ModLfoState(C.Structure):
    _fields_ = [("phase", C.c_float), ("phase_inc", C.c_float), ("sample_hold", C.c_float), ("jitter_current", C.c_float), ("jitter_target", C.c_float),
                ("waveform", C.c_int32), ("rng_state", C.c_uint64 * 4)]


class ModulationState(C.Structure):
    """pg_modulation_state: debug read-back of the matrix."""
    _fields_ = [("lfo", ModLfoState * 2), ("velocity", C.c_float), ("note_pitch", C.c_float), ("routes", (ModRoute * MOD_TARGETS) * MOD_SOURCES),
                ("last", C.c_float * MOD_TARGETS), ("reserved", C.c_int32)]


def modulation_params(rates=None, waveforms=None, rng_states=None, velocity=None, note=None, routes=()):
    """pg_modulation_params_default() with overrides: rates / waveforms / rng_states per LFO (None: keep), routes = (source, target, amount, bipolar)."""
    p = ModulationParams()
    load().pg_modulation_params_default(C.byref(p))
    for l in range(2):
        if rates is not None and rates[l] is not None:
            p.lfo[l].rate_hz = float(rates[l])
        if waveforms is not None and waveforms[l] is not None:
            p.lfo[l].waveform = int(waveforms[l])
        if rng_states is not None and rng_states[l] is not None:
            for i in range(4):
                p.lfo[l].rng_state[i] = int(rng_states[l][i])
    if velocity is not None:
        p.velocity = float(velocity)
    if note is not None:
        p.note = int(note)
    for (s, t, amount, bipolar) in routes:
        p.routes[s][t].amount, p.routes[s][t].bipolar = float(amount), 1 if bipolar else 0
    return p


def modulation_state_dict(st):
    """A ModulationState as numpy scalars / arrays (the layout tests/modulation_model.py's Matrix.state() uses)."""
    import numpy as np

    d = {"velocity": np.float32(st.velocity), "note_pitch": np.float32(st.note_pitch),
         "amount": np.array([[st.routes[s][t].amount for t in range(MOD_TARGETS)] for s in range(MOD_SOURCES)], dtype=np.float32),
         "bipolar": np.array([[st.routes[s][t].bipolar for t in range(MOD_TARGETS)] for s in range(MOD_SOURCES)], dtype=np.int32),
         "last": np.array(list(st.last), dtype=np.float32)}
    for l in range(2):
        o = st.lfo[l]
        for k in ("phase", "phase_inc", "sample_hold", "jitter_current", "jitter_target"):
            d[f"lfo{l}_{k}"] = np.float32(getattr(o, k))
        d[f"lfo{l}_waveform"] = int(o.waveform)
        d[f"lfo{l}_rng"] = tuple(int(x) for x in o.rng_state)
    return d


class SampleBufferDesc(C.Structure):
    """pg_sample_buffer_desc: AudioFileBuffer (reference src/source/file/buffer.rs) — channels, rate, the file's embedded loop range in source frames."""
    _fields_ = [("channels", C.c_uint32), ("rate", C.c_uint32), ("has_loop_range", C.c_uint32), ("reserved", C.c_uint32), ("loop_start", C.c_uint64), ("loop_end", C.c_uint64)]


class SampleBufferInfo(C.Structure):
    """pg_sample_buffer_info"""
    _fields_ = [("n_frames", C.c_uint64), ("channels", C.c_uint32), ("rate", C.c_uint32), ("has_loop_range", C.c_uint32), ("use_count", C.c_int32),
                ("loop_start", C.c_uint64), ("loop_end", C.c_uint64), ("granular_frames", C.c_int64)]


class WaveformPoint(C.Structure):
    """pg_waveform_point: waveform::Point (reference src/utils/waveform.rs:73-81) — `frame` inside the slice, `time` = frame as f32 / rate as f32."""
    _fields_ = [("frame", C.c_uint64), ("time", C.c_float), ("min", C.c_float), ("max", C.c_float), ("reserved", C.c_uint32)]


PG_WAVEFORM_MIXED_DOWN, PG_WAVEFORM_MULTI_CHANNEL = 0, 1   # waveform::mixed_down / multi_channel
PG_WAVEFORM_OF_FILE, PG_WAVEFORM_OF_GRANULAR = 0, 1        # the buffer as uploaded / its granular mono buffer at the graph's rate


def sample_buffer_desc(channels, rate, loop_range=None):
    """loop_range = (start, end) in source frames: the file's embedded loop, or None."""
    d = SampleBufferDesc(channels=channels, rate=rate)
    if loop_range is not None:
        d.has_loop_range, d.loop_start, d.loop_end = 1, int(loop_range[0]), int(loop_range[1])
    return d


def sample_buffer_info_dict(info):
    return dict(n_frames=info.n_frames, channels=info.channels, rate=info.rate, loop_range=(info.loop_start, info.loop_end) if info.has_loop_range else None,
                use_count=info.use_count, granular_frames=info.granular_frames)


def mono_downmix(pcm, channels):
    """The down-mix of Sampler::create_granular_sample_buffer (sampler.rs:940-943) for a buffer that is already at the graph's rate: per frame, the f32
    sum of the channels in order, divided by the channel count."""
    import numpy as np

    pcm = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1, channels)
    if channels == 1:
        return pcm.reshape(-1).copy()
    acc = np.zeros(pcm.shape[0], dtype=np.float32)
    for c in range(channels):
        acc = (acc + pcm[:, c]).astype(np.float32)
    return (acc / np.float32(channels)).astype(np.float32)


PG_SAMPLER_MAX_VOICES = 64
SAMPLER_PARAM_IDS = ("STRN", "SFTN", "SVOL", "SPAN")   # Sampler::base_parameters() order (reference src/generator/sampler.rs:120-127)
UINT64_MAX = 2**64 - 1


class SamplerOptions(C.Structure):
    """pg_sampler_options: voice count, Sampler::with_ahdsr, Sampler::set_loop_range before playback, play_generator / add_generator, start time."""
    _fields_ = [("voice_count", C.c_uint32), ("has_envelope", C.c_uint32), ("envelope", AhdsrParams), ("has_loop_range", C.c_uint32), ("transient", C.c_uint32),
                ("loop_start", C.c_uint64), ("loop_end", C.c_uint64), ("start_time", C.c_uint64)]


class SamplerSlotState(C.Structure):
    """pg_sampler_slot_state"""
    _fields_ = [("note_id", C.c_int64), ("release_start_frame", C.c_uint64), ("note_volume", C.c_float), ("note_panning", C.c_float), ("note", C.c_int32),
                ("envelope_stage", C.c_int32)]


class SamplerState(C.Structure):
    """pg_sampler_state"""
    _fields_ = [("voice_count", C.c_int32), ("active_voices", C.c_int32), ("stopping", C.c_int32), ("stopped", C.c_int32), ("transpose", C.c_int32),
                ("finetune", C.c_int32), ("volume", C.c_float), ("panning", C.c_float), ("slots", SamplerSlotState * PG_SAMPLER_MAX_VOICES)]


def sampler_options(voice_count=8, envelope=None, loop_range=None, transient=False, start_time=0):
    """pg_sampler_options_default with overrides. envelope: an AhdsrParams, a dict of overrides of AhdsrParameters::default(), or None; loop_range:
    (start, end) in source frames, or None."""
    o = SamplerOptions(voice_count=int(voice_count), transient=1 if transient else 0, start_time=int(start_time))
    o.envelope = ahdsr_params()
    if envelope is not None:
        o.has_envelope = 1
        o.envelope = envelope if isinstance(envelope, AhdsrParams) else ahdsr_params(**envelope)
    if loop_range is not None:
        o.has_loop_range, o.loop_start, o.loop_end = 1, int(loop_range[0]), int(loop_range[1])
    return o


def sampler_state_dict(st):
    """A pg_sampler_state as plain values: the sampler's fields and `slots`, one dict per slot of the pool (release_start_frame None = none)."""
    slots = []
    for k in range(st.voice_count):
        s = st.slots[k]
        import numpy as np

        slots.append(dict(note_id=int(s.note_id), note=int(s.note), note_volume=np.float32(s.note_volume), note_panning=np.float32(s.note_panning),
                          envelope_stage=int(s.envelope_stage), release_start_frame=None if s.release_start_frame == UINT64_MAX else int(s.release_start_frame)))
    import numpy as np

    return dict(voice_count=int(st.voice_count), active_voices=int(st.active_voices), stopping=bool(st.stopping), stopped=bool(st.stopped), transpose=int(st.transpose),
                finetune=int(st.finetune), volume=np.float32(st.volume), panning=np.float32(st.panning), slots=slots)


SAMPLER_ENVELOPE_PARAM_IDS = ("AATK", "AHLD", "ADCY", "ASTN", "AREL")   # Sampler::envelope_parameters() order (reference src/generator/sampler.rs:173-181)
ENV_HOLD_ZERO, ENV_DECAY_ZERO, ENV_RELEASE_ZERO = 1, 2, 4                # pg_sampler_envelope_state.zero_times


class SamplerEnvelopeState(C.Structure):
    """pg_sampler_envelope_state: a sampler's AhdsrParameters as the device holds them (rates per frame; a zero time is a rate of f32::MAX)."""
    _fields_ = [("attack_rate", C.c_float), ("decay_rate", C.c_float), ("release_rate", C.c_float), ("sustain_level", C.c_float), ("hold_samples", C.c_float),
                ("attack_scaling", C.c_float), ("decay_scaling", C.c_float), ("release_scaling", C.c_float), ("zero_times", C.c_int32)]


def sampler_envelope_state_dict(st):
    """A SamplerEnvelopeState as numpy scalars."""
    import numpy as np

    d = {k: np.float32(getattr(st, k)) for k, _ in SamplerEnvelopeState._fields_[:-1]}
    d["zero_times"] = int(st.zero_times)
    return d


class GeneratorOptions(C.Structure):
    """pg_generator_options: GeneratorPlaybackOptions::volume / ::panning of a sampler on the main mixer."""
    _fields_ = [("volume", C.c_float), ("panning", C.c_float)]


class SamplerOutputState(C.Structure):
    """pg_sampler_output_state: the two smoothers of a main-mixer sampler's output stage."""
    _fields_ = [("volume_current", C.c_float), ("volume_target", C.c_float), ("panning_current", C.c_float), ("panning_target", C.c_float),
                ("volume_ramping", C.c_int32), ("panning_ramping", C.c_int32)]


def generator_options(volume=None, panning=None):
    """pg_generator_options_default with overrides."""
    o = GeneratorOptions()
    load().pg_generator_options_default(C.byref(o))
    if volume is not None:
        o.volume = volume
    if panning is not None:
        o.panning = panning
    return o


def sampler_output_state_dict(st):
    """A pg_sampler_output_state as plain values (f32 values, booleans)."""
    import numpy as np

    d = {k: np.float32(getattr(st, k)) for k in ("volume_current", "volume_target", "panning_current", "panning_target")}
    d["volume_ramping"], d["panning_ramping"] = bool(st.volume_ramping), bool(st.panning_ramping)
    return d


class GranularSamplerOptions(C.Structure):
    """pg_granular_sampler_options: the GranularParameters of Sampler::with_granular_playback, an optional matrix for every slot, an optional table
    of Xoshiro256++ states (voice_count x 3 x 4 words: slot k's pool, LFO 1, LFO 2)."""
    _fields_ = [("params", GranularParams), ("modulation", C.POINTER(ModulationParams)), ("rng_states", C.POINTER(C.c_uint64))]


def granular_sampler_options(params=None, modulation=None, rng_states=None):
    """pg_granular_sampler_options_default with overrides. params: a GranularParams; modulation: a ModulationParams or None; rng_states: None, or
    per slot three states of four u64 (pool, LFO 1, LFO 2). The returned struct keeps what it points to alive."""
    o = GranularSamplerOptions()
    load().pg_granular_sampler_options_default(C.byref(o))
    if params is not None:
        o.params = params
    if modulation is not None:
        o._modulation = modulation
        o.modulation = C.pointer(modulation)
    if rng_states is not None:
        flat = [int(w) & (2**64 - 1) for slot in rng_states for gen in slot for w in gen]
        o._rng_states = (C.c_uint64 * len(flat))(*flat)
        o.rng_states = C.cast(o._rng_states, C.POINTER(C.c_uint64))
    return o


def granular_sampler_rng_state(given, slot, generator):
    """pg_granular_sampler_rng_state: the state slot `slot`'s generator (0 pool, 1 LFO 1, 2 LFO 2) gets without an explicit table. No device."""
    g = (C.c_uint64 * 4)(*[int(x) & (2**64 - 1) for x in (given if given is not None else (0, 0, 0, 0))])
    out = (C.c_uint64 * 4)()
    load().pg_granular_sampler_rng_state(g, int(slot), int(generator), out)
    return tuple(int(x) for x in out)


def make_init(params=None, reverb_seeds=None, lfo_seed=None):
    """Build a pg_effect_init. params: dict {fourcc-str: raw value}; reverb_seeds: (fpd_l, fpd_r, [16 phases]); lfo_seed: the four u64 of the
    Delay LFO's Xoshiro256++ state (Random / Smooth Random shapes)."""
    init = EffectInit()
    params = params or {}
    assert len(params) <= PG_MAX_INIT_PARAMS
    init.n_params = len(params)
    for i, (k, v) in enumerate(params.items()):
        init.fourcc[i] = fourcc(k)
        init.value[i] = float(v)
    if reverb_seeds is not None:
        init.has_reverb_seeds = 1
        init.reverb_fpd_l, init.reverb_fpd_r = int(reverb_seeds[0]), int(reverb_seeds[1])
        for i in range(16):
            init.reverb_vib_phase[i] = float(reverb_seeds[2][i])
    if lfo_seed is not None:
        init.has_lfo_seed = 1
        for i in range(4):
            init.lfo_rng_state[i] = int(lfo_seed[i]) & (2**64 - 1)
    return init


def default_voice_options(**kw):
    """FilePlaybackOptions::default() (reference src/source/file.rs:94-112)."""
    o = VoiceOptions()
    o.volume, o.panning, o.speed = 1.0, 0.0, 1.0
    o.repeat, o.has_repeat, o.has_loop_range = 0, 0, 0
    o.loop_start = o.loop_end = 0
    o.start_time = 0
    o.fade_in_seconds, o.fade_out_seconds = 0.0, 0.05
    o.source_rate, o.non_transient = 0, 0
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


_P, _vp, _int, _u32, _u64, _sz, _f32, _f64 = C.POINTER, C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float, C.c_double

# `dyn Effect`: (name behind "<prefix>effect_", restype, argument types behind the handle)
EFFECT_CALLS = (
    ("initialize", _int, [_u32, _sz, _sz]),
    ("process", _int, [_P(_f32), _sz, _u64]),
    ("tail", C.c_int64, []),
    ("set_parameter", _int, [_u32, _f32, _int]),
    ("message_reset", _int, []),
    ("destroy", None, []),
)

# The main mixer's calls, the same on every handle: (name, restype, argument types behind the handle) of pg_graph_<name> and pg_sharded_<name>
# (and, through declare(), of the test oracle's graph calls of the same names, for the ones it has). A call that exists on both handles is
# declared here and nowhere else.
MIXER_CALLS = (
    ("add_mixer", _int, []),
    ("add_mixer_to", _int, [_int]),
    ("add_effect", _int, [_int, _int, _P(EffectInit)]),
    ("add_voice", _int, [_int, _P(_f32), _sz, _u32, _u32, _P(VoiceOptions)]),
    ("schedule_param", _int, [_int, _u32, _f32, _int, _u64]),
    ("schedule_reset", _int, [_int, _u64]),
    ("remove_effect", _int, [_int]),
    ("remove_mixer", _int, [_int]),
    ("stop_all_voices", _int, []),
    ("move_effect", _int, [_int, _int, _int, _int]),
    ("set_voice_volume", _int, [_int, _f32, _u64]),
    ("set_voice_panning", _int, [_int, _f32, _u64]),
    ("stop_voice", _int, [_int, _u64]),
    ("remove_voice", _int, [_int]),
    ("set_voice_speed", _int, [_int, _f64, _f32, _u64]),
    ("seek_voice", _int, [_int, _f64, _u64]),
    ("write", _sz, [_P(_f32), _sz, _u64]),
    ("is_voice_playing", _int, [_int]),
    ("synchronize", _int, []),
    ("device_errors", _int, []),
    ("set_max_blocks_per_launch", _int, [_int]),
    # host-fed sources
    ("add_stream_voice", _int, [_int, _u32, _u32, _sz, _P(VoiceOptions)]),
    ("feed_voice", _int, [_int, _P(_f32), _sz]),
    ("end_stream_voice", _int, [_int]),
    ("stream_voice_consumed", C.c_int64, [_int]),
    # envelopes
    ("set_voice_envelope", _int, [_int, _P(AhdsrParams)]),
    ("release_voice", _int, [_int, _u64]),
    ("voice_envelope_stage", _int, [_int]),
    # metering
    ("set_metering", _int, [_f64]),
    ("mixer_audio_level", _int, [_int, _P(AudioLevel)]),
    # playback status
    ("enable_status", _int, [_sz]),
    ("set_voice_status", _int, [_int, _f64, _int]),
    ("poll_status", _int, [_P(StatusEvent), _sz]),
    ("status_dropped", _u64, []),
    # granular voices, their parameters and their modulation matrix
    ("add_granular_voice", _int, [_int, _P(_f32), _sz, _P(GranularParams), _P(VoiceOptions)]),
    ("voice_grain_state", _int, [_int, _P(GrainState)]),
    ("set_voice_granular_parameter", _int, [_int, _u32, _f32, _int, _u64]),
    ("set_voice_grain_loop_range", _int, [_int, _int, _f32, _f32, _u64]),
    ("voice_granular_params", _int, [_int, _P(GranularParams)]),
    ("set_voice_modulation_matrix", _int, [_int, _P(ModulationParams)]),
    ("set_voice_modulation", _int, [_int, _int, _int, _f32, _int, _u64]),
    ("clear_voice_modulation", _int, [_int, _int, _int, _u64]),
    ("set_voice_lfo_rate", _int, [_int, _int, _f32, _u64]),
    ("set_voice_lfo_waveform", _int, [_int, _int, _int, _u64]),
    ("voice_modulation_state", _int, [_int, _P(ModulationState)]),
    # sample buffers (read_granular_buffer: below, the one call whose arguments differ between the handles)
    ("add_sample_buffer", _int, [_P(_f32), _sz, _P(SampleBufferDesc)]),
    ("release_sample_buffer", _int, [_int]),
    ("add_voice_from_buffer", _int, [_int, _int, _P(VoiceOptions)]),
    ("add_granular_voice_from_buffer", _int, [_int, _int, _P(GranularParams), _P(VoiceOptions)]),
    ("prepare_granular_buffer", _int, [_int]),
    ("sample_buffer_info", _int, [_int, _P(SampleBufferInfo)]),
)

# what only the plain graph has (argument types behind the handle)
GRAPH_ONLY_CALLS = (
    ("read_granular_buffer", C.c_int64, [_int, _P(_f32), _sz]),
    ("sample_buffer_waveform", C.c_int64, [_int, _int, _int, _u64, _u64, _u32, _P(WaveformPoint), _sz]),   # (buffer, source, mode, first frame, frames, resolution, out, capacity)
    ("write_device", _sz, [_vp, _sz, _u64, _vp]),
    ("set_defer_bus", _int, [_int]),
    ("process_bus_device", _int, [_vp, _sz, _u64, _vp]),
    ("process_bus_device_flags", _int, [_vp, _sz, _u64, _vp, _vp, _int]),
    ("export_audible", _int, [_vp, _int, _vp]),
    ("audible_words", _int, []),
    ("next_main_event", _u64, [_u64]),
    ("voice_count", _int, []),
    ("deferred_units", _int, []),
    ("kernel_ms", _f64, [_int, _P(_u64)]),
    ("kernel_stats", _int, [_int, _P(_f64), _P(_u64), _P(_u64)]),
    ("bus_kernel_stats", _int, [_int, _P(_f64), _P(_u64), _P(_u64)]),
    ("dynamic_stats", _int, [_int, _P(_u64), _P(_f64), _P(_u64)]),
    ("bus_kernel", C.c_char_p, []),
    ("dominant_kernel", C.c_char_p, []),
    ("set_fast_math", _int, [_int]),
    ("set_timing_period", _int, [_int]),
    ("set_staged", _int, [_int]),
    # samplers: the note layer (the sharded handle has none yet)
    ("add_sampler", _int, [_int, _int, _P(SamplerOptions)]),
    ("remove_sampler", _int, [_int]),
    ("sampler_note_on", C.c_int64, [_int, C.c_uint8, _f32, _f32, _u64]),
    ("sampler_note_off", _int, [_int, C.c_int64, _u64]),
    ("sampler_all_notes_off", _int, [_int, _u64]),
    ("sampler_set_note_speed", _int, [_int, C.c_int64, _f64, _f32, _u64]),
    ("sampler_set_note_volume", _int, [_int, C.c_int64, _f32, _u64]),
    ("sampler_set_note_panning", _int, [_int, C.c_int64, _f32, _u64]),
    ("sampler_set_parameter", _int, [_int, _u32, _f32, _int, _u64]),
    ("sampler_stop", _int, [_int, _u64]),
    ("sampler_state", _int, [_int, _P(SamplerState)]),
    # granular-mode samplers
    ("add_granular_sampler", _int, [_int, _int, _P(SamplerOptions), _P(GranularSamplerOptions)]),
    ("sampler_set_granular_parameter", _int, [_int, _u32, _f32, _int, _u64]),
    ("sampler_voice_grain_state", _int, [_int, _int, _P(GrainState)]),
    ("sampler_voice_modulation_state", _int, [_int, _int, _P(ModulationState)]),
    ("sampler_granular_params", _int, [_int, _P(GranularParams)]),
    # what changes every voice of a pool while notes sound: the envelope's knobs, the matrix, the loop range
    ("sampler_set_envelope_parameter", _int, [_int, _u32, _f32, _int, _u64]),
    ("sampler_envelope_params", _int, [_int, _int, _P(SamplerEnvelopeState)]),
    ("sampler_set_modulation", _int, [_int, _int, _int, _f32, _int, _u64]),
    ("sampler_clear_modulation", _int, [_int, _int, _int, _u64]),
    ("sampler_set_lfo_rate", _int, [_int, _int, _f32, _u64]),
    ("sampler_set_lfo_waveform", _int, [_int, _int, _int, _u64]),
    ("sampler_set_loop_range", _int, [_int, _int, _u64, _u64, _u64]),
    # samplers on the main mixer, with the generator's volume and panning
    ("add_sampler_to_main", _int, [_int, _P(SamplerOptions), _P(GeneratorOptions)]),
    ("add_granular_sampler_to_main", _int, [_int, _P(SamplerOptions), _P(GranularSamplerOptions), _P(GeneratorOptions)]),
    ("sampler_set_volume", _int, [_int, _f32, _u64]),
    ("sampler_set_panning", _int, [_int, _f32, _u64]),
    ("sampler_output_state", _int, [_int, _P(SamplerOutputState)]),
)

# what only the sharded handle has (pg_sharded_create and _destroy: in load)
SHARDED_ONLY_CALLS = (
    ("read_granular_buffer", C.c_int64, [_int, _int, _P(_f32), _sz]),   # (buffer, shard, out, capacity)
    ("write_device", _sz, [_vp, _sz, _u64]),
    ("shard_count", _int, []),
    ("shard_of_mixer", _int, [_int]),
    ("set_reduce", _int, [_int]),
    ("reduce_mode", _int, []),
)

# calls without a handle: (full name, restype, argument types)
PLAIN_CALLS = (
    ("pg_last_error_message", C.c_char_p, []),
    ("pg_device_count", _int, []),
    ("pg_effect_create", _vp, [_int, _P(EffectInit), _int]),
    ("pg_effect_debug_index_log", _int, [_vp, _P(C.c_int32), _sz]),
    ("pg_effect_process_started", _int, [_vp]),
    ("pg_effect_process_stopped", _int, [_vp]),
    ("pg_effect_kind_name", C.c_char_p, [_int]),
    ("pg_effect_kind_weight", _int, [_int]),
    ("pg_effect_kind_param_count", _int, [_int]),
    ("pg_effect_kind_param", _int, [_int, _int, _P(ParamDesc)]),
    ("pg_voice_options_default", None, [_P(VoiceOptions)]),
    ("pg_ahdsr_params_default", None, [_P(AhdsrParams)]),
    ("pg_granular_params_default", None, [_P(GranularParams)]),
    ("pg_granular_params_check", _int, [_P(GranularParams)]),
    ("pg_granular_param_count", _int, []),
    ("pg_granular_param", _int, [_int, _P(ParamDesc)]),
    ("pg_sampler_options_default", None, [_P(SamplerOptions)]),
    ("pg_sampler_options_check", _int, [_P(SamplerOptions)]),
    ("pg_sampler_param_count", _int, []),
    ("pg_sampler_param", _int, [_int, _P(ParamDesc)]),
    ("pg_sampler_envelope_param_count", _int, []),
    ("pg_sampler_envelope_param", _int, [_int, _P(ParamDesc)]),
    ("pg_granular_sampler_options_default", None, [_P(GranularSamplerOptions)]),
    ("pg_granular_sampler_options_check", _int, [_P(GranularSamplerOptions)]),
    ("pg_granular_sampler_rng_state", None, [_P(_u64), _u32, _u32, _P(_u64)]),
    ("pg_generator_options_default", None, [_P(GeneratorOptions)]),
    ("pg_generator_options_check", _int, [_P(GeneratorOptions)]),
    ("pg_modulation_params_default", None, [_P(ModulationParams)]),
    ("pg_modulation_params_check", _int, [_P(ModulationParams)]),
    ("pg_debug_sample_buffer_times", _int, [_vp, _int, _P(_f32)]),
    ("pg_debug_sample_buffer_waveform_time", _int, [_vp, _int, _P(_f32)]),
    ("pg_debug_fail_launch_round", None, [_int]),
    ("pg_debug_hip_calls", None, [_P(_u64)]),
    ("pg_sharded_create", _vp, [_u32, _u32, _sz, _P(_int), _int]),
    ("pg_sharded_destroy", None, [_vp]),
)


def _declare(lib, prefix, calls, present_only=False):
    for name, res, args in calls:
        if present_only and not hasattr(lib, prefix + name):
            continue
        fn = getattr(lib, prefix + name)
        fn.restype = res
        fn.argtypes = [_vp] + args


def declare(lib, prefix):
    """Declare argtypes/restypes of the API shared by the product (pg_) and, in tests, the oracle (po_): the effect handle, graph_create /
    graph_destroy and the mixer's calls — all of them for the product, for the oracle the ones it has."""
    _declare(lib, prefix + "effect_", EFFECT_CALLS)
    create = getattr(lib, prefix + "graph_create")
    create.restype, create.argtypes = _vp, [_u32, _u32, _sz, _int]
    _declare(lib, prefix + "graph_", (("destroy", None, []),))
    _declare(lib, prefix + "graph_", MIXER_CALLS, present_only=prefix != "pg_")
    return lib


def _preload_hip_runtime():
    """One HIP runtime per process. PyTorch wheels bundle their own libamdhip64.so (soname libamdhip64.so.7, the same
    soname libphonic_gpu.so needs); if the system runtime from /opt/rocm were loaded first, a later `import torch`
    would bring in a second runtime that sees no GPUs. So when torch is installed its runtime is loaded first
    (RTLD_GLOBAL) and libphonic_gpu.so binds to it by soname. PHONIC_HIP_RUNTIME=system opts out (torch-free runs,
    e.g. profiling the single-GPU bench against /opt/rocm)."""
    import sys

    if os.environ.get("PHONIC_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def preload_rccl():
    """The RCCL that matches the HIP runtime in the process: libphonic_gpu.so looks RCCL up by soname (librccl.so.1) when
    pg_sharded_set_reduce(PG_REDUCE_RCCL) is called. With PyTorch's runtime loaded (see above) that must be PyTorch's RCCL, so it is
    loaded first; without torch (or with PHONIC_HIP_RUNTIME=system) the library finds ROCm's own on its run path."""
    import sys

    if os.environ.get("PHONIC_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def source_hash():
    """16 hex digits over the sources libphonic_gpu.so is built from (csrc/*.hip|.h|.inl, the Makefile, include/phonic_gpu.h). Profiles that
    bench.py quotes (profiles/*_pmc_traffic.json) carry the hash of the build they were measured with."""
    import glob
    import hashlib

    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "csrc", "*.hip")) + glob.glob(os.path.join(here, "csrc", "*.h")) + glob.glob(os.path.join(here, "csrc", "*.inl")))
    files += [os.path.join(here, "csrc", "Makefile"), os.path.join(here, "csrc", "phonic_gpu.map"), os.path.join(os.path.dirname(here), "include", "phonic_gpu.h")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


_LIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libphonic_gpu.so")


def load():
    """Load libphonic_gpu.so (HIP). Raises if it has not been built — no fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PHONIC_LIB: another build of the SAME library (tools/ab_libs/*.so: A/B runs of kernel variants on one box) — still HIP, still no fallback
    path = os.environ.get("PHONIC_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). phonic_amd has no CPU fallback."
        )
    _preload_hip_runtime()
    lib = C.CDLL(path)
    declare(lib, "pg_")
    _declare(lib, "pg_graph_", GRAPH_ONLY_CALLS)
    _declare(lib, "pg_sharded_", MIXER_CALLS)
    _declare(lib, "pg_sharded_", SHARDED_ONLY_CALLS)
    for name, res, args in PLAIN_CALLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _LIB = lib
    return lib
