"""Thin object wrappers over the C ABI (include/phonic_gpu.h).

`EffectHandle` mirrors the reference `Effect` trait (src/effect.rs:86-215) and `GraphHandle` the
main `MixedSource` as driven by `Player` (src/player.rs, src/source/mixed.rs). Both are written
against a (library, prefix) pair so that the test-suite can drive the CPU oracle (prefix `po_`)
with exactly the same call sequence as the product (prefix `pg_`).
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import fourcc


class PhonicError(RuntimeError):
    """Maps the reference `Error` enum (src/error.rs:8-22)."""

    def __init__(self, code, msg=""):
        names = {1: "ParameterError", 2: "NotFoundError", 3: "SendError", 4: "DeviceError", 5: "StateError"}
        super().__init__(f"{names.get(code, code)}: {msg}")
        self.code = code


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class EffectHandle:
    """`dyn Effect` (src/effect.rs:86-215)."""

    def __init__(self, lib, prefix, kind, params=None, reverb_seeds=None, device=0, lfo_seed=None):
        self._lib, self._p = lib, prefix
        self.kind = kind
        init = _capi.make_init(params, reverb_seeds, lfo_seed)
        create = getattr(lib, prefix + "effect_create")
        if prefix == "pg_":
            self._h = create(kind, C.byref(init), device)
        else:
            create.restype = C.c_void_p
            create.argtypes = [C.c_int, C.POINTER(_capi.EffectInit)]
            self._h = create(kind, C.byref(init))
        if not self._h:
            raise PhonicError(_capi.PG_ERR_PARAMETER, self._err() or "effect_create failed")
        self.channels = 2

    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _err(self):
        if self._p == "pg_":
            m = self._lib.pg_last_error_message()
            return m.decode() if m else ""
        return ""

    def _check(self, code):
        if code != 0:
            raise PhonicError(code, self._err())

    def name(self):
        return _capi.FX_NAMES[self.kind]

    def initialize(self, sample_rate, channel_count, max_frames):
        self.channels = channel_count
        self._check(self._fn("effect_initialize")(self._h, sample_rate, channel_count, max_frames))

    def process(self, buf, pos_in_frames=0):
        """In place on a contiguous float32 numpy array of interleaved samples."""
        assert buf.dtype == np.float32 and buf.flags["C_CONTIGUOUS"]
        self._check(self._fn("effect_process")(self._h, _f32p(buf), buf.size, pos_in_frames))
        return buf

    def process_tail(self):
        t = self._fn("effect_tail")(self._h)
        if t < 0:
            return None
        return t

    def set_parameter(self, id4, value, normalized=False):
        self._check(self._fn("effect_set_parameter")(self._h, fourcc(id4), float(value), 1 if normalized else 0))

    def reset(self):
        self._check(self._fn("effect_message_reset")(self._h))

    def close(self):
        if self._h:
            self._fn("effect_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphHandle:
    """The main `MixedSource` plus the `Player` calls that populate it."""

    def __init__(self, lib, prefix, sample_rate=48000, channels=2, max_frames=4096, device=0):
        self._lib, self._p = lib, prefix
        self.sample_rate, self.channels = sample_rate, channels
        self._h = getattr(lib, prefix + "graph_create")(sample_rate, channels, max_frames, device)
        if not self._h:
            raise PhonicError(_capi.PG_ERR_DEVICE, self._err() or "graph_create failed")

    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _err(self):
        if self._p == "pg_":
            m = self._lib.pg_last_error_message()
            return m.decode() if m else ""
        return ""

    def _check(self, code):
        if code != 0:
            raise PhonicError(code, self._err())

    def _id(self, v):
        if v < 0:
            raise PhonicError(-v, self._err())
        return v

    def add_mixer(self, parent=None):
        """Player::add_mixer(parent_mixer_id): None / 0 = child of the main mixer."""
        if not parent:
            return self._id(self._fn("graph_add_mixer")(self._h))
        return self._id(self._fn("graph_add_mixer_to")(self._h, parent))

    def add_effect(self, mixer_id, kind, params=None, reverb_seeds=None, lfo_seed=None):
        init = _capi.make_init(params, reverb_seeds, lfo_seed)
        return self._id(self._fn("graph_add_effect")(self._h, mixer_id, kind, C.byref(init)))

    def add_voice(self, mixer_id, pcm, src_channels, src_rate, **opts):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        assert pcm.size % src_channels == 0
        o = _capi.default_voice_options(**opts)
        return self._id(
            self._fn("graph_add_voice")(self._h, mixer_id, _f32p(pcm), pcm.size // src_channels, src_channels, src_rate, C.byref(o))
        )

    def add_granular_voice(self, mixer_id, pcm, params=None, channels=1, **opts):
        """A sampler voice in granular mode (GrainPool, src/generator/sampler/granular.rs): `pcm` at the graph's rate, mono — or `channels`
        interleaved channels, mixed down as Sampler::create_granular_sample_buffer does. `params`: a _capi.GranularParams (see
        _capi.granular_params); opts: volume, panning, speed, start_time."""
        mono = _capi.mono_downmix(pcm, channels)
        p = params if params is not None else _capi.granular_params()
        o = _capi.default_voice_options(**opts)
        return self._id(self._fn("graph_add_granular_voice")(self._h, mixer_id, _f32p(mono), mono.size, C.byref(p), C.byref(o)))

    # ---- sample buffers: one decoded file on the device (Arc<AudioFileBuffer>), played by any number of file and granular voices ----
    def add_sample_buffer(self, pcm, channels, rate, loop_range=None):
        """Uploads `pcm` (interleaved, with the decoder's extra zero frame) once and returns a buffer id. loop_range = the file's embedded loop
        (start, end) in source frames, or None."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        assert pcm.size % channels == 0
        d = _capi.sample_buffer_desc(channels, rate, loop_range)
        return self._id(self._fn("graph_add_sample_buffer")(self._h, _f32p(pcm), pcm.size // channels, C.byref(d)))

    def release_sample_buffer(self, buffer_id):
        """Drops the host's reference: the id is gone, voices that play the buffer keep playing, the last of them frees the memory."""
        self._check(self._fn("graph_release_sample_buffer")(self._h, buffer_id))

    def add_voice_from_buffer(self, mixer_id, buffer_id, **opts):
        """PreloadedFileSource::from_shared_buffer: add_voice on the buffer's PCM, without a copy; the buffer's loop range is the file's embedded one."""
        o = _capi.default_voice_options(**opts)
        return self._id(self._fn("graph_add_voice_from_buffer")(self._h, mixer_id, buffer_id, C.byref(o)))

    def add_granular_voice_from_buffer(self, mixer_id, buffer_id, params=None, **opts):
        """add_granular_voice on the buffer's granular mono buffer (Sampler::create_granular_sample_buffer, made on the device, once per buffer)."""
        p = params if params is not None else _capi.granular_params()
        o = _capi.default_voice_options(**opts)
        return self._id(self._fn("graph_add_granular_voice_from_buffer")(self._h, mixer_id, buffer_id, C.byref(p), C.byref(o)))

    def prepare_granular_buffer(self, buffer_id):
        """Makes the buffer's granular mono buffer now (load time) instead of with its first granular voice."""
        self._check(self._fn("graph_prepare_granular_buffer")(self._h, buffer_id))

    def sample_buffer_info(self, buffer_id):
        info = _capi.SampleBufferInfo()
        self._check(self._fn("graph_sample_buffer_info")(self._h, buffer_id, C.byref(info)))
        return _capi.sample_buffer_info_dict(info)

    def read_granular_buffer(self, buffer_id):
        """The buffer's granular mono buffer as a float32 array (debug read-back; makes it if it is not there)."""
        n = self._fn("graph_read_granular_buffer")(self._h, buffer_id, None, 0)
        out = np.zeros(self._id(n), np.float32)
        self._id(self._fn("graph_read_granular_buffer")(self._h, buffer_id, _f32p(out), out.size))
        return out

    def sample_buffer_waveform(self, buffer_id, resolution, mode="mixed_down", source="file", first_frame=0, n_frames=None):
        """waveform::mixed_down / multi_channel (reference src/utils/waveform.rs) of frames [first_frame, first_frame + n_frames) of the buffer
        (source="file": the PCM as uploaded) or of its granular mono buffer (source="granular"), computed on the device. n_frames=None: up to the
        source's end. Returns a dict of numpy arrays frame (uint64), time (float32 seconds), min, max (float32), counted from the slice's start:
        shape (P,) for mode="mixed_down", (channels, P) for mode="multi_channel", P = min(n_frames, resolution). A display helper, not a
        real-time call: it waits for the device."""
        modes = {"mixed_down": _capi.PG_WAVEFORM_MIXED_DOWN, "multi_channel": _capi.PG_WAVEFORM_MULTI_CHANNEL}
        sources = {"file": _capi.PG_WAVEFORM_OF_FILE, "granular": _capi.PG_WAVEFORM_OF_GRANULAR}
        if mode not in modes or source not in sources:
            raise ValueError(f"mode must be one of {sorted(modes)}, source one of {sorted(sources)}")
        info = self.sample_buffer_info(buffer_id)
        if source == "granular":
            if info["granular_frames"] < 0:
                self.prepare_granular_buffer(buffer_id)
                info = self.sample_buffer_info(buffer_id)
            total, channels = info["granular_frames"], 1
        else:
            total, channels = info["n_frames"], info["channels"]
        if n_frames is None:
            n_frames = max(total - int(first_frame), 0)
        rows = channels if mode == "multi_channel" else 1
        cap = rows * min(int(n_frames), int(resolution))
        buf = (_capi.WaveformPoint * max(cap, 1))()
        p = self._id(self._fn("graph_sample_buffer_waveform")(self._h, buffer_id, sources[source], modes[mode], int(first_frame), int(n_frames), int(resolution), buf, cap))
        pts = np.frombuffer(buf, dtype=np.dtype([("frame", "<u8"), ("time", "<f4"), ("min", "<f4"), ("max", "<f4"), ("reserved", "<u4")]), count=rows * p)
        shape = (rows, p) if mode == "multi_channel" else (p,)
        return {k: pts[k].reshape(shape).copy() for k in ("frame", "time", "min", "max")}

    def voice_grain_state(self, voice):
        """The voice's GrainPool and its 100 grains as a dict (debug read-back: waits for the graph's stream)."""
        st = _capi.GrainState()
        self._check(self._fn("graph_voice_grain_state")(self._h, voice, C.byref(st)))
        return _capi.grain_state_dict(st)

    def set_voice_granular_parameter(self, voice, id4, value, sample_time, normalized=False):
        """GeneratorPlaybackHandle::set_parameter for one of the Sampler's GRAIN_* ids (_capi.GRANULAR_PARAM_IDS) on this voice, in front of frame
        sample_time. Raw values are clamped to the descriptor's range, enum values are the variant's index."""
        self._check(self._fn("graph_set_voice_granular_parameter")(self._h, voice, _capi.fourcc(id4), float(value), 1 if normalized else 0, sample_time))

    def set_voice_grain_loop_range(self, voice, loop_range, sample_time):
        """GrainPool::set_loop_range in front of frame sample_time: (start, end) normalised to [0, 1], or None."""
        has = loop_range is not None
        self._check(self._fn("graph_set_voice_grain_loop_range")(self._h, voice, 1 if has else 0, float(loop_range[0]) if has else 0.0, float(loop_range[1]) if has else 0.0, sample_time))

    def voice_granular_params(self, voice):
        """The voice's granular parameters and loop range as the device holds them (debug read-back: waits for the graph's stream)."""
        p = _capi.GranularParams()
        self._check(self._fn("graph_voice_granular_params")(self._h, voice, C.byref(p)))
        return _capi.granular_params_dict(p)

    def set_voice_modulation_matrix(self, voice, params=None, **kw):
        """The ModulationMatrix of a granular voice (two LFOs, velocity, keytracking -> the seven granular targets) + note_on; before the voice
        renders. `params`: a _capi.ModulationParams, or the keywords of _capi.modulation_params."""
        p = params if params is not None else _capi.modulation_params(**kw)
        self._check(self._fn("graph_set_voice_modulation_matrix")(self._h, voice, C.byref(p)))

    def set_voice_modulation(self, voice, source, target, amount, bipolar, sample_time):
        """GeneratorPlaybackHandle::set_modulation for this voice, in front of frame sample_time (|amount| < 0.001 removes the route)."""
        self._check(self._fn("graph_set_voice_modulation")(self._h, voice, source, target, float(amount), 1 if bipolar else 0, sample_time))

    def clear_voice_modulation(self, voice, source, target, sample_time):
        self._check(self._fn("graph_clear_voice_modulation")(self._h, voice, source, target, sample_time))

    def set_voice_lfo_rate(self, voice, lfo, rate_hz, sample_time):
        self._check(self._fn("graph_set_voice_lfo_rate")(self._h, voice, lfo, float(rate_hz), sample_time))

    def set_voice_lfo_waveform(self, voice, lfo, waveform, sample_time):
        self._check(self._fn("graph_set_voice_lfo_waveform")(self._h, voice, lfo, int(waveform), sample_time))

    def voice_modulation_state(self, voice):
        """The matrix as a dict (debug read-back: waits for the graph's stream)."""
        st = _capi.ModulationState()
        self._check(self._fn("graph_voice_modulation_state")(self._h, voice, C.byref(st)))
        return _capi.modulation_state_dict(st)

    # ---- host-fed sources (any `dyn Source` the host pulls itself) ----
    def add_stream_voice(self, mixer_id, channels, rate, capacity_frames, **opts):
        o = _capi.default_voice_options(**opts)
        v = self._id(self._fn("graph_add_stream_voice")(self._h, mixer_id, channels, rate, capacity_frames, C.byref(o)))
        if not hasattr(self, "_stream_channels"):
            self._stream_channels = {}
        self._stream_channels[v] = channels
        return v

    def feed_voice(self, voice, frames):
        """Interleaved float32 frames of the host's source; raises SendError (PG_ERR_QUEUE_FULL) when the ring has no room for all of them."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        ch = self._stream_channels.get(voice) if hasattr(self, "_stream_channels") else None
        n = frames.size // (ch or 1)
        self._check(self._fn("graph_feed_voice")(self._h, voice, _f32p(frames), n))

    def end_stream_voice(self, voice):
        self._check(self._fn("graph_end_stream_voice")(self._h, voice))

    def stream_voice_consumed(self, voice):
        return self._id(self._fn("graph_stream_voice_consumed")(self._h, voice))

    def is_voice_playing(self, voice):
        return bool(self._fn("graph_is_voice_playing")(self._h, voice))

    def stop_all_voices(self):
        """Player::stop_all_sources (src/player.rs:1012-1045)."""
        self._check(self._fn("graph_stop_all_voices")(self._h))

    def remove_mixer(self, mixer_id):
        """Player::remove_mixer (src/player.rs:825-867)."""
        self._check(self._fn("graph_remove_mixer")(self._h, mixer_id))

    def remove_effect(self, effect_id):
        """Player::remove_effect (src/player.rs:977-990)."""
        self._check(self._fn("graph_remove_effect")(self._h, effect_id))

    def move_effect(self, effect_id, mixer_id, movement, offset=0):
        """Player::move_effect (src/player.rs:942-972): movement = MOVE_DIRECTION (with offset) / MOVE_START / MOVE_END."""
        self._check(self._fn("graph_move_effect")(self._h, effect_id, mixer_id, movement, offset))

    def schedule_param(self, effect_id, id4, value, sample_time, normalized=False):
        self._check(self._fn("graph_schedule_param")(self._h, effect_id, fourcc(id4), float(value), 1 if normalized else 0, sample_time))

    def schedule_reset(self, effect_id, sample_time):
        self._check(self._fn("graph_schedule_reset")(self._h, effect_id, sample_time))

    def set_voice_volume(self, voice, volume, sample_time):
        self._check(self._fn("graph_set_voice_volume")(self._h, voice, float(volume), sample_time))

    def set_voice_panning(self, voice, panning, sample_time):
        self._check(self._fn("graph_set_voice_panning")(self._h, voice, float(panning), sample_time))

    def stop_voice(self, voice, sample_time):
        self._check(self._fn("graph_stop_voice")(self._h, voice, sample_time))

    def set_voice_envelope(self, voice, params=None, **kw):
        """AHDSR volume envelope of a voice (SamplerVoice::start: parameters at the graph's rate + note_on(1.0)); before the voice renders.
        `params`: a _capi.AhdsrParams, or keyword overrides of AhdsrParameters::default()."""
        p = params if params is not None else _capi.ahdsr_params(**kw)
        self._check(self._fn("graph_set_voice_envelope")(self._h, voice, C.byref(p)))

    def release_voice(self, voice, sample_time):
        """SamplerVoice::stop: the envelope's note_off at exactly sample_time (a voice without an envelope stops there)."""
        self._check(self._fn("graph_release_voice")(self._h, voice, sample_time))

    def voice_envelope_stage(self, voice):
        """0 Idle .. 5 Release, -1: no envelope (waits for the graph's stream)."""
        return int(self._fn("graph_voice_envelope_stage")(self._h, voice))

    def set_metering(self, interval_seconds):
        """PlayerConfig::metering_interval for every mixer of the graph: seconds >= 0 switches the level meters on (all levels reset to 0),
        None switches them off."""
        self._check(self._fn("graph_set_metering")(self._h, -1.0 if interval_seconds is None else float(interval_seconds)))

    def audio_level(self, mixer_id=0):
        """Player::audio_level (mixer 0) / MixerHandle::audio_level: the level the mixer last published (a _capi.Level). Never waits for the device."""
        raw = _capi.AudioLevel()
        self._check(self._fn("graph_mixer_audio_level")(self._h, mixer_id, C.byref(raw)))
        return _capi.Level(raw)

    def enable_status(self, capacity_events=4096):
        """Playback status events (PlaybackStatusEvent::Position / Stopped): once, before the first write; the ring holds `capacity_events` unpolled records."""
        self._check(self._fn("graph_enable_status")(self._h, capacity_events))

    def set_voice_status(self, voice, position_emit_seconds=None, report_stopped=True):
        """FilePlaybackOptions::playback_pos_emit_rate of a voice (None: no Position records) and whether it reports Stopped; before the voice renders."""
        self._check(self._fn("graph_set_voice_status")(self._h, voice, -1.0 if position_emit_seconds is None else float(position_emit_seconds), 1 if report_stopped else 0))

    def poll_status(self, max_events=4096):
        """The records of every write that has returned, oldest first, as _capi.status_tuple tuples."""
        buf = (_capi.StatusEvent * max_events)()
        n = int(self._fn("graph_poll_status")(self._h, buf, max_events))
        return [_capi.status_tuple(buf[i]) for i in range(n)]

    def status_dropped(self):
        """Records dropped because the ring was full (the reference's try_send on a full channel)."""
        return int(self._fn("graph_status_dropped")(self._h))

    def remove_voice(self, voice):
        """MixerMessage::RemoveSource: the source leaves its mixer at the start of the next write, at once (no fade)."""
        self._check(self._fn("graph_remove_voice")(self._h, voice))

    def set_voice_speed(self, voice, speed, sample_time, glide=None):
        """FilePlaybackHandle::set_speed(speed, glide): glide in semitones per second, None = immediate."""
        self._check(self._fn("graph_set_voice_speed")(self._h, voice, float(speed), float(glide) if glide else 0.0, sample_time))

    def seek_voice(self, voice, seconds, sample_time):
        self._check(self._fn("graph_seek_voice")(self._h, voice, float(seconds), sample_time))

    def write(self, out, pos_in_frames):
        """`Source::write`: fills `out` (float32 interleaved), returns samples written."""
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        return self._fn("graph_write")(self._h, _f32p(out), out.size, pos_in_frames)

    def render(self, n_blocks, block_frames=1024, start_pos=0):
        """Offline pull loop of the reference WavOutput (src/output/wav.rs:210-250): fixed size blocks."""
        out = np.zeros((n_blocks, block_frames * self.channels), dtype=np.float32)
        pos = start_pos
        for b in range(n_blocks):
            self.write(out[b], pos)
            pos += block_frames
        return out.reshape(-1)

    def close(self):
        if self._h:
            self._fn("graph_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
