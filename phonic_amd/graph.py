"""GPU-resident mixer graph: Python mirror of the reference's `Player` calls that populate the main
`MixedSource` (src/player.rs:519-602,773-822,893-939) and of `Source::write` (src/source.rs:95).
Everything forwards to the C ABI of include/phonic_gpu.h; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _capi
from ._wrap import GraphHandle, PhonicError


class Graph(GraphHandle):
    def __init__(self, sample_rate=48000, channels=2, max_frames=4096, device=0):
        super().__init__(_capi.load(), "pg_", sample_rate, channels, max_frames, device)
        self.max_frames = max_frames

    # -- device-side output (multi-GPU master-bus reduce, bench.py) ------------------------------------
    def write_device(self, d_out_ptr, n_samples, pos_in_frames, stream=None):
        """`Source::write` into device memory (`d_out_ptr` = device pointer as int). Asynchronous on `stream` (a hipStream_t as int);
        without one — and that includes the default stream, whose handle is 0 — the call renders on the graph's own stream and
        returns when the block is complete."""
        return self._lib.pg_graph_write_device(self._h, C.c_void_p(d_out_ptr), n_samples, pos_in_frames, C.c_void_p(stream or 0))

    def sample_buffer_times(self, buffer_id):
        """Measurement hook (pg_debug_sample_buffer_times): hipEvent ms of the buffer's upload and of the two passes of its conversion, taken only
        in a process with PHONIC_DEBUG_HOOKS=1 in its environment (zeros otherwise)."""
        out = (C.c_float * 3)()
        self._check(self._lib.pg_debug_sample_buffer_times(self._h, buffer_id, out))
        return dict(upload_ms=out[0], sched_ms=out[1], interp_ms=out[2])

    def sample_buffer_waveform_time(self, buffer_id):
        """Measurement hook (pg_debug_sample_buffer_waveform_time): hipEvent ms of the kernels of the buffer's last sample_buffer_waveform call, taken
        only in a process with PHONIC_DEBUG_HOOKS=1 in its environment (zero otherwise)."""
        out = C.c_float(0.0)
        self._check(self._lib.pg_debug_sample_buffer_waveform_time(self._h, buffer_id, C.byref(out)))
        return float(out.value)

    # -- samplers: the Sampler generator's note layer (notes, voice allocation, stealing) for file playback; sub-mixers only ----------
    def add_sampler(self, mixer_id, buffer_id, options=None, **kw):
        """A pool of `voice_count` file voices of sample buffer `buffer_id` in sub-mixer `mixer_id` (Sampler::from_file + Player::add_generator /
        play_generator). `options`: a _capi.SamplerOptions, or the keywords of _capi.sampler_options (voice_count, envelope, loop_range, transient,
        start_time). Returns the sampler id."""
        o = options if options is not None else _capi.sampler_options(**kw)
        return self._id(self._lib.pg_graph_add_sampler(self._h, mixer_id, buffer_id, C.byref(o)))

    def remove_sampler(self, sampler):
        """MixerMessage::RemoveSource: the pool leaves its mixer at the start of the next write."""
        self._check(self._lib.pg_graph_remove_sampler(self._h, sampler))

    def sampler_note_on(self, sampler, note, volume=1.0, panning=0.0, sample_time=0):
        """GeneratorPlaybackHandle::note_on in front of frame sample_time (0: the next write's first frame); returns the note id."""
        return self._id(self._lib.pg_graph_sampler_note_on(self._h, sampler, int(note), float(volume), float(panning), sample_time))

    def sampler_note_off(self, sampler, note_id, sample_time=0):
        self._check(self._lib.pg_graph_sampler_note_off(self._h, sampler, note_id, sample_time))

    def sampler_all_notes_off(self, sampler, sample_time=0):
        self._check(self._lib.pg_graph_sampler_all_notes_off(self._h, sampler, sample_time))

    def sampler_set_note_speed(self, sampler, note_id, speed, sample_time=0, glide=None):
        """set_speed of one note: composed with the base pitch; glide in semitones per second, None = immediate."""
        self._check(self._lib.pg_graph_sampler_set_note_speed(self._h, sampler, note_id, float(speed), float(glide) if glide else 0.0, sample_time))

    def sampler_set_note_volume(self, sampler, note_id, volume, sample_time=0):
        self._check(self._lib.pg_graph_sampler_set_note_volume(self._h, sampler, note_id, float(volume), sample_time))

    def sampler_set_note_panning(self, sampler, note_id, panning, sample_time=0):
        self._check(self._lib.pg_graph_sampler_set_note_panning(self._h, sampler, note_id, float(panning), sample_time))

    def sampler_set_parameter(self, sampler, id4, value, sample_time=0, normalized=False):
        """One of the base parameters (_capi.SAMPLER_PARAM_IDS: STRN, SFTN, SVOL, SPAN) in front of frame sample_time."""
        self._check(self._lib.pg_graph_sampler_set_parameter(self._h, sampler, _capi.fourcc(id4), float(value), 1 if normalized else 0, sample_time))

    def sampler_stop(self, sampler, sample_time=0):
        """Sampler::stop: all notes off; a transient sampler stops for good once its last voice has ended."""
        self._check(self._lib.pg_graph_sampler_stop(self._h, sampler, sample_time))

    # -- granular-mode samplers: Sampler::with_granular_playback — pools of granular voices that notes start, steal and release ----------
    def add_granular_sampler(self, mixer_id, buffer_id, params=None, modulation=None, rng_states=None, options=None, **kw):
        """A pool of `voice_count` granular voices over sample buffer `buffer_id`'s granular mono buffer in sub-mixer `mixer_id`. params: a
        _capi.GranularParams (default: GranularParameters::default()); modulation: a _capi.ModulationParams (every slot gets such a matrix) or
        None (no matrix); rng_states: None, or per slot three Xoshiro256++ states (pool, LFO 1, LFO 2); `options` / keywords as for add_sampler.
        Every sampler_* call works on the returned id."""
        o = options if options is not None else _capi.sampler_options(**kw)
        go = _capi.granular_sampler_options(params if params is not None else _capi.granular_params(), modulation, rng_states)
        return self._id(self._lib.pg_graph_add_granular_sampler(self._h, mixer_id, buffer_id, C.byref(o), C.byref(go)))

    def sampler_set_granular_parameter(self, sampler, id4, value, sample_time=0, normalized=False):
        """Sampler::set_granular_parameter for one of _capi.GRANULAR_PARAM_IDS, in front of frame sample_time: every slot, playing or free."""
        self._check(self._lib.pg_graph_sampler_set_granular_parameter(self._h, sampler, _capi.fourcc(id4), float(value), 1 if normalized else 0, sample_time))

    def sampler_voice_grain_state(self, sampler, slot):
        """Slot `slot`'s GrainPool as _capi.grain_state_dict gives it (debug read-back: waits for the graph's work)."""
        st = _capi.GrainState()
        self._check(self._lib.pg_graph_sampler_voice_grain_state(self._h, sampler, slot, C.byref(st)))
        return _capi.grain_state_dict(st)

    def sampler_voice_modulation_state(self, sampler, slot):
        """Slot `slot`'s modulation matrix as _capi.modulation_state_dict gives it."""
        st = _capi.ModulationState()
        self._check(self._lib.pg_graph_sampler_voice_modulation_state(self._h, sampler, slot, C.byref(st)))
        return _capi.modulation_state_dict(st)

    def sampler_granular_params(self, sampler):
        """The sampler's granular parameters and loop range as _capi.granular_params_dict gives them."""
        p = _capi.GranularParams()
        self._check(self._lib.pg_graph_sampler_granular_params(self._h, sampler, C.byref(p)))
        return _capi.granular_params_dict(p)

    # -- what changes every voice of a pool while notes sound (SetParameter(AMP_* | ML1R ..), SetModulation, ClearModulation, SetLoopRange) ----------
    def sampler_set_envelope_parameter(self, sampler, id4, value, sample_time=0, normalized=False):
        """One of _capi.SAMPLER_ENVELOPE_PARAM_IDS (AATK, AHLD, ADCY, ASTN, AREL) of the pool's one AhdsrParameters, in front of frame sample_time.
        File samplers and granular ones; the sampler must have an envelope."""
        self._check(self._lib.pg_graph_sampler_set_envelope_parameter(self._h, sampler, _capi.fourcc(id4), float(value), 1 if normalized else 0, sample_time))

    def sampler_envelope_params(self, sampler, slot=0):
        """The AhdsrParameters as the device holds them (_capi.sampler_envelope_state_dict): slot `slot`'s copy of a file sampler, a granular
        sampler's one set. Debug read-back: waits for the graph's work."""
        st = _capi.SamplerEnvelopeState()
        self._check(self._lib.pg_graph_sampler_envelope_params(self._h, sampler, slot, C.byref(st)))
        return _capi.sampler_envelope_state_dict(st)

    def sampler_set_modulation(self, sampler, source, target, amount, bipolar=False, sample_time=0):
        """SetModulation for the matrix of every slot of a granular sampler, playing or free (|amount| < 0.001 removes the route)."""
        self._check(self._lib.pg_graph_sampler_set_modulation(self._h, sampler, int(source), int(target), float(amount), 1 if bipolar else 0, sample_time))

    def sampler_clear_modulation(self, sampler, source, target, sample_time=0):
        self._check(self._lib.pg_graph_sampler_clear_modulation(self._h, sampler, int(source), int(target), sample_time))

    def sampler_set_lfo_rate(self, sampler, lfo, rate_hz, sample_time=0):
        """ML1R / ML2R: every slot's LFO `lfo` (0, 1), clamped to 0.01..20 Hz; phase and draws stay."""
        self._check(self._lib.pg_graph_sampler_set_lfo_rate(self._h, sampler, int(lfo), float(rate_hz), sample_time))

    def sampler_set_lfo_waveform(self, sampler, lfo, waveform, sample_time=0):
        """ML1W / ML2W: an index into _capi.LFO_WAVEFORMS."""
        self._check(self._lib.pg_graph_sampler_set_lfo_waveform(self._h, sampler, int(lfo), int(waveform), sample_time))

    def sampler_set_loop_range(self, sampler, loop_range, sample_time=0):
        """SamplerMessage::SetLoopRange on a granular sampler: (start, end) in source frames of its buffer, or None for NO loop."""
        has = loop_range is not None
        self._check(self._lib.pg_graph_sampler_set_loop_range(self._h, sampler, 1 if has else 0, int(loop_range[0]) if has else 0, int(loop_range[1]) if has else 0, sample_time))

    # -- samplers on the main mixer: Player::play_generator / add_generator without a target mixer, with the generator's volume and panning ----
    def add_sampler_to_main(self, buffer_id, volume=None, panning=None, options=None, **kw):
        """A file sampler as ONE source of the main mixer behind AmplifiedSource(volume) -> PannedSource(panning) (GeneratorPlaybackOptions;
        defaults 1.0 / 0.0). `options` / keywords as for add_sampler. Every sampler_* call works on the returned id."""
        o = options if options is not None else _capi.sampler_options(**kw)
        gen = _capi.generator_options(volume, panning)
        return self._id(self._lib.pg_graph_add_sampler_to_main(self._h, buffer_id, C.byref(o), C.byref(gen)))

    def add_granular_sampler_to_main(self, buffer_id, params=None, modulation=None, rng_states=None, volume=None, panning=None, options=None, **kw):
        """A granular-mode sampler on the main mixer: add_granular_sampler's arguments, add_sampler_to_main's placement and output stage."""
        o = options if options is not None else _capi.sampler_options(**kw)
        go = _capi.granular_sampler_options(params if params is not None else _capi.granular_params(), modulation, rng_states)
        gen = _capi.generator_options(volume, panning)
        return self._id(self._lib.pg_graph_add_granular_sampler_to_main(self._h, buffer_id, C.byref(o), C.byref(go), C.byref(gen)))

    def sampler_set_volume(self, sampler, volume, sample_time=0):
        """GeneratorPlaybackHandle::set_volume of a sampler on the main mixer (PG_ERR_STATE for one in a sub-mixer)."""
        self._check(self._lib.pg_graph_sampler_set_volume(self._h, sampler, float(volume), sample_time))

    def sampler_set_panning(self, sampler, panning, sample_time=0):
        """GeneratorPlaybackHandle::set_panning of a sampler on the main mixer (PG_ERR_STATE for one in a sub-mixer)."""
        self._check(self._lib.pg_graph_sampler_set_panning(self._h, sampler, float(panning), sample_time))

    def sampler_output_state(self, sampler):
        """The two smoothers of a main-mixer sampler's output stage (_capi.sampler_output_state_dict). Debug read-back: waits for the graph's work."""
        st = _capi.SamplerOutputState()
        self._check(self._lib.pg_graph_sampler_output_state(self._h, sampler, C.byref(st)))
        return _capi.sampler_output_state_dict(st)

    def sampler_state(self, sampler):
        """The slot table and the sampler's own state as a dict (debug read-back: waits for the graph's work)."""
        st = _capi.SamplerState()
        self._check(self._lib.pg_graph_sampler_state(self._h, sampler, C.byref(st)))
        return _capi.sampler_state_dict(st)

    def set_max_blocks_per_launch(self, n_blocks):
        """Offline rendering: let one write call render up to `n_blocks` blocks of max_frames per launch sequence (steady state only)."""
        self._check(self._lib.pg_graph_set_max_blocks_per_launch(self._h, int(n_blocks)))

    def device_errors(self):
        """Sticky consistency flags raised by the kernels (0 = none)."""
        return self._id(self._lib.pg_graph_device_errors(self._h))

    def set_defer_bus(self, defer):
        self._check(self._lib.pg_graph_set_defer_bus(self._h, 1 if defer else 0))

    def process_bus_device(self, d_bus_ptr, n_samples, pos_in_frames, stream=None, flags_ptr=None, n_words=0):
        """The main mixer's chain over a summed bus the caller holds; flags_ptr: the ranks' summed `audible` words (export_audible), one per block of max_frames."""
        if flags_ptr:
            self._check(self._lib.pg_graph_process_bus_device_flags(self._h, C.c_void_p(d_bus_ptr), n_samples, pos_in_frames, C.c_void_p(stream or 0), C.c_void_p(flags_ptr), n_words))
        else:
            self._check(self._lib.pg_graph_process_bus_device(self._h, C.c_void_p(d_bus_ptr), n_samples, pos_in_frames, C.c_void_p(stream or 0)))

    def export_audible(self, d_dst_ptr, n_words, stream=None):
        """The `audible` words of the last write_device call of a deferred-bus graph as floats (0 / 1): they ride with the partial bus in one reduce."""
        self._check(self._lib.pg_graph_export_audible(self._h, C.c_void_p(d_dst_ptr), n_words, C.c_void_p(stream or 0)))

    def audible_words(self):
        """Words the last deferred-bus write_device call left: one per piece it was rendered in (events add pieces)."""
        return int(self._lib.pg_graph_audible_words(self._h))

    def next_main_event(self, pos_in_frames):
        """Sample time of the first main-mixer event behind pos_in_frames (None: none pending). Writing thread only (drains the control ring)."""
        t = int(self._lib.pg_graph_next_main_event(self._h, int(pos_in_frames)))
        return None if t == 0xFFFFFFFFFFFFFFFF else t

    def synchronize(self):
        self._check(self._lib.pg_graph_synchronize(self._h))

    def voice_count(self):
        return self._lib.pg_graph_voice_count(self._h)

    def deferred_units(self):
        """Units the time-parallel kernels handed to the exact serial kernel in the last block (0 in steady state)."""
        return self._id(self._lib.pg_graph_deferred_units(self._h))

    def kernel_ms(self, reset=True):
        """(average ms of the unit kernel per launch, launches) since the last reset, from hipEvents on the graph's stream."""
        n = C.c_uint64(0)
        ms = self._lib.pg_graph_kernel_ms(self._h, 1 if reset else 0, C.byref(n))
        return ms, n.value

    def kernel_stats(self, reset=True):
        """(average ms per timed launch of the dominant kernel, timed launches, blocks those launches rendered): a super-block launch
        renders several max_frames blocks per unit."""
        ms, n, b = C.c_double(0.0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.pg_graph_kernel_stats(self._h, 1 if reset else 0, C.byref(ms), C.byref(n), C.byref(b)))
        return (ms.value / n.value if n.value else 0.0), n.value, b.value

    def bus_kernel_stats(self, reset=True):
        """The same for the launches of the main mixer's effect chain: (average ms per timed bus launch, timed launches, blocks they walked)."""
        ms, n, b = C.c_double(0.0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.pg_graph_bus_kernel_stats(self._h, 1 if reset else 0, C.byref(ms), C.byref(n), C.byref(b)))
        return (ms.value / n.value if n.value else 0.0), n.value, b.value

    def dynamic_stats(self, reset=True):
        """{unit_blocks, deferred_unit_blocks, generic_launches, generic_launches_with_work, generic_ms, generic_timed}: what leaving the
        steady state cost since the last reset (pg_graph_dynamic_stats; waits for the stream)."""
        out = (C.c_uint64 * 4)()
        ms, n = C.c_double(0.0), C.c_uint64(0)
        self._check(self._lib.pg_graph_dynamic_stats(self._h, 1 if reset else 0, out, C.byref(ms), C.byref(n)))
        return {"unit_blocks": int(out[0]), "deferred_unit_blocks": int(out[1]), "generic_launches": int(out[2]), "generic_launches_with_work": int(out[3]),
                "generic_ms": ms.value, "generic_timed": int(n.value)}

    def bus_kernel(self):
        return self._lib.pg_graph_bus_kernel(self._h).decode()

    def set_timing_period(self, every_n_rounds):
        """Time every n-th round with a hipEvent pair (the pair costs ~8 us of stream time); 0 = never."""
        self._check(self._lib.pg_graph_set_timing_period(self._h, int(every_n_rounds)))

    def dominant_kernel(self):
        """Name(s) of the kernel launch(es) that `kernel_ms` brackets for this graph."""
        return self._lib.pg_graph_dominant_kernel(self._h).decode()

    def set_fast_math(self, level):
        self._check(self._lib.pg_graph_set_fast_math(self._h, int(level)))

    def set_staged(self, mode):
        """[Gain|Panning]* -> Reverb sub-mixers: 1/True = staged single launch (default), 2 = one launch per stage, 0/False = fused fast kernel."""
        self._check(self._lib.pg_graph_set_staged(self._h, int(mode)))


class ShardedGraph(GraphHandle):
    """The main mixer spread over several devices behind ONE handle (pg_sharded_*, include/phonic_gpu.h): every call of `GraphHandle` for
    building, automation and `write`, under the name pg_sharded_<call>; sub-mixers and main-mixer sources are placed on the least loaded
    shard, the main mixer's effects run on the root behind the sum of the shards' partial buses. Here: only what the plain graph does not
    have, or takes differently."""

    def __init__(self, devices, sample_rate=48000, channels=2, max_frames=4096):
        self._lib, self._p = _capi.load(), "pg_"
        self.sample_rate, self.channels, self.max_frames = sample_rate, channels, max_frames
        arr = (C.c_int * len(devices))(*devices)
        self._h = self._lib.pg_sharded_create(sample_rate, channels, max_frames, arr, len(devices))
        if not self._h:
            raise PhonicError(_capi.PG_ERR_DEVICE, self._err())

    def _fn(self, name):
        assert name.startswith("graph_"), name
        return getattr(self._lib, "pg_sharded_" + name[len("graph_"):])

    def shard_count(self):
        return self._lib.pg_sharded_shard_count(self._h)

    def shard_of_mixer(self, mixer_id):
        return self._id(self._lib.pg_sharded_shard_of_mixer(self._h, mixer_id))

    def set_reduce(self, mode):
        """REDUCE_PEER_COPY (default) or REDUCE_RCCL (ncclReduce over xGMI; one device per shard). Raises with RCCL's error text on failure."""
        if int(mode) == _capi.REDUCE_RCCL:
            _capi.preload_rccl()
        self._check(self._lib.pg_sharded_set_reduce(self._h, int(mode)))

    def reduce_mode(self):
        return self._lib.pg_sharded_reduce_mode(self._h)

    def read_granular_buffer(self, buffer_id, shard=-1):
        """The granular mono buffer as shard `shard` holds it (-1: the first shard that holds the buffer)."""
        n = self._id(self._lib.pg_sharded_read_granular_buffer(self._h, buffer_id, shard, None, 0))
        out = np.zeros(n, np.float32)
        self._id(self._lib.pg_sharded_read_granular_buffer(self._h, buffer_id, shard, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def sample_buffer_waveform(self, *args, **kwargs):
        raise NotImplementedError("the sharded handle takes no waveform overviews: take them from a single-device Graph that holds the buffer")

    def write_device(self, d_out_ptr, n_samples, pos_in_frames):
        return self._lib.pg_sharded_write_device(self._h, C.c_void_p(d_out_ptr), n_samples, pos_in_frames)

    def set_max_blocks_per_launch(self, n_blocks):
        self._check(self._lib.pg_sharded_set_max_blocks_per_launch(self._h, int(n_blocks)))

    def synchronize(self):
        self._check(self._lib.pg_sharded_synchronize(self._h))

    def device_errors(self):
        return self._id(self._lib.pg_sharded_device_errors(self._h))


def hip_calls():
    """Process-wide counters of the library's own HIP calls: dict(alloc, free, sync, blocking_copy) — see pg_debug_hip_calls."""
    out = (C.c_uint64 * 4)()
    _capi.load().pg_debug_hip_calls(out)
    return dict(alloc=out[0], free=out[1], sync=out[2], blocking_copy=out[3])


def sampler_parameters():
    """The four base parameter descriptors of the Sampler (Sampler::base_parameters()), as effect_parameters returns them."""
    lib = _capi.load()
    out = []
    for i in range(lib.pg_sampler_param_count()):
        d = _capi.ParamDesc()
        if lib.pg_sampler_param(i, C.byref(d)) != 0:
            raise PhonicError(_capi.PG_ERR_NOT_FOUND, "parameter")
        out.append(dict(fourcc=d.fourcc, type=d.type, min=d.min, max=d.max, default=d.default_value, scaling=d.scaling,
                        scaling_args=(d.scaling_arg0, d.scaling_arg1), n_values=d.n_values, name=d.name.decode()))
    return out


def sampler_envelope_parameters():
    """The five envelope parameter descriptors of the Sampler (Sampler::envelope_parameters()), as effect_parameters returns them."""
    lib = _capi.load()
    out = []
    for i in range(lib.pg_sampler_envelope_param_count()):
        d = _capi.ParamDesc()
        if lib.pg_sampler_envelope_param(i, C.byref(d)) != 0:
            raise PhonicError(_capi.PG_ERR_NOT_FOUND, "parameter")
        out.append(dict(fourcc=d.fourcc, type=d.type, min=d.min, max=d.max, default=d.default_value, scaling=d.scaling,
                        scaling_args=(d.scaling_arg0, d.scaling_arg1), n_values=d.n_values, name=d.name.decode()))
    return out


def effect_parameters(kind):
    """`Effect::parameters()` descriptors of an effect kind."""
    lib = _capi.load()
    out = []
    for i in range(lib.pg_effect_kind_param_count(kind)):
        d = _capi.ParamDesc()
        if lib.pg_effect_kind_param(kind, i, C.byref(d)) != 0:
            raise PhonicError(_capi.PG_ERR_NOT_FOUND, "parameter")
        out.append(dict(fourcc=d.fourcc, type=d.type, min=d.min, max=d.max, default=d.default_value, scaling=d.scaling,
                        scaling_args=(d.scaling_arg0, d.scaling_arg1), n_values=d.n_values, name=d.name.decode()))
    return out
