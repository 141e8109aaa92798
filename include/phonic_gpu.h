/*
 * phonic_gpu.h — C ABI of the MI355X-native phonic DSP hot path.
 *
 * This is the drop-in boundary: a Rust shim (`impl Effect`, `impl Source`,
 * see INTEGRATION.md) binds exactly these entry points. Every function cites the reference
 * interface it replaces (paths relative to the reference repo, emuell/phonic v0.16.0).
 *
 * Conventions
 *   - audio buffers are interleaved f32; all stock effects and the graph are stereo
 *     (reference: `enforce_stereo_playback`, src/player.rs:134,179).
 *   - threading (reference: src/source/mixed.rs:113-194,233-234,294-499): exactly one thread at a time may be inside
 *     process/write of a handle (the reference passes `&mut self`, src/effect.rs:155, src/source.rs:95), and the calls that CHANGE a graph
 *     (pg_graph_add_* / remove_* / move_effect / set_*) belong to that owner too. The CONTROL calls — pg_graph_schedule_param,
 *     pg_graph_schedule_reset, pg_graph_set_voice_volume / _panning / _speed, pg_graph_seek_voice, pg_graph_stop_voice,
 *     pg_graph_stop_all_voices — may be called from ANY thread at ANY time, concurrently with write and with each other: like the
 *     reference's handles they only push a record into a lock-free queue (PG_ERR_QUEUE_FULL when 65536 records wait), which write drains
 *     at its top exactly like MixedSource::process_messages.
 *   - all functions returning `int` return a pg_status; the message of the last failure
 *     on the calling thread is available from pg_last_error_message().
 *   - host/device allocations happen in create/initialize/add_* / set_* only (grow-by-doubling); process/write allocate nothing,
 *     free nothing and — on a caller's stream — never wait for the device (reference: assert_no_alloc, src/output/cpal.rs:712-715;
 *     checked with pg_debug_hip_calls). The graph-changing calls first wait for the work of earlier writes (also on the caller's
 *     stream the last write used): none of them may run between two asynchronous writes without that wait.
 */
#ifndef PHONIC_GPU_H
#define PHONIC_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error taxonomy: reference `Error` enum (src/error.rs:8-22) ------------------------- */
typedef enum pg_status {
  PG_OK = 0,
  PG_ERR_PARAMETER = 1,   /* Error::ParameterError: unknown FourCC, non-stereo I/O, bad value */
  PG_ERR_NOT_FOUND = 2,   /* Error::EffectNotFoundError / MixerNotFoundError / unknown voice  */
  PG_ERR_QUEUE_FULL = 3,  /* Error::SendError: message queue of a mixer is full               */
  PG_ERR_DEVICE = 4,      /* HIP failure; the handle becomes silent (GuardedSource semantics) */
  PG_ERR_STATE = 5        /* call order violated (e.g. process before initialize)            */
} pg_status;

const char* pg_last_error_message(void);

/* Number of HIP devices visible, or a negative pg_status. */
int pg_device_count(void);

/* ---- effect kinds: the ten stock effects (src/effect/ *.rs) ------------------------------ */
typedef enum pg_effect_kind {
  PG_FX_GAIN = 0,        /* src/effect/gain.rs        "Gain"       */
  PG_FX_PANNING = 1,     /* src/effect/pan.rs         "Panning"    */
  PG_FX_FILTER = 2,      /* src/effect/filter.rs      "Filter"     */
  PG_FX_EQ5 = 3,         /* src/effect/eq5.rs         "Eq5"        */
  PG_FX_DELAY = 4,       /* src/effect/delay.rs       "Delay"      */
  PG_FX_REVERB = 5,      /* src/effect/reverb.rs      "Reverb"     */
  PG_FX_CHORUS = 6,      /* src/effect/chorus.rs      "Chorus"     */
  PG_FX_COMPRESSOR = 7,  /* src/effect/compressor.rs  "Compressor" */
  PG_FX_GATE = 8,        /* src/effect/gate.rs        "Gate"       */
  PG_FX_DISTORTION = 9,  /* src/effect/distortion.rs  "Distortion" */
  PG_FX_KIND_COUNT = 10
} pg_effect_kind;

/* FourCC of a parameter id, e.g. PG_FOURCC('r','o','o','m') == FourCC(*b"room"). */
#define PG_FOURCC(a, b, c, d) \
  ((uint32_t)(uint8_t)(a) << 24 | (uint32_t)(uint8_t)(b) << 16 | (uint32_t)(uint8_t)(c) << 8 | (uint32_t)(uint8_t)(d))

#define PG_MAX_INIT_PARAMS 16

/*
 * Construction-time values of an effect: the `with_parameters(..)` constructors of the
 * reference (e.g. ReverbEffect::with_parameters, src/effect/reverb.rs:154-159). Values are
 * raw (not normalized); enum parameters take the variant index, booleans 0/1. Parameters
 * not listed keep the reference default. n_params == 0 is `Effect::new()`.
 *
 * The reverb draws fpd_l/fpd_r and the 16 vibrato phases from rand::rng()
 * (src/effect/reverb.rs:95-103,532-538); here they are explicit so results are reproducible.
 * vib_phase index = line * 2 + channel, lines in order a..h.
 */
typedef struct pg_effect_init {
  uint32_t n_params;
  uint32_t fourcc[PG_MAX_INIT_PARAMS];
  float value[PG_MAX_INIT_PARAMS];
  uint32_t has_reverb_seeds;
  uint32_t reverb_fpd_l;
  uint32_t reverb_fpd_r;
  double reverb_vib_phase[16];
  /* The Delay's LFO shapes Random and Smooth Random (LfoWaveform, src/utils/dsp/lfo.rs:35-46) draw from `SmallRng::from_os_rng()`
   * (lfo.rs:73): the reference is not reproducible there. Here the generator's state is an explicit input, like the reverb's seeds:
   * rand ^0.9's SmallRng on 64-bit targets is Xoshiro256++ (Blackman / Vigna; state = four u64), `random::<f32>()` = (next_u64() >> 40) *
   * 2^-24 (StandardUniform: the upper 24 bits of next_u32 = the upper 32 of next_u64). `lfo_rng_state` is that state as
   * Effect::initialize finds it (Lfo::new then draws sample_hold, jitter_current, jitter_target from it, lfo.rs:74-76). Without a
   * seed (or with an all-zero state, which xoshiro cannot hold) the state is SplitMix64(0x5EED0000) x 4 — every unseeded Delay then
   * runs the same random sequence. */
  uint32_t has_lfo_seed;
  uint32_t reserved_lfo;
  uint64_t lfo_rng_state[4];
} pg_effect_init;

/* ---- parameter descriptors: `Effect::parameters()` (src/effect.rs:105-111) -------------- */
typedef enum pg_param_type { PG_PARAM_FLOAT = 0, PG_PARAM_ENUM = 1, PG_PARAM_BOOL = 2, PG_PARAM_INTEGER = 3 /* IntegerParameter (src/parameter/integer.rs): min / max / default hold integers */ } pg_param_type;
typedef enum pg_param_scaling {
  PG_SCALE_LINEAR = 0,
  PG_SCALE_EXPONENTIAL = 1, /* src/parameter/scaling.rs:21  arg0 = factor          */
  PG_SCALE_DECIBEL = 2      /* src/parameter/scaling.rs:31  arg0/1 = min_db/max_db */
} pg_param_scaling;

typedef struct pg_param_desc {
  uint32_t fourcc;
  int32_t type;          /* pg_param_type */
  float min, max;        /* float range; for enums 0 .. n_values-1 */
  float default_value;   /* raw default */
  int32_t scaling;       /* pg_param_scaling */
  float scaling_arg0, scaling_arg1;
  int32_t n_values;      /* enum variant count, else 0 */
  const char* name;
} pg_param_desc;

const char* pg_effect_kind_name(int kind);                   /* Effect::name()   src/effect.rs:96 */
int pg_effect_kind_weight(int kind);                         /* Effect::weight() src/effect.rs:101 */
int pg_effect_kind_param_count(int kind);
int pg_effect_kind_param(int kind, int index, pg_param_desc* out);

/* ---- standalone effect: the `Effect` trait (src/effect.rs:86-215) ----------------------- */
typedef struct pg_effect pg_effect;

/* Effect::new()/with_parameters(); `device` = HIP device ordinal. NULL on failure. */
pg_effect* pg_effect_create(int kind, const pg_effect_init* init, int device);
/* Effect::initialize(sample_rate, channel_count, max_frames)  src/effect.rs:113-125 */
int pg_effect_initialize(pg_effect* fx, uint32_t sample_rate, size_t channel_count, size_t max_frames);
/* Effect::process_started / process_stopped  src/effect.rs:127-139 */
int pg_effect_process_started(pg_effect* fx);
int pg_effect_process_stopped(pg_effect* fx);
/* Effect::process(&mut output, time): in place, host buffer, n_samples <= max_frames*channels
 * and a multiple of the channel count (src/effect.rs:141-155). */
int pg_effect_process(pg_effect* fx, float* interleaved, size_t n_samples, uint64_t pos_in_frames);
/* Effect::process_tail(): -1 = None, INT64_MAX = Some(usize::MAX)  src/effect.rs:157-176 */
int64_t pg_effect_tail(pg_effect* fx);
/* Effect::process_parameter_update(id, Raw|Normalized)  src/effect.rs:178-195 */
int pg_effect_set_parameter(pg_effect* fx, uint32_t fourcc, float value, int is_normalized);
/* Effect::process_message(Reset) (ReverbEffectMessage::Reset etc., src/effect/reverb.rs:24-27) */
int pg_effect_message_reset(pg_effect* fx);
void pg_effect_destroy(pg_effect* fx);
/* Test hook (index streams are compared separately from sample values). With out == NULL the effect (re)arms a log of
 * `words` slots, all -1; the following process calls record the floor()-derived ring index of every delay-line read their time-parallel
 * path takes — Reverb: slot ((frame * 8 + line) * 2 + channel) = read_1 of ReverbDelayLine::get (src/effect/reverb.rs:563-570); Delay and
 * Chorus: slot (frame * 2 + channel) = read_idx1 of InterpolatedDelayLine::process (src/utils/dsp/delay.rs:120-133); frame counts from the
 * start of each process call. With out != NULL the log is copied out. */
int pg_effect_debug_index_log(pg_effect* fx, int32_t* out, size_t words);

/* ---- batched mixer graph: `MixedSource` as a `Source` (src/source/mixed.rs, src/source.rs:80-110)
 *
 * Mixer 0 is the main mixer. Sub-mixers (Player::add_mixer, src/player.rs:773-822) hang off
 * the main mixer; each owns its sources and its effect chain and is one GPU workgroup.
 */
typedef struct pg_graph pg_graph;

#define PG_MAIN_MIXER 0
#define PG_REPEAT_FOREVER UINT64_MAX

/* FilePlaybackOptions (src/source/file.rs:34-75) for a preloaded source. */
typedef struct pg_voice_options {
  float volume;            /* default 1.0 */
  float panning;           /* default 0.0, -1..1 */
  double speed;            /* default 1.0 */
  uint64_t repeat;         /* 0 = play once, PG_REPEAT_FOREVER; (Option<usize>: has_repeat) */
  uint32_t has_repeat;     /* 0 = None: forever iff a loop range is set (preloaded.rs:89-95) */
  uint32_t has_loop_range; /* loop_range override in source frames (preloaded.rs:101-104)   */
  uint64_t loop_start, loop_end;
  uint64_t start_time;     /* sample time in output frames at which the source starts       */
  float fade_in_seconds;   /* < 0 or 0 = none                                               */
  float fade_out_seconds;  /* default 0.05 (file.rs:106); < 0 = none                        */
  uint32_t source_rate;    /* output rate the file source itself is created with (PreloadedFileSource::from_shared_buffer(.., sample_rate),
                              preloaded.rs:71-117); 0 = the graph's rate (what Player passes). When it differs, ConvertedSource puts a cubic
                              ResampledSource — 512-frame input / output staging, src/source/resampled.rs:44-152 — between the file source
                              and the channel mapping (src/source/converted.rs:15-45), exactly as for any source whose rate is not the mixer's */
  uint32_t non_transient;  /* 0 (default) = PlayingSource::is_transient (src/source/mixed.rs:34-42,117-123): the mixer drops the source when it is exhausted
                              (mixed.rs:612-616,715) and RemoveAllPendingEvents takes it when it has not started yet (:298-305). 1 = a source the
                              mixer keeps: exhausted, it stays in the list (asked once per chunk, delivering nothing), stop_all_voices does not take it,
                              write never returns 0 for want of sources — until pg_graph_remove_voice. (In the reference: generators; here: a host-fed
                              source the host wants to keep across pauses of its stream.) */
} pg_voice_options;

void pg_voice_options_default(pg_voice_options* opt);

/* MixedSource::new(channel_count, sample_rate) for the main mixer (src/source/mixed.rs:222-264).
 * max_frames (1..=4096) is the kernels' PIECE size — how many frames a workgroup holds in LDS at a time (the staged kernels of reverb-terminated
 * chains take pieces of <= 1024 frames) — and nothing else: a write of any length is walked in the reference's chunks, min(remaining, 4096)
 * frames (MAX_MIX_BUFFER_SAMPLES / 2, src/source/mixed.rs:216) from the call's start and from every main-mixer event (mixed.rs:679-712),
 * whatever max_frames is; a chunk is rendered as pieces of max_frames frames, and everything the reference decides once per chunk — the effect
 * processors' bypass and tail counters (src/source/mixed/effect.rs:56-145), the sub-mixers' silence gate (submixer.rs:47-77), `audible_input`,
 * an effect's own call-end bookkeeping, a source's fader arrival / end-of-file / is_exhausted — is decided once per chunk here too.
 * 1024 is the size the kernels are tuned for; a host with 2048- or 4096-frame callbacks keeps it and gets the same chunk grid as the reference. */
pg_graph* pg_graph_create(uint32_t sample_rate, uint32_t channel_count, size_t max_frames, int device);
void pg_graph_destroy(pg_graph* g);

/* Player::add_mixer(parent = main) -> mixer id > 0 (src/player.rs:773-822). */
int pg_graph_add_mixer(pg_graph* g);
/* Player::add_mixer(parent_mixer_id) (src/player.rs:771-822): the new mixer is a child of `parent_mixer_id` (0 = main mixer); the
 * parent sums its sub-mixers first, then its sources, then runs its effects (MixedSource::write, src/source/mixed.rs:696-703;
 * SubMixerProcessor::process, src/source/mixed/submixer.rs:47-77). PG_ERR_NOT_FOUND for an unknown parent. */
int pg_graph_add_mixer_to(pg_graph* g, int parent_mixer_id);
/* Player::add_effect(effect, mixer) -> effect id >= 0 (src/player.rs:893-939). */
int pg_graph_add_effect(pg_graph* g, int mixer_id, int kind, const pg_effect_init* init);
/* Player::remove_mixer(mixer_id) (src/player.rs:825-867 -> MixerMessage::RemoveMixer to the parent, src/source/mixed.rs:422-424): the
 * sub-mixer leaves its parent at the start of the next write, with its effects, sources and nested sub-mixers (their ids return
 * PG_ERR_NOT_FOUND afterwards). PG_ERR_PARAMETER for the main mixer. */
int pg_graph_remove_mixer(pg_graph* g, int mixer_id);
/* Player::remove_effect(effect_id) (src/player.rs:977-990 -> MixerMessage::RemoveEffect, src/source/mixed.rs:433-440): takes effect at
 * the start of the next write; later calls with this id return PG_ERR_NOT_FOUND. */
int pg_graph_remove_effect(pg_graph* g, int effect_id);
/* Player::move_effect(movement, effect_id, mixer_id) (src/player.rs:942-972 -> MixerMessage::MoveEffect, src/source/mixed.rs:441-462):
 * EffectMovement::Direction(offset) / Start / End (src/player.rs:75-82). PG_ERR_PARAMETER when the effect is not in `mixer_id`. */
#define PG_MOVE_DIRECTION 0
#define PG_MOVE_START 1
#define PG_MOVE_END 2
int pg_graph_move_effect(pg_graph* g, int effect_id, int mixer_id, int movement, int offset);
/* Player::play_file_source(PreloadedFileSource::from_shared_buffer(..), start_time)
 * (src/player.rs:519-602, src/source/file/preloaded.rs:71-117). `pcm` is the decoded interleaved
 * buffer INCLUDING the extra zero frame symphonia decoding appends (file/buffer.rs:103-104);
 * it is copied to the device. Returns a voice (playback) id >= 0. */
int pg_graph_add_voice(pg_graph* g, int mixer_id, const float* pcm, size_t n_frames, uint32_t src_channels,
                       uint32_t src_rate, const pg_voice_options* opt);

/* Player::play_synth_source / any `dyn Source` (MixerMessage::AddSource{source: Box<dyn Source>}, src/source/mixed.rs:117-123;
 * SynthSourceImpl, src/source/synth/common.rs:194-263; streamed files): a source whose samples the HOST produces. The voice is a ring
 * of `capacity_frames` frames (>= 1024) in device memory at the source's own `rate` and channel count (1 or 2); the host keeps it filled
 * with what it pulls from its source (pg_graph_feed_voice), the device reads it where a file voice reads its preloaded buffer, behind
 * the same adapter chain: ResampledSource when `rate` is not the mixer's (src/source/converted.rs:15-45, 512-frame staging), mono ->
 * stereo, volume, panning, start time (`opt`: volume, panning, start_time are used). A short ring read is a source that delivered
 * less (the rest of the block is silent); the voice ends when the host has ended the stream and everything fed has been played, or
 * at a stop. Device ring and pinned staging ring are reserved here: feed and write allocate nothing. Returns a voice id >= 0 (valid
 * for set_voice_volume / _panning / stop_voice / remove_voice like any other; set_voice_speed and seek_voice return PG_ERR_PARAMETER: those
 * exist on FilePlaybackHandle only, src/player/handles/file.rs). In steady state such a voice is rendered by the same time-parallel kernels
 * as a file voice (the ring read is a copy), also inside a write of several blocks. */
int pg_graph_add_stream_voice(pg_graph* g, int mixer_id, uint32_t channels, uint32_t rate, size_t capacity_frames, const pg_voice_options* opt);
/* The next n_frames frames of the host's source (interleaved). Owner thread, before the write that should play them; they reach the
 * device on that write's stream. PG_ERR_QUEUE_FULL (nothing taken) when fed - consumed + n_frames would exceed the capacity, with
 * `consumed` as last reported by pg_graph_stream_voice_consumed. */
int pg_graph_feed_voice(pg_graph* g, int voice_id, const float* frames, size_t n_frames);
/* Source::is_exhausted (src/source.rs:88-93): nothing more will be fed. */
int pg_graph_end_stream_voice(pg_graph* g, int voice_id);
/* Frames of the stream the device has read so far (waits for the graph's work; negative on failure): frees that much ring for feeds. */
int64_t pg_graph_stream_voice_consumed(pg_graph* g, int voice_id);

/* MixerMessage::RemoveSource (src/source/mixed.rs:149-151,400-402): the source leaves its mixer at the start of the next write, at once — no
 * fade-out (stop_voice is the call that fades) — whether transient or not, started or not; events already scheduled for it find no source and
 * are dropped when they come due. Any thread. Later calls with this id return PG_ERR_NOT_FOUND. */
int pg_graph_remove_voice(pg_graph* g, int voice_id);

/* EffectHandle::set_parameter((id, update), sample_time) (src/player/handles/effect.rs:67-95) */
int pg_graph_schedule_param(pg_graph* g, int effect_id, uint32_t fourcc, float value, int is_normalized,
                            uint64_t sample_time);
/* EffectHandle::send_message(Reset, sample_time) */
int pg_graph_schedule_reset(pg_graph* g, int effect_id, uint64_t sample_time);
/* FilePlaybackHandle::set_volume / set_panning / stop (src/player/handles/file.rs) */
int pg_graph_set_voice_volume(pg_graph* g, int voice_id, float volume, uint64_t sample_time);
int pg_graph_set_voice_panning(pg_graph* g, int voice_id, float panning, uint64_t sample_time);
int pg_graph_stop_voice(pg_graph* g, int voice_id, uint64_t sample_time);
/* Player::stop_all_sources() (src/player.rs:1012-1045): stops every playing source from the next write on (with its fade-out) and sends
 * MixerMessage::RemoveAllPendingEvents to every mixer (src/source/mixed.rs:298-305): sources that have not started by then and events
 * scheduled after that write's position are dropped. */
int pg_graph_stop_all_voices(pg_graph* g);
/* FilePlaybackHandle::set_speed(speed, glide) / seek(position) (src/player/handles/file.rs -> MixerMessage::SetSourceSpeed /
 * SeekSource, src/source/mixed.rs:338-383; PreloadedFileSource::set_speed / seek, src/source/file/preloaded.rs:139-192).
 * glide_semitones_per_second <= 0 = no glide (Option<f32>::None). */
int pg_graph_set_voice_speed(pg_graph* g, int voice_id, double speed, float glide_semitones_per_second, uint64_t sample_time);
int pg_graph_seek_voice(pg_graph* g, int voice_id, double position_seconds, uint64_t sample_time);

/* Per-voice AHDSR volume envelope: AhdsrParameters / AhdsrEnvelope (src/utils/ahdsr.rs) as the sampler puts them around every voice chain
 * (src/generator/sampler/voice.rs:28-30, :469-486). Times are f32 seconds — the value Duration::as_secs_f32() returns for the reference's
 * Duration; 0 skips the stage (a rate of f32::MAX, ahdsr.rs:160-169, :205-214, :240-249). Scalings in [-1, 1]: 0 linear, > 0 logarithmic,
 * < 0 exponential (AhdsrParameters::apply_scaling, ahdsr.rs:324-345). As in the reference, a decay scaling only has a range to work on when
 * the attack time is 0: a timed attack leaves target_volume at the sustain level (ahdsr.rs:456-468, :526-542). */
typedef struct pg_ahdsr_params { float attack_s, attack_scaling, hold_s, decay_s, decay_scaling, sustain_level, release_s, release_scaling; } pg_ahdsr_params;
/* AhdsrParameters::default (ahdsr.rs:348-359): attack 10 ms, hold 1 s, decay 500 ms, sustain 0.75, release 1 s, scalings 0 */
void pg_ahdsr_params_default(pg_ahdsr_params* p);
/* SamplerVoice::start (voice.rs:181-184): AhdsrParameters::new_with_scaling(..) + set_sample_rate(graph rate) (ahdsr.rs:75-98, :123-136), then
 * AhdsrEnvelope::note_on(params, 1.0) (ahdsr.rs:402-419). Only before the voice has rendered a frame (PG_ERR_STATE afterwards). Errors as
 * the reference's setters (ahdsr.rs:143-152, :179-188, :224-233, :259-268): a scaling outside [-1, 1], a sustain level outside [0, 1]; also
 * a negative or non-finite time (no Duration holds one) and a null `p` — PG_ERR_PARAMETER, checked before anything touches the device.
 * The envelope multiplies what the voice's panning step wrote (voice.rs:469-486); when it reaches Idle the voice ends with that write
 * (voice.rs:488-495). A unit that holds a living enveloped voice is rendered by the exact kernel. */
int pg_graph_set_voice_envelope(pg_graph* g, int voice_id, const pg_ahdsr_params* p);
/* SamplerVoice::stop (voice.rs:196-212): AhdsrEnvelope::note_off (ahdsr.rs:422-436) at exactly `sample_time` (0: the next write's first frame)
 * — the release runs from the envelope's current level; a voice without an envelope stops there like pg_graph_stop_voice (voice.rs:207-208).
 * Any thread. */
int pg_graph_release_voice(pg_graph* g, int voice_id, uint64_t sample_time);
/* AhdsrEnvelope::stage (ahdsr.rs:389-393): 0 Idle, 1 Attack, 2 Hold, 3 Decay, 4 Sustain, 5 Release; -1: the voice has no envelope (or is
 * gone). Waits for the graph's stream: call it after pg_graph_write / a synchronize. */
int pg_graph_voice_envelope_stage(pg_graph* g, int voice_id);

/* Granular playback voices: a sampler voice in granular mode — GrainPool<100> (src/generator/sampler/granular.rs) driven as
 * SamplerVoice::process drives it (src/generator/sampler/voice.rs:406-432). Rendered on the device by pg_grain_kernel ("Granular
 * voices"); each grain's per-frame stereo terms are the reference's bits, the f32 sum over the grains of a frame runs in ascending slot order.
 * The voice's modulation matrix is pg_graph_set_voice_modulation_matrix below; without one every `*_mod` input of try_trigger_grain /
 * advance_playhead is 0.0 — what a sampler without routings feeds.
 * The granular parameters and the loop range change while the voice plays: pg_graph_set_voice_granular_parameter / _grain_loop_range below.
 * The mono buffer the pool reads is what create_granular_sample_buffer (sampler.rs:908-952) makes of a file: hand it over here as `mono_pcm`, or
 * let the device make it from a sample buffer (pg_graph_add_granular_voice_from_buffer below).
 * The note, voice-allocation and voice-stealing layer of Sampler and its base transpose, finetune, volume and panning parameters exist for pools
 * of such voices too: pg_graph_add_granular_sampler, below. A voice added HERE is a lone one: the host starts it once, a binding drives it with
 * pg_graph_set_voice_speed / _volume / _panning.
 * OUT OF SCOPE for granular voices: AHDSR parameter changes on a running envelope. (The voice's playback-position status events — the start event, a Position per process call,
 * the two Stopped records — are pg_graph_set_voice_status's, below.)
 * pg_granular_params = GranularParameters (granular.rs:241-266): overlap_mode 0 Cloud, 1 Sequential (:35-45); window 0 Hann, 1 Blackman,
 * 2 Triangle, 3 Tukey, 4 Trapezoid, 5 Exponential, 6 RampUp, 7 RampDown (:61-70); size in ms, density in Hz, playback_direction 0 Forward,
 * 1 Backward, 2 Random (:19-26); plus GrainPool::sample_loop_range (:357, voice.rs:355-360) as has_loop_range / loop_start / loop_end,
 * normalised to [0, 1]. rng_state: the pool seeds its SmallRng from the OS (granular.rs:410) — here the state is an input, by the rule of
 * pg_effect_init::lfo_rng_state above: Xoshiro256++, an all-zero state means SplitMix64(0x5EED0000) x 4. The draws are rand 0.9's:
 * random::<f32>() = (next_u64 >> 40) * 2^-24, random::<f64>() = (next_u64 >> 11) * 2^-53, random::<bool>() = the top bit of next_u64 — these
 * three definitions are taken from rand's documentation and are UNVERIFIED against the crate (its source is not part of this project).
 * The window tables' cos / exp and the pitch variation's 2^x are the correctly rounded values, where a libm may be an ulp off. */
typedef struct pg_granular_params {
  int32_t overlap_mode, window;
  float size, density, variation, spray, pan_spread;
  int32_t playback_direction;
  float position, step;
  int32_t has_loop_range;
  float loop_start, loop_end;
  int32_t reserved;
  uint64_t rng_state[4];
} pg_granular_params;
/* GranularParameters::default (granular.rs:268-283): Cloud, Triangle, 100 ms, 10 Hz, no variation / spray / pan spread, Forward, position 0.5,
 * step 0; no loop range, rng_state 0 */
void pg_granular_params_default(pg_granular_params* p);
/* GranularParameters::validate (granular.rs:291-335): size 1..1000, density 1..100, spray / variation / pan_spread / position 0..1, step -4..4;
 * also 0 <= loop_start, loop_end <= 1 (GrainPool::new's assertion, :393-398), enum fields in range, `p` not null. PG_OK or PG_ERR_PARAMETER;
 * touches no graph and no device. */
int pg_granular_params_check(const pg_granular_params* p);
/* A sampler voice in granular mode on mixer `mixer_id`: `mono_pcm` = n_frames >= 1 mono f32 frames at the graph's rate (copied to the device).
 * opt->volume / panning / speed become GrainPool::start(parameters, speed, volume, panning) (granular.rs:474-489); as in the reference's granular
 * branch the output does NOT pass the amplified / panned / fader stages (voice.rs:412-427): volume and panning act through the grains only.
 * opt->start_time works as for file voices; the other options are not used. Returns a voice id >= 0. On such a voice:
 *  - pg_graph_set_voice_volume / _panning / _speed are GrainPool::set_volume / set_panning / set_speed (granular.rs:504-514) at the exact frame,
 *    not smoothed: they reach the grains activated from that frame on (:824-831, :857); a glide is ignored (SamplerVoice::set_speed);
 *  - pg_graph_stop_voice, and pg_graph_release_voice without an envelope, are GrainPool::stop() (:491-493): no new grains; the voice ends with
 *    the chunk (the source's process call) in which the pool became exhausted (:442-444, voice.rs:488-495), which it writes in full;
 *  - pg_graph_set_voice_envelope works as for any voice (before the first frame); then pg_graph_release_voice is the envelope's note_off and the
 *    voice ends on Idle or on exhaustion, whichever comes first;
 *  - pg_graph_seek_voice returns PG_ERR_STATE.
 * A unit that holds a living granular voice is rendered by the exact kernel, which takes pg_grain_kernel's frames as the voice's source output. */
int pg_graph_add_granular_voice(pg_graph* g, int mixer_id, const float* mono_pcm, size_t n_frames, const pg_granular_params* p, const pg_voice_options* opt);
/* Debug read-back of a granular voice's GrainPool (granular.rs:345-377) and its 100 Grain records (:961-985). Waits for the graph's stream.
 * PG_ERR_NOT_FOUND: not a granular voice. */
#define PG_GRAIN_POOL_SIZE 100
typedef struct pg_grain_slot {
  double position, increment, window_phase, window_increment;
  uint64_t samples_remaining;
  float volume, panning;
  int32_t active, window_mode, has_loop_range, reserved;
} pg_grain_slot;
typedef struct pg_grain_state {
  float trigger_phase, playhead;
  int32_t playing_loop_range, trigger_new_grains;
  int32_t primary_slot;      /* primary_grain_index, -1: None */
  int32_t overlap_mode;      /* the pool's own copy (granular.rs:346): Cloud from GrainPool::new (:399) until the first rendered frame takes the parameters' (:535-538) */
  double speed;
  float volume, panning;
  uint64_t rng_state[4];
  pg_grain_slot slots[PG_GRAIN_POOL_SIZE];
} pg_grain_state;
int pg_graph_voice_grain_state(pg_graph* g, int voice_id, pg_grain_state* out);

/* The granular parameters while the voice plays: Sampler::GRAIN_* (src/generator/sampler.rs:219-296), ordinary automatable parameters in the
 * reference — GeneratorPlaybackHandle::set_parameter(id, value, sample_time) -> Sampler::set_granular_parameter (:299-360, :1132-1147) — and the
 * sampler's loop range (SamplerMessage::SetLoopRange, sampler.rs:1246-1270 -> GrainPool::set_loop_range, granular.rs:516-518).
 * pg_granular_param_count / pg_granular_param: the ten descriptors in Sampler::granular_parameters() order — GOVM Overlap Mode, GWND Window,
 * GSIZ Grain Size, GDEN Density, GVAR Variation, GSPY Spray, GPAN Pan Spread, GDIR Direction, GPOS Position, GSTP Step — as the record
 * pg_effect_kind_param returns; they touch no graph and no device. (GWND's descriptor default is Hann; GranularParameters::default() is Triangle.)
 * pg_graph_set_voice_granular_parameter: `fourcc` is one of the ten ids. A raw float value is clamped to the descriptor's range
 * (Sampler::parameter_update_value, sampler.rs:862-883); a normalized one is clamped to 0..1 and denormalized, min + scaling.scale(n) * (max - min)
 * (src/parameter/float.rs:137-141; GSIZ and GDEN scale with Exponential(2.0)). A normalized enum value is (n * (count - 1)).round()
 * (src/parameter/enum.rs:154); a raw enum value is the variant's index, as for pg_graph_schedule_param — one out of range is ignored (PG_OK).
 * pg_graph_set_voice_grain_loop_range: GrainPool::sample_loop_range becomes (loop_start, loop_end), normalised to [0, 1] as in
 * pg_granular_params, or None (has_loop_range 0); it accepts what pg_granular_params_check accepts. Only sample_loop_range changes:
 * playing_loop_range, the playhead and the living grains keep what they have.
 * Both are scheduled like pg_graph_set_voice_modulation: events of the voice's mixer that cut its chunk and act in front of frame `sample_time`
 * (0: the next write's first frame), several at one frame in the order of the calls; any thread. What a change means for the grains is the
 * reference's: a grain keeps the window and the loop range it was activated with (granular.rs:823, :1038-1047); the pool follows a new overlap
 * mode at the next frame and forgets its primary grain (:535-538); the crossfade point is the current window's (:547); `position` places the
 * grains only while step == 0 (:448-452) and the playhead keeps its value while it does. A command in front of the voice's start time changes the
 * parameters, and a new position then is the playhead's too: GrainPool::start reads it at note-on (:487). A voice whose pool has run dry takes no
 * parameters any more. In the reference these calls reach every voice of a Sampler; here they address ONE voice — a binding loops over its voices.
 * PG_ERR_PARAMETER: an unknown fourcc, a NaN value, loop points outside [0, 1] or NaN, a null handle — checked in that order, before anything
 * touches a device; PG_ERR_NOT_FOUND: no such voice, or not a granular voice.
 * pg_graph_voice_granular_params: the parameters and the loop range as the device holds them (rng_state reads 0). Waits for the graph's stream.
 * PG_ERR_NOT_FOUND: not a granular voice. */
int pg_granular_param_count(void);
int pg_granular_param(int index, pg_param_desc* out);
int pg_graph_set_voice_granular_parameter(pg_graph* g, int voice_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time);
int pg_graph_set_voice_grain_loop_range(pg_graph* g, int voice_id, int has_loop_range, float loop_start, float loop_end, uint64_t sample_time);
int pg_graph_voice_granular_params(pg_graph* g, int voice_id, pg_granular_params* out);

/* Sample buffers: one decoded file on the device, played by any number of voices — the reference's Arc<AudioFileBuffer> (src/source/file/buffer.rs),
 * which every PreloadedFileSource::from_shared_buffer / clone (src/source/file/preloaded.rs:71-135) and every voice of a Sampler
 * (src/generator/sampler.rs) plays from. The buffer is uploaded once; voices made from it point at its memory and own none of it.
 * pg_graph_add_sample_buffer: `pcm` is what pg_graph_add_voice takes (interleaved, including symphonia's extra zero frame), copied to the device
 * once. Returns a buffer id >= 0. -PG_ERR_PARAMETER — checked before the handle and before anything touches the device — for a null `pcm`, a null
 * desc, n_frames < 1, channels other than 1 or 2, rate 0, or a loop range with loop_start >= n_frames, loop_end > n_frames or
 * loop_start >= loop_end (AudioFileBuffer::new refuses an empty range, file/buffer.rs:49-55).
 * pg_graph_release_sample_buffer drops the host's reference (Arc semantics): the id returns PG_ERR_NOT_FOUND from then on, voices that play the
 * buffer keep playing, unchanged, and the device memory — the granular mono buffer too, if one was made — is freed when the last such voice's
 * memory is released: like a voice's private copy, in the first graph-changing call after the write that carried the voice's removal to the
 * device (never inside a write), or with pg_graph_destroy. Voices of pg_graph_add_voice keep their private copy.
 * pg_graph_add_voice_from_buffer = PreloadedFileSource::from_shared_buffer(buffer, options, rate): pg_graph_add_voice with the buffer's PCM,
 * channels and rate, and every timed call works on the voice as on any file voice. The buffer's embedded loop range plays the role the reference
 * gives it (preloaded.rs:90-104, :150-156): without a repeat count (has_repeat == 0) the voice repeats forever iff the buffer has a loop range;
 * the active loop range is opt's override if set, else the buffer's.
 * pg_graph_add_granular_voice_from_buffer = pg_graph_add_granular_voice with the buffer's granular mono buffer: what
 * Sampler::create_granular_sample_buffer (sampler.rs:908-952) makes of the file — a temporary PreloadedFileSource at the graph's rate (default
 * options, repeat(0), cubic resampler) pulled in writes of 1024 frames until one returns 0, each frame the f32 sum of its channels divided by
 * their count; a single 0.0 if nothing came. It is made on the device (pg_sample_sched_kernel + pg_sample_interp_kernel, DESIGN.md "Sample
 * buffers") on first use, or earlier by pg_graph_prepare_granular_buffer (a no-op once it exists), once per buffer, shared by all its granular
 * voices as Sampler::new shares its Arc<Box<[f32]>>; a mono buffer at the graph's rate IS its granular buffer (sampler.rs:912-914: no copy
 * here). Every sample equals the reference's; an all-zero frame's sum may differ in the sign of its zero (the identity of the Rust release's
 * f32 Sum). If p->has_loop_range == 0 and the buffer carries a loop range, the pool's sample_loop_range is (start as f32 / n_frames as f32,
 * end as f32 / n_frames as f32) (voice.rs:355-360). Conversion with ResamplingQuality::HighQuality (rubato) is out of scope.
 * pg_graph_sample_buffer_info: use_count = voices holding the buffer; granular_frames = -1 while the granular buffer has not been made.
 * pg_graph_read_granular_buffer: debug read-back of up to cap_frames frames; returns the granular buffer's length (negative: -PG_ERR_*); makes the
 * buffer if it is not there. All calls: owner thread; the graph-changing ones wait for the work of earlier writes. */
typedef struct pg_sample_buffer_desc {
  uint32_t channels;        /* 1 or 2 */
  uint32_t rate;            /* > 0 */
  uint32_t has_loop_range;  /* AudioFileBuffer::loop_range(), the file's embedded loop */
  uint32_t reserved;
  uint64_t loop_start, loop_end;   /* source frames */
} pg_sample_buffer_desc;
typedef struct pg_sample_buffer_info {
  uint64_t n_frames;
  uint32_t channels, rate;
  uint32_t has_loop_range;
  int32_t use_count;
  uint64_t loop_start, loop_end;
  int64_t granular_frames;
} pg_sample_buffer_info;
int pg_graph_add_sample_buffer(pg_graph* g, const float* pcm, size_t n_frames, const pg_sample_buffer_desc* desc);
int pg_graph_release_sample_buffer(pg_graph* g, int buffer_id);
int pg_graph_add_voice_from_buffer(pg_graph* g, int mixer_id, int buffer_id, const pg_voice_options* opt);
int pg_graph_add_granular_voice_from_buffer(pg_graph* g, int mixer_id, int buffer_id, const pg_granular_params* p, const pg_voice_options* opt);
int pg_graph_prepare_granular_buffer(pg_graph* g, int buffer_id);
int pg_graph_sample_buffer_info(pg_graph* g, int buffer_id, pg_sample_buffer_info* out);
int64_t pg_graph_read_granular_buffer(pg_graph* g, int buffer_id, float* out, size_t cap_frames);

/* Waveform overviews of a sample buffer: phonic::utils::waveform::mixed_down / multi_channel (src/utils/waveform.rs:95-199) over the copy the
 * device already holds — min / max pairs per display column, so that a host that draws a sample keeps no second copy of its PCM and reads none
 * back. A display helper, NOT a real-time call: it runs on the owner thread, waits for the work of earlier writes, allocates its staging memory,
 * launches (pg_waveform_*_kernel, DESIGN.md "Waveform overviews"), waits for the result and frees the memory again. It may be called between
 * writes while voices play the buffer: it reads immutable memory and changes nothing a later write renders.
 * The slice is frames [first_frame, first_frame + n_frames) of the source — the `&buffer[a * ch .. b * ch]` a caller of the reference passes
 * when it zooms; `frame` and `time` count from the slice's start. PG_WAVEFORM_OF_FILE: the buffer as uploaded (AudioFileBuffer::buffer(), the
 * decoder's extra zero frame included), with the buffer's channel count and rate. PG_WAVEFORM_OF_GRANULAR: the buffer's granular mono buffer
 * (made if it is not there, as pg_graph_read_granular_buffer does — a graph-changing step), one channel at the graph's rate.
 * Returns the number of points per channel, P = min(n_frames, resolution), or -PG_ERR_*. PG_WAVEFORM_MIXED_DOWN writes P points;
 * PG_WAVEFORM_MULTI_CHANNEL writes channels * P points, channel-major: out[c * P + i]. Every value is the reference's, operation for operation
 * (the sign of a zero aside): n_frames <= resolution gives one point per frame with min == max; otherwise step = n_frames as f32 / resolution
 * as f32 and point i covers frames [b(i), b(i + 1)), b(i) = min((i as f32 * step) as usize, n_frames) — one rounded f32 product, truncated —
 * with frame = b(i) before the clamp; a point that covers no frame, or only NaN samples, keeps min = FLT_MAX, max = -FLT_MAX (f32::MAX,
 * f32::MIN); the mono value of a frame is the fold 0.0 + l / ch + r / ch in channel order, each sample divided first; a NaN sample is skipped.
 * -PG_ERR_PARAMETER, answered before the handle and before anything touches the device: a null `out`, resolution == 0, n_frames == 0, a `source`
 * or `mode` outside the two values, cap_points < P. Then: a null handle (-PG_ERR_PARAMETER, "graph handle is null"), an unknown or released
 * buffer (-PG_ERR_NOT_FOUND), a slice that leaves the source, or cap_points < channels * P for PG_WAVEFORM_MULTI_CHANNEL (-PG_ERR_PARAMETER;
 * 2 * P always suffices, P does for a mono source). Nothing is written to `out` when the call fails.
 * The sharded handle has no such call on purpose: a host that holds one takes overviews from a single-device graph (pg_graph_create) to which it
 * has added the buffer. */
#define PG_WAVEFORM_MIXED_DOWN    0   /* waveform::mixed_down    (waveform.rs:95-140)  */
#define PG_WAVEFORM_MULTI_CHANNEL 1   /* waveform::multi_channel (waveform.rs:149-199) */
#define PG_WAVEFORM_OF_FILE       0   /* the buffer as uploaded: AudioFileBuffer::buffer(), the decoder's extra zero frame included */
#define PG_WAVEFORM_OF_GRANULAR   1   /* the buffer's granular mono buffer at the graph's rate (made if it is not there, as pg_graph_read_granular_buffer does) */
typedef struct pg_waveform_point {   /* waveform::Point; 24 bytes */
  uint64_t frame;   /* frame_index inside the slice this point starts at */
  float time;       /* frame as f32 / rate as f32, seconds: the argument the reference gives Duration::from_secs_f32 (the binding converts) */
  float min, max;
  uint32_t reserved;  /* 0 */
} pg_waveform_point;
int64_t pg_graph_sample_buffer_waveform(pg_graph* g, int buffer_id, int source, int mode, uint64_t first_frame, uint64_t n_frames, uint32_t resolution,
                                        pg_waveform_point* out, size_t cap_points);

/* The modulation matrix of a granular voice: the ModulationMatrix every granular sampler voice owns (src/generator/sampler/voice.rs:341-373,
 * src/modulation/matrix.rs, src/generator/sampler/modulation.rs), run in front of the grain engine (voice.rs:412-427) — on the device as phase 0
 * of pg_grain_kernel ("Granular voices", Modulation). Sources in the matrix's slot order (sampler.rs:362-416): 0 LFO 1 (`LFO1`,
 * 1 Hz Sine), 1 LFO 2 (`LFO2`, 2 Hz Triangle), 2 velocity (`VELM`), 3 keytracking (`KEYM`). Targets in Sampler::modulation_config's order
 * (sampler.rs:417-425): 0 GRAIN_SIZE, 1 GRAIN_DENSITY, 2 GRAIN_VARIATION, 3 GRAIN_SPRAY, 4 GRAIN_PAN_SPREAD, 5 GRAIN_POSITION, 6 GRAIN_STEP.
 * Per target and frame the sum starts at 0.0 and takes the slots in that order, each only if it routes to the target (matrix.rs:194-303), in
 * f32: an LFO adds v * amount to a bipolar target and ((v + 1) / 2) * amount to a unipolar one; velocity (the note's volume) and keytracking
 * (note / 127) add ((v - 0.5) * 2) * amount to a bipolar target and v * amount to a unipolar one. The sums enter the pool as granular.rs writes
 * them: density * (1 + mod) clamped to 1..100 (:798-799), spray + mod clamped to 0..1 (:565), position + mod when mod != 0, in front of the
 * loop fold (:455-471), variation + mod clamped to 0..1 (:827), size * (1 + mod) clamped to 1..1000 (:848-849), pan spread + mod clamped to
 * 0..1 (:855), step * (1 + mod) (:609-613). The LFOs are src/utils/dsp/lfo.rs with all seven shapes; their generators follow the rule of
 * pg_granular_params::rng_state above (Xoshiro256++ state as an input, all-zero = SplitMix64(0x5EED0000) x 4, random::<f32>() as defined there
 * and as UNVERIFIED against the crate). The matrix advances on the frames the voice renders only: not in front of its start time, not after it
 * has ended. A release touches no modulation source (note_off reaches envelope slots, and the sampler has none, sampler/modulation.rs:101-103).
 * In the reference the timed calls below reach every voice of a Sampler; here they address ONE voice — a binding loops over its voices.
 * OUT OF SCOPE: envelope modulation sources and the FunDSP generator's matrix. (The note layer of a granular-mode Sampler: pg_graph_add_granular_sampler.)
 * (pg_modulation_state::last[5] is the value a granular voice's Position records use, voice.rs:435-446: pg_graph_set_voice_status.) (The granular parameters
 * themselves change through pg_graph_set_voice_granular_parameter above; a route's sum applies to the parameter's value as of its frame.) */
#define PG_MOD_SOURCES 4
#define PG_MOD_TARGETS 7
typedef struct pg_mod_lfo   { float rate_hz; int32_t waveform; uint64_t rng_state[4]; } pg_mod_lfo;   /* waveform: LfoWaveform 0..6 (lfo.rs:35-47): Sine, Triangle, RampUp, RampDown, Square, Random, SmoothRandom */
typedef struct pg_mod_route { float amount; int32_t bipolar; } pg_mod_route;                          /* ModulationProcessorTarget (processor.rs); amount 0: no route */
typedef struct pg_modulation_params {
  pg_mod_lfo lfo[2];
  float velocity;      /* SamplerVoice::start's per-note `volume`, 0..1 — NOT the effective volume handed to GrainPool::start */
  int32_t note;        /* 0..127 */
  pg_mod_route routes[PG_MOD_SOURCES][PG_MOD_TARGETS];
} pg_modulation_params;
/* Sampler::modulation_config's defaults (sampler.rs:369-390): 1 Hz Sine, 2 Hz Triangle; velocity 1.0, note 60, no routes, rng states 0 */
void pg_modulation_params_default(pg_modulation_params* p);
/* ModulationState::set_modulation's errors (src/modulation/state.rs:195-201) for every route: an amount outside [-1, 1] or NaN; a waveform outside
 * 0..6; a NaN rate (other rates are clamped to 0.01..=20.0 like the reference's raw parameter update, sampler.rs:870-874, :369-384); a velocity
 * outside [0, 1]; a note outside 0..127; a null `p`. PG_OK or PG_ERR_PARAMETER; touches no graph and no device. */
int pg_modulation_params_check(const pg_modulation_params* p);
/* SamplerVoice::enable_granular_playback's create_matrix (voice.rs:341-373, src/modulation/state.rs:91-156: each Lfo::new draws its three random
 * values at the default rate and waveform), then the rates, waveforms and routes of `p` (Lfo::set_rate / set_waveform change nothing else,
 * lfo.rs:102-119; a route with |amount| < 0.001 is not added, matrix.rs:60-83), then SamplerVoiceModulationState::start(note, velocity) =
 * ModulationMatrix::note_on (matrix.rs:394-408): both LFOs reset (lfo.rs:89-99: phase 0; Random and SmoothRandom draw again). Granular voices
 * only (PG_ERR_NOT_FOUND otherwise); only before the voice has rendered a frame (PG_ERR_STATE afterwards). A granular voice without this call has
 * no matrix and nothing about it changes. */
int pg_graph_set_voice_modulation_matrix(pg_graph* g, int voice_id, const pg_modulation_params* p);
/* GeneratorPlaybackHandle::set_modulation / clear_modulation (player/handles/generator.rs:337-430, sampler.rs:694-720; ModulationMatrixSlot::
 * update_target, matrix.rs:60-83: |amount| < 0.001 removes the route) and set_parameter(ML1R | ML2R) / (ML1W | ML2W) (sampler.rs:1148-1186; the
 * rate is clamped to 0.01..=20.0). Scheduled like pg_graph_set_voice_volume: events of the voice's mixer that cut its chunk and act in front of
 * frame `sample_time` (0: the next write's first frame); any thread. clear is set with amount 0. PG_ERR_PARAMETER: an index out of range, an
 * amount outside [-1, 1] or NaN, a NaN rate; PG_ERR_NOT_FOUND: no such voice; PG_ERR_STATE: the voice has no matrix. */
int pg_graph_set_voice_modulation(pg_graph* g, int voice_id, int source, int target, float amount, int bipolar, uint64_t sample_time);
int pg_graph_clear_voice_modulation(pg_graph* g, int voice_id, int source, int target, uint64_t sample_time);
int pg_graph_set_voice_lfo_rate(pg_graph* g, int voice_id, int lfo, float rate_hz, uint64_t sample_time);
int pg_graph_set_voice_lfo_waveform(pg_graph* g, int voice_id, int lfo, int waveform, uint64_t sample_time);
/* Debug read-back of the matrix: per LFO the fields of Lfo (lfo.rs:52-60), the two static sources, the 4 x 7 routes as the matrix holds them (a
 * removed route reads amount 0, bipolar 0) and last[7], the seven sums of the last rendered frame (what voice.rs:435-446 reads with
 * output_at(.., output_size - 1)), all 0 before the first frame. Waits for the graph's stream. PG_ERR_NOT_FOUND: not a granular voice;
 * PG_ERR_STATE: no matrix. */
typedef struct pg_mod_lfo_state { float phase, phase_inc, sample_hold, jitter_current, jitter_target; int32_t waveform; uint64_t rng_state[4]; } pg_mod_lfo_state;
typedef struct pg_modulation_state {
  pg_mod_lfo_state lfo[2];
  float velocity, note_pitch;
  pg_mod_route routes[PG_MOD_SOURCES][PG_MOD_TARGETS];
  float last[PG_MOD_TARGETS];
  int32_t reserved;
} pg_modulation_state;
int pg_graph_voice_modulation_state(pg_graph* g, int voice_id, pg_modulation_state* out);

/* The Sampler generator's note layer: notes, voice allocation and voice stealing (src/generator/sampler.rs, src/generator/sampler/voice.rs) for
 * file-playback samplers. A sampler is a fixed pool of voice_count file voices of ONE sample buffer in a SUB-mixer; it takes note_on / note_off
 * and the other GeneratorPlaybackEvents at sample times, picks a free voice or steals one, restarts it and composes the note's pitch, volume and
 * panning with its base parameters. The layer runs on the device (pg_sampler_dev.h, DESIGN.md "Sampler"): which slot a note gets depends on which
 * voices still play and which release at exactly the note's frame, and that is decided by the kernel that renders them.
 *   messages     are applied at the top of the Sampler::write that follows them (process_playback_messages, sampler.rs:656-731); the owning mixer
 *                cuts its chunk at the message's sample time (mixed.rs:679-712, :902-918), so each acts in front of exactly that frame
 *                (sample_time 0: the next write's first frame, as for pg_graph_release_voice). Several at one frame: in the order of the calls.
 *   allocation   next_free_voice_index (sampler.rs:826-860): the first slot that is not active; else, with an envelope, the slot in Release with the
 *                smallest release_start_frame; else the active slot with the smallest note id. A voice that fades out after a note-off WITHOUT
 *                an envelope is not "releasing" under this rule. Ties go to the lower slot.
 *   start        SamplerVoice::start (voice.rs:122-193): an active slot's file source is killed without a fade (preloaded.rs:212-230); speed =
 *                speed_from_note(note) * 2^(transpose / 12 + finetune / 1200) in f64 (utils.rs:67-78), no glide; volume target = base_volume *
 *                volume, panning target = clamp(base_panning + panning, -1, 1) — set_target calls on the two exponential smoothers, which are NOT
 *                reset: a reused slot ramps from what the previous note left, a fresh one from 1.0 / 0.0 (voice.rs:60-65, amplified.rs:60-62);
 *                AhdsrEnvelope::note_on(params, 1.0) (ahdsr.rs:402-419) with an envelope.
 *   stop         SamplerVoice::stop (voice.rs:196-219), on an active slot only: release_start_frame = the current frame (also when the slot
 *                releases already); with an envelope note_off, which restarts the release from the current level; without one the file source's
 *                stop(): the 50 ms fade-out every sampler voice is built with (sampler.rs:513-514).
 *   free         a slot becomes free in the source write in which its file is exhausted, its fade-out arrives or its envelope is Idle
 *                (voice.rs:488-502), not earlier and not later.
 *   sum          the active voices in slot order (sampler.rs:989-1006).
 * pg_sampler_options: voice_count 1..=64, default 8 (generator.rs:48-72; the cap of 64 is THIS implementation's: one wave lane per slot);
 * has_envelope + envelope: Sampler::with_ahdsr, checked like pg_graph_set_voice_envelope's; has_loop_range + loop_start / loop_end (source
 * frames): Sampler::set_loop_range before playback, every voice then repeats forever (voice.rs:313-328) — without it the buffer's embedded loop
 * range applies as for pg_graph_add_voice_from_buffer; transient: 1 = Player::play_generator (player.rs:708-718), 0 = add_generator; start_time.
 * pg_sampler_options_default / _check touch no graph and no device; _check: PG_OK or PG_ERR_PARAMETER with a message (null options, voice_count
 * outside 1..=64, envelope errors, loop_start >= loop_end).
 * pg_graph_add_sampler: returns a sampler id >= 0. -PG_ERR_PARAMETER for mixer_id == PG_MAIN_MIXER (see OUT OF SCOPE) and a loop range outside the
 * buffer; -PG_ERR_NOT_FOUND for an unknown mixer or buffer. Every pool voice holds a reference on the sample buffer, like any voice made from it.
 * The pool's voices carry no public voice id. Owner thread; waits for earlier writes like every graph-changing call.
 * pg_graph_remove_sampler: MixerMessage::RemoveSource — the pool leaves the mixer at the start of the next write, at once; its buffer references
 * return like those of removed voices; queued messages for it are dropped when they come due. Any thread.
 * The timed messages (any thread, through the control ring: PG_ERR_QUEUE_FULL applies instead of the reference's 54-entry queue with force_push):
 *   pg_graph_sampler_note_on       returns the note id: positive, strictly increasing per graph (unique_note_id, generator.rs:32), below 2^31
 *                                  (-PG_ERR_STATE beyond). -PG_ERR_PARAMETER: a negative or non-finite volume, a non-finite panning, a null handle.
 *   pg_graph_sampler_note_off / _set_note_speed / _set_note_volume / _set_note_panning   reach the FIRST slot in index order that plays the note
 *                                  (sampler.rs:776-822); an unknown or ended note id is ignored. speed > 0 and finite, composed with the base pitch
 *                                  (voice.rs:239-254); glide_semitones_per_second <= 0: none. Volume >= 0, panning finite (composed and clamped).
 *   pg_graph_sampler_all_notes_off stops every active slot.
 *   pg_graph_sampler_set_parameter the base parameters, sampler.rs:1076-1120: STRN Transpose (integer -48..48, 0), SFTN Finetune (integer -100..100,
 *                                  0), SVOL Volume (0.000001..15.848932, 1.0, Decibel(-60, 24)), SPAN Panning (-1..1, 0.0). The host resolves the
 *                                  value as parameter_update_value / _integer do (sampler.rs:862-906): raw values are clamped (integers truncated
 *                                  first), normalized ones denormalized (integers rounded, integer.rs:121-126). The stored base value changes and
 *                                  every ACTIVE voice is recomputed; a pitch change ends a glide. PG_ERR_PARAMETER: an unknown FourCC, a NaN, a
 *                                  normalized value outside [0, 1] (player/handles/generator.rs:342-348).
 *   pg_graph_sampler_stop          Sampler::stop (sampler.rs:733-738): all notes off; a transient sampler is `stopping` from then on, drops every
 *                                  later message, becomes `stopped` in the first write that ends with no active slot (:1011-1024) and leaves the
 *                                  mixer (its id returns PG_ERR_NOT_FOUND once the host has seen that, at the top of a later write).
 * pg_sampler_param_count / pg_sampler_param: the four descriptors in Sampler::base_parameters() order (PG_PARAM_INTEGER for the first two).
 * pg_graph_sampler_state: debug read-back; waits for the graph's work like pg_graph_voice_envelope_stage. Per slot: note_id (0 = free), and note,
 * note_volume, note_panning of the slot's last note; envelope_stage (-1 without an envelope); release_start_frame (UINT64_MAX = none).
 * An id of a removed or never-created sampler: PG_ERR_NOT_FOUND. A null handle: PG_ERR_PARAMETER ("graph handle is null"), after the argument checks.
 * A unit that holds a sampler is rendered by the exact kernel for as long as the sampler lives.
 * The sharded handle has NO sampler entry points yet (tests/test_host_sharded_routing.py counts the header's handle-taking pg_sharded_* functions
 * against its fixed program): they follow in a change that may touch that program.
 * OUT OF SCOPE: the main mixer through THIS entry point (a sampler there is one source unit that holds the whole pool, behind the generator's
 * output stage: pg_graph_add_sampler_to_main, below); the AMP_* envelope ids through pg_graph_sampler_set_parameter (they have a call and a table
 * of their own: pg_graph_sampler_set_envelope_parameter, below); SetLoopRange on a file sampler while it plays; playback status events of sampler
 * voices and the sampler's own Stopped event; GeneratorPlaybackOptions::volume / panning for a sampler in a sub-mixer (identity at their defaults,
 * smoothing.rs:60-71, :98-101; with other values: pg_graph_add_sampler_to_main).
 * (Granular-mode samplers, Sampler::with_granular_playback: pg_graph_add_granular_sampler, below.) */
#define PG_SAMPLER_MAX_VOICES 64
typedef struct pg_sampler_options {
  uint32_t voice_count;      /* 1..=64, default 8 */
  uint32_t has_envelope;     /* Sampler::with_ahdsr */
  pg_ahdsr_params envelope;
  uint32_t has_loop_range;   /* Sampler::set_loop_range before playback, source frames */
  uint32_t transient;        /* 1 = play_generator, 0 = add_generator (default) */
  uint64_t loop_start, loop_end;
  uint64_t start_time;
} pg_sampler_options;
typedef struct pg_sampler_slot_state {
  int64_t note_id;               /* 0 = free */
  uint64_t release_start_frame;  /* UINT64_MAX = none */
  float note_volume, note_panning;
  int32_t note;
  int32_t envelope_stage;        /* AhdsrStage 0..5, -1 without an envelope */
} pg_sampler_slot_state;
typedef struct pg_sampler_state {
  int32_t voice_count, active_voices;
  int32_t stopping, stopped;
  int32_t transpose, finetune;
  float volume, panning;
  pg_sampler_slot_state slots[PG_SAMPLER_MAX_VOICES];
} pg_sampler_state;
void pg_sampler_options_default(pg_sampler_options* opt);
int pg_sampler_options_check(const pg_sampler_options* opt);
int pg_sampler_param_count(void);
int pg_sampler_param(int index, pg_param_desc* out);
int pg_graph_add_sampler(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt);
int pg_graph_remove_sampler(pg_graph* g, int sampler_id);
int64_t pg_graph_sampler_note_on(pg_graph* g, int sampler_id, uint8_t note, float volume, float panning, uint64_t sample_time);
int pg_graph_sampler_note_off(pg_graph* g, int sampler_id, int64_t note_id, uint64_t sample_time);
int pg_graph_sampler_all_notes_off(pg_graph* g, int sampler_id, uint64_t sample_time);
int pg_graph_sampler_set_note_speed(pg_graph* g, int sampler_id, int64_t note_id, double speed, float glide_semitones_per_second, uint64_t sample_time);
int pg_graph_sampler_set_note_volume(pg_graph* g, int sampler_id, int64_t note_id, float volume, uint64_t sample_time);
int pg_graph_sampler_set_note_panning(pg_graph* g, int sampler_id, int64_t note_id, float panning, uint64_t sample_time);
int pg_graph_sampler_set_parameter(pg_graph* g, int sampler_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time);
int pg_graph_sampler_stop(pg_graph* g, int sampler_id, uint64_t sample_time);
int pg_graph_sampler_state(pg_graph* g, int sampler_id, pg_sampler_state* out);

/* Granular-mode samplers: Sampler::with_granular_playback (src/generator/sampler.rs:598-637) — a pool of up to 64 granular voices (GrainPool<100>
 * each, with or without a modulation matrix) that notes start, steal and release. The note layer runs on the device in a kernel of its own
 * (pg_gsampler_kernel; DESIGN.md "Granular samplers"), between the grain launches of consecutive Sampler::write spans: a granular slot becomes free
 * at the END of the Sampler::write in which its pool ran dry or its envelope went Idle (voice.rs:488-502), and the ends of those writes are the
 * cuts of the owning mixer chain (its own events and its ancestors', mixed.rs:679-712) — until then the slot's scheduler, and its generator, run on.
 * pg_graph_add_granular_sampler(g, mixer, buffer, opt, gopt): `opt` as for pg_graph_add_sampler (voice count 1..=64, envelope, transient, start
 * time; null: the defaults). has_loop_range + loop_start / loop_end there are Sampler::set_loop_range before playback (voice.rs:329-338): source
 * frames over the file's frame count, as f32; without it gopt->params' own normalised range applies, and without that the buffer's embedded loop
 * (enable_granular_playback, voice.rs:353-360). `gopt` (not null):
 *   params       the GranularParameters (checked by pg_granular_params_check); params.rng_state is the pools' base state (below);
 *   modulation   null: no slot has a matrix (every `*_mod` input is 0.0: what a sampler without routings feeds, at a lower cost); else every slot
 *                gets a matrix made as pg_graph_set_voice_modulation_matrix makes one — Lfo::new's three draws, then the rates, waveforms and
 *                routes — but WITHOUT a note: velocity 0, keytracking 60 / 127 until the slot's first note_on; `velocity` and `note` of the
 *                struct are not used, a note brings its own;
 *   rng_states   null, or voice_count x 3 x 4 words: the Xoshiro256++ state of slot k's pool, LFO 1 and LFO 2 at rng_states[(3 k + j) * 4 ..]
 *                (an all-zero state: SplitMix64(0x5EED0000) x 4, as everywhere). Without the table, slot k's generator j (0 pool, 1 LFO 1,
 *                2 LFO 2) gets pg_granular_sampler_rng_state(given, k, j): `given` = params.rng_state for j = 0, modulation->lfo[j - 1].rng_state
 *                else, all-zero replaced as above; z = (given[0] ^ rotl(given[1], 16) ^ rotl(given[2], 32) ^ rotl(given[3], 48)) +
 *                (3 k + j + 1) * 0xD1B54A32D192ED03; the state is four SplitMix64 outputs from z, the low byte of the last word replaced by
 *                3 k + j — so no two generators of a sampler share a state. The reference seeds from the OS: this rule is this implementation's.
 * The mono buffer the pools read is the buffer's granular buffer (pg_graph_prepare_granular_buffer), shared by all slots. Refusals as for
 * pg_graph_add_sampler (the main mixer included), plus what pg_granular_params_check / pg_modulation_params_check refuse and a null `gopt`.
 * Every pg_graph_sampler_* call above works on such a sampler, with the same sample_time and start-time rules. What a message does:
 *   note_on      next_free_voice_index as above (releasing = an envelope in Release); SamplerVoice::start (voice.rs:122-193): the pool is reset if
 *                the slot was active (granular.rs:495-502: every grain deactivated, the primary cleared — the generator carries on), then
 *                GrainPool::start (:474-489): trigger_phase 1, playhead = the position parameter, speed / volume / panning set DIRECTLY (a pool
 *                has no smoothers: no ramps, no glide); AhdsrEnvelope::note_on(params, 1.0); ModulationMatrix::note_on (matrix.rs:394-408): both
 *                LFOs reset, velocity = the note's volume, keytracking = note / 127;
 *   note_off     with an envelope its note_off alone — the pool goes on triggering until Idle; without one GrainPool::stop: no new grains, the slot
 *                is free with the write in which the last grain ends (the file source behind the voice is never written in this mode);
 *   setters      the per-note ones and STRN / SFTN / SVOL / SPAN go to the pool as voice.rs:239-310 sends them, from that frame on.
 * pg_graph_sampler_set_granular_parameter: Sampler::set_granular_parameter (sampler.rs:299-360) at exactly `sample_time`, resolved as
 * pg_graph_set_voice_granular_parameter resolves it; it reaches every slot, playing or free; grains keep the window and loop range they were born
 * with, the pool follows a new overlap mode. Dropped while the sampler stops, like every trigger. PG_ERR_STATE on a file sampler.
 * Read-backs (debug; they wait for the graph's work): after a write each shows the state as of the end of that write, the last span closed.
 * pg_graph_sampler_voice_grain_state / _voice_modulation_state: slot `slot`'s pool and matrix (PG_ERR_STATE: a file sampler, no matrix;
 * PG_ERR_PARAMETER: no such slot); pg_graph_sampler_granular_params: the sampler's parameters and loop range.
 * Exact / not exact: DESIGN.md. The sub-mixer that holds such a sampler counts it as a source that delivered a full block for as long as it lives.
 * Messages that change what EVERY voice of the pool does while notes sound (Sampler::process_playback_messages, sampler.rs:656-731). Any thread,
 * through the control ring, with the sample_time, start-time and same-frame ordering rules of the other sampler messages (a message stamped before
 * the start time acts at the start time); dropped while the sampler stops (:663-664); PG_ERR_NOT_FOUND for an unknown or removed id; argument
 * checks first, a null handle last.
 *   pg_graph_sampler_set_envelope_parameter   SetParameter(AMP_*) -> set_envelope_parameter (:184-217, :1122-1131) on a file sampler AND a granular
 *       one: AATK Attack, AHLD Hold, ADCY Decay, AREL Release (0..=10 s, Exponential(2.0), defaults 0.001 / 0.75 / 0.5 / 1.0) and ASTN Sustain
 *       (0..=1, linear, 0.75) of the pool's ONE AhdsrParameters. Raw values are clamped, normalized ones clamped to 0..=1 and denormalized
 *       (:862-883). PG_ERR_PARAMETER: an unknown FourCC, a NaN, a sampler without an envelope (the reference's "Invalid or unknown sampler
 *       parameter", :1128-1131, :1189). The setters are not independent (ahdsr.rs:143-249): set_sustain_level leaves decay_rate as it is,
 *       set_decay_time divides (1 - sustain) as it holds THEN, a zero time is a rate of f32::MAX, a Hold in progress keeps its remaining samples.
 *       Messages may be sent out of time order, so the host resolves each one where its event leaves the mixer's sorted list: an ADCY sent first
 *       but due behind an ASTN sees the new sustain. A time goes through Duration::from_secs_f32(s.max(0.0)).as_secs_f32() (:191-208):
 *       nanoseconds rounded to nearest (ties to even), then `secs as f32 + nanos as f32 / 1e9f32` — 4e-10 s is a zero Duration and a rate of
 *       f32::MAX, 0.6e-9 s is 1 ns. That rounding rule is the standard library documentation's; it is UNVERIFIED against the library's source,
 *       which this project does not hold. pg_graph_sampler_set_parameter does NOT take these ids: the two calls have disjoint tables.
 *   pg_sampler_envelope_param_count / pg_sampler_envelope_param   the five descriptors in Sampler::envelope_parameters() order (:173-181).
 *   pg_graph_sampler_set_modulation / _clear_modulation / _set_lfo_rate / _set_lfo_waveform   SetModulation / ClearModulation and
 *       SetParameter(ML1R | ML2R | ML1W | ML2W) (:704-720, :1148-1186, :1210-1244) for the matrix of every slot, playing or free; sources, targets,
 *       LFO indices, waveforms, the amount range, the 0.001 threshold and the rate clamp are pg_graph_set_voice_modulation's / _lfo_rate's /
 *       _lfo_waveform's. A rate or waveform changes nothing else of the LFO (no draw, no phase change); a later note_on resets both LFOs and keeps
 *       the rate, waveform and routes a message gave them. PG_ERR_STATE: a file sampler ("only available when granular playback is enabled"),
 *       a granular sampler created with modulation == NULL (it has no matrix to route in: that mode is this implementation's).
 *   pg_graph_sampler_set_loop_range   SamplerMessage::SetLoopRange (:1246-1271, voice.rs:312-339) on a granular sampler: source frames of the
 *       sampler's buffer, normalised as at creation (`start as f32 / frame_count as f32`); has_loop_range == 0 is SetLoopRange(None): NO loop,
 *       not the buffer's embedded one. Every slot's pool takes it; playing_loop_range, the playhead and living grains keep what they have
 *       (granular.rs:516-518). PG_ERR_PARAMETER: start >= end, start >= frame_count, end > frame_count. PG_ERR_STATE: a file sampler.
 *   pg_graph_sampler_envelope_params   debug read-back (waits for the graph's work): the AhdsrParameters as the device holds them — for a file
 *       sampler slot `slot`'s own copy, for a granular one the sampler's one set (`slot` must still name a slot: PG_ERR_PARAMETER).
 *       PG_ERR_STATE: a sampler without an envelope. zero_times: bit 0 hold, bit 1 decay, bit 2 release time is zero.
 * OUT OF SCOPE: the main mixer through pg_graph_add_sampler / pg_graph_add_granular_sampler, which still refuse it (its entry points are
 * pg_graph_add_sampler_to_main / pg_graph_add_granular_sampler_to_main, below); the sharded handle; modulation messages to a sampler created
 * WITHOUT a matrix (with one: pg_graph_sampler_set_modulation and the LFO calls above); set_loop_range while playing on FILE samplers (it would
 * move where a playing PreloadedFileSource wraps; granular ones: pg_graph_sampler_set_loop_range); the AMP_* ids through
 * pg_graph_sampler_set_parameter (their call is pg_graph_sampler_set_envelope_parameter); playback status events of sampler voices and the
 * sampler's own Stopped event; GeneratorPlaybackOptions::volume and ::panning for samplers in a SUB-mixer (there the pool is summed source by
 * source and no sum of the sampler exists to scale: see pg_graph_add_sampler_to_main); the reference's 54-entry message queue (the control ring
 * and PG_ERR_QUEUE_FULL stand in for it). */
typedef struct pg_granular_sampler_options {
  pg_granular_params params;
  const pg_modulation_params* modulation;   /* NULL: no matrix */
  const uint64_t* rng_states;               /* NULL, or voice_count * 3 * 4 words */
} pg_granular_sampler_options;
void pg_granular_sampler_options_default(pg_granular_sampler_options* opt);
int pg_granular_sampler_options_check(const pg_granular_sampler_options* opt);
void pg_granular_sampler_rng_state(const uint64_t given[4], uint32_t slot, uint32_t generator, uint64_t out[4]);
int pg_graph_add_granular_sampler(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt, const pg_granular_sampler_options* gopt);
int pg_graph_sampler_set_granular_parameter(pg_graph* g, int sampler_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time);
int pg_graph_sampler_voice_grain_state(pg_graph* g, int sampler_id, int slot, pg_grain_state* out);
int pg_graph_sampler_voice_modulation_state(pg_graph* g, int sampler_id, int slot, pg_modulation_state* out);
int pg_graph_sampler_granular_params(pg_graph* g, int sampler_id, pg_granular_params* out);
typedef struct pg_sampler_envelope_state {   /* AhdsrParameters after set_sample_rate(graph rate), as the device holds them */
  float attack_rate, decay_rate, release_rate;   /* per frame; a zero time: FLT_MAX */
  float sustain_level;
  float hold_samples;                            /* hold_time.as_secs_f32() * sample_rate as f32 */
  float attack_scaling, decay_scaling, release_scaling;
  int32_t zero_times;                            /* bit 0: hold_time, bit 1: decay_time, bit 2: release_time is zero */
} pg_sampler_envelope_state;
int pg_sampler_envelope_param_count(void);
int pg_sampler_envelope_param(int index, pg_param_desc* out);
int pg_graph_sampler_set_envelope_parameter(pg_graph* g, int sampler_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time);
int pg_graph_sampler_envelope_params(pg_graph* g, int sampler_id, int slot, pg_sampler_envelope_state* out);
int pg_graph_sampler_set_modulation(pg_graph* g, int sampler_id, int source, int target, float amount, int bipolar, uint64_t sample_time);
int pg_graph_sampler_clear_modulation(pg_graph* g, int sampler_id, int source, int target, uint64_t sample_time);
int pg_graph_sampler_set_lfo_rate(pg_graph* g, int sampler_id, int lfo, float rate_hz, uint64_t sample_time);
int pg_graph_sampler_set_lfo_waveform(pg_graph* g, int sampler_id, int lfo, int waveform, uint64_t sample_time);
int pg_graph_sampler_set_loop_range(pg_graph* g, int sampler_id, int has_loop_range, uint64_t loop_start, uint64_t loop_end, uint64_t sample_time);

/* Samplers on the MAIN mixer, with the generator's volume and panning: what Player::play_generator / add_generator do by default
 * (GeneratorPlaybackOptions::target_mixer = None, src/generator.rs:41-78; add_or_play_generator, src/player.rs:1048-1133): the Sampler goes to the
 * main mixer as ONE source behind AmplifiedSource(options.volume) -> PannedSource(options.panning), and GeneratorPlaybackHandle::set_volume /
 * set_panning drive those two at a sample time (src/player/handles/generator.rs:119-196). DESIGN.md, "Samplers on the main mixer".
 * pg_generator_options: volume (default 1.0) and panning (default 0.0). _default / _check touch no graph and no device; _check: PG_OK or
 * PG_ERR_PARAMETER with GeneratorPlaybackOptions::validate's text (generator.rs:120-140) for a negative or NaN volume ("playback options 'volume'
 * value is '..'") and a panning outside [-1, 1] or NaN ("playback options 'panning' value is '..'"); null options are refused.
 * pg_graph_add_sampler_to_main(g, buffer, opt, gen) / pg_graph_add_granular_sampler_to_main(g, buffer, opt, gopt, gen): `opt` / `gopt` as for
 * pg_graph_add_sampler / pg_graph_add_granular_sampler (transient 1 = play_generator, 0 = add_generator; start_time as there); gen == NULL: the
 * defaults. Checks in this order, the first three before the handle is looked at or a device touched: sampler options, granular options,
 * generator options, handle, buffer, loop range. Returns a sampler id of the same id space: EVERY pg_graph_sampler_* call above takes it with
 * unchanged rules (pg_graph_remove_sampler, the read-backs, the envelope, matrix, LFO, loop-range and granular-parameter messages included).
 *   the unit    the whole pool is one source unit of the main mixer, one workgroup of the exact kernel, for as long as the sampler lives; a source
 *               added later with the same start time stands in front of it in the mixer's sum (mixed.rs:324-329).
 *   the grid    a message to such a sampler is an event of the MAIN mixer: it ends the main mixer's chunk at its frame and the next chunk begins
 *               there, min(remaining, 4096) frames long (mixed.rs:659-719). Under a sub-mixer the parent's chunk simply goes on. So the ends of
 *               Sampler::write — where a slot becomes free, what a later note of that slot finds — differ between the two placements.
 *   the result  `produced_output` of the mixer is what Sampler::write returns: 0 when stopped, or when no voice is active and it is not stopping,
 *               evaluated behind the messages of that write (sampler.rs:974-981); else the whole buffer, zeros included. A granular pool counts
 *               as having delivered for as long as it lives (the deviation pg_graph_add_granular_sampler documents).
 *   the stage   apply_smoothed_gain, then apply_smoothed_panning (smoothing.rs:59-125) over the samples written: while the volume ramps one
 *               next() per interleaved SAMPLE, at rest a scale iff |1 - gain| > 1e-6; while the panning ramps one next() per FRAME, at rest the pan
 *               law iff |pan| > 1e-6. Whether a smoother ramps is asked once per write. Both stand still over a write that returned 0.
 *   end of life a transient sampler that has stopped leaves the mixer after the write in which it stopped (mixed.rs:612-615); its read-backs stay.
 * pg_graph_sampler_set_volume / _set_panning: MixerMessage::SetSourceVolume / SetSourcePanning. Any thread, through the control ring
 * (PG_ERR_QUEUE_FULL); sample_time 0 = the next write's first frame; a time before the start time acts at the start time. The target is set in
 * front of the message's frame, which begins a chunk. Of several messages of one kind due on one frame the LAST one sent counts (the wrapper's
 * one-slot queue, amplified.rs:33-35). PG_ERR_PARAMETER: a negative or non-finite volume, a non-finite panning (the bounds
 * pg_graph_sampler_set_note_volume / _set_note_panning state); PG_ERR_NOT_FOUND: an unknown or removed id; PG_ERR_STATE: a sampler that lives in
 * a sub-mixer — there the pool is summed source by source and no sum of the sampler exists to scale (OUT OF SCOPE, above).
 * pg_graph_sampler_output_state: debug read-back of the two smoothers (waits for the graph's work): current, target, and whether need_ramp()
 * holds. PG_ERR_STATE for a sampler in a sub-mixer.
 * OUT OF SCOPE: the sharded handle; generator volume and panning for samplers in a sub-mixer; GeneratorPlaybackOptions::measure_cpu_load; playback
 * status events of sampler voices and the sampler's Stopped; the FunDSP generator. */
typedef struct pg_generator_options { float volume; float panning; } pg_generator_options;   /* GeneratorPlaybackOptions::volume / ::panning */
typedef struct pg_sampler_output_state {
  float volume_current, volume_target, panning_current, panning_target;
  int32_t volume_ramping, panning_ramping;
} pg_sampler_output_state;
void pg_generator_options_default(pg_generator_options* opt);   /* 1.0, 0.0 */
int pg_generator_options_check(const pg_generator_options* opt);
int pg_graph_add_sampler_to_main(pg_graph* g, int buffer_id, const pg_sampler_options* opt, const pg_generator_options* gen);
int pg_graph_add_granular_sampler_to_main(pg_graph* g, int buffer_id, const pg_sampler_options* opt, const pg_granular_sampler_options* gopt, const pg_generator_options* gen);
int pg_graph_sampler_set_volume(pg_graph* g, int sampler_id, float volume, uint64_t sample_time);
int pg_graph_sampler_set_panning(pg_graph* g, int sampler_id, float panning, uint64_t sample_time);
int pg_graph_sampler_output_state(pg_graph* g, int sampler_id, pg_sampler_output_state* out);

/* Per-mixer level metering: PlayerConfig::metering_interval (src/player.rs:162-217) wraps the main mixer and every sub-mixer in a MeteredSource
 * (src/player.rs:346-348, :784-786; src/source/mixed/submixer.rs:24); Player::audio_level / MixerHandle::audio_level return per-channel peak and
 * RMS (AudioLevel, src/source/metered.rs), linear. The meter runs on the device (pg_meter_kernel: the sub-mixers' samples never leave it).
 * AudioLevelState (metered.rs:75-143) per mixer: peak_hold (f32) and sum_square (f64) per channel, collected_frames, a clock with start_time 0,
 * update_interval = (interval.as_secs_f64() * sample_rate as f64) as u64 frames, truncated (src/utils/time.rs:28-35). One RECORD is one write call
 * of the wrapped mixer that returned samples: every sample enters peak_hold by a compare (a NaN never does) and sum_square as an f64 square; the
 * frames are counted; then, with `time` the START of that call, `time.saturating_sub(start_time) >= update_interval` publishes peak = peak_hold,
 * rms = sqrt(sum_square / collected_frames) as f32, sets start_time = time and zeroes the accumulators.
 *   main mixer: one record per pg_graph_write* call whatever its length or the chunks and pieces it is rendered in, over the samples the call
 *     delivers (behind the bus effects), time = the call's pos_in_frames; a call that returns 0 (mixed.rs:664-670) records nothing.
 *   sub-mixer (nested ones too): one record per chunk of its parent — the call of SubMixerProcessor::process (submixer.rs:47-77) in which its
 *     silence gate is decided, over the same buffer — time = the chunk's start (chunks: min(remaining, 4096) frames, cut at the parent's events,
 *     mixed.rs:679-712). A sub-mixer with no source in its list, no effect, no sub-mixer and no pending event as the chunk begins returns 0 and
 *     records nothing: its level stays FROZEN at what it last published (decided on the device, where the drop of an exhausted transient source
 *     is known at the reference's time). A call the silence gate has closed (2 s below -60 dB) reads as zeros.
 * The reference skips a record when its try_lock fails (metered.rs:196-204); nothing contends here, so no record is ever skipped.
 * The published RMS is within one f32 rounding of the reference's sequential f64 sum (the kernel sums in a fixed parallel order), the peak equal. */
typedef struct pg_audio_level { float peak[2]; float rms[2]; } pg_audio_level;   /* AudioLevel, linear; 16 bytes */
/* PlayerConfig::metering_interval for all mixers of the graph, also those added later: interval_seconds >= 0 (the value Duration::as_secs_f64()
 * returns) enables metering and resets every mixer to AudioLevelState::new (levels 0); < 0 is None: metering off, nothing is launched and a write
 * is exactly what it is without this call. NaN / +inf: PG_ERR_PARAMETER (checked before the handle), a null handle too. Owner thread; waits for
 * earlier writes like every graph-changing call. All memory (state, published levels, span tables) is reserved here and in the add_* calls:
 * writes allocate nothing. */
int pg_graph_set_metering(pg_graph* g, double interval_seconds);
/* Player::audio_level (mixer 0) / MixerHandle::audio_level: the level the mixer last published. Any thread, any time: reads pinned host memory
 * the kernel writes (guarded by a sequence word; the reader retries), never waits for the device, makes no HIP call. After pg_graph_synchronize
 * (or a host-buffer pg_graph_write) it reflects every record of the writes issued so far. PG_ERR_STATE: metering is off; PG_ERR_NOT_FOUND: unknown
 * or removed mixer; PG_ERR_PARAMETER: null handle or null `out`. With pg_graph_set_defer_bus the main mixer's record is taken at the end of
 * pg_graph_process_bus_device*, with that call's pos_in_frames and samples, not in the write. */
int pg_graph_mixer_audio_level(pg_graph* g, int mixer_id, pg_audio_level* out);

/* Playback status events: PlaybackStatusEvent::Position / ::Stopped { exhausted } (src/source/status.rs) as every file source and every sampler
 * voice of the reference sends them — FileSourceImpl::send_playback_position_status / send_playback_stopped_status (src/source/file/common.rs:171-221)
 * from PreloadedFileSource::write / stop / kill (src/source/file/preloaded.rs:196-239, :396-475) and SamplerVoice::process
 * (src/generator/sampler/voice.rs:434-467, :488-502). The reference decides them once per Source::write call of the voice — once per chunk of the
 * voice's mixer, once per segment where the mixer's events (or an ancestor's) cut the chunk, and where the voice's stop time cuts the call
 * (src/source/mixed.rs:558-624, :679-712) — and so does the device (pg_playback_status_kernel, DESIGN.md "Playback status"): every record equals the
 * reference's, field by field; the host derives no position.
 *   sample_time       SourceTime::pos_in_frames of the source write that sent the record (for a stop without a fade-out: the stop's time)
 *   Position          after every source write that was not skipped as finished, if `elapsed(time.pos_in_frames) >= emit_rate` — elapsed: a saturating
 *                     subtraction from the clock's start_time, 0 at first (src/utils/time.rs:19-55) — with playback_pos as it stands BEHIND that write,
 *                     and the clock restarts at time.pos_in_frames (common.rs:171-208). frame_pos = sample_pos / channel_count, position_seconds =
 *                     frame_pos as f64 / sample_rate as f64 (:195-196), both of the FILE buffer. A file voice sends no start event: `playback_started`
 *                     is never set to true anywhere in the reference (docs/parity_findings.md).
 *   Stopped           { exhausted: playback_pos_eof } with the write in which the end of the file was reached or the fade-out completed (preloaded.rs:464-472);
 *                     at the stop's time when the voice stops without a fade-out (:196-208); for an enveloped voice with the write in which the envelope
 *                     reached Idle — SamplerVoice::reset -> PreloadedFileSource::reset -> kill, if the source had not finished already (voice.rs:488-495,
 *                     preloaded.rs:212-239). Position stands before Stopped.
 *   granular voices   every process call sends Position (under the emit test), the first one as a start event: unconditionally (grain_pool_started,
 *                     voice.rs:449-467); sample_pos = (GrainPool::playback_position(parameters, pos_mod) * buffer_len as f32) as u64 (granular.rs:446-472),
 *                     pos_mod = the last frame's GRAIN_POSITION sum (0.0 without a matrix). buffer_len, channel_count and sample_rate are the FILE
 *                     buffer's for a voice made from a sample buffer; n_frames, 1 and the graph's rate for pg_graph_add_granular_voice. When the voice
 *                     ends, two Stopped records (voice.rs:488-502): reset()'s kill with exhausted 0 (the file source never played), then
 *                     { exhausted: pool.is_exhausted() } evaluated behind GrainPool::reset, which re-arms the trigger (granular.rs:442-444, :495-502): 0.
 *   nothing           from pg_graph_remove_voice, and from a voice pg_graph_stop_all_voices took before it had started.
 * pg_graph_enable_status: once, before the first write (PG_ERR_STATE otherwise); reserves the ring of `capacity_events` records (>= 1, else
 *   PG_ERR_PARAMETER) and the tables the kernel works from — writes and polls allocate nothing. The reference sends with try_send on a bounded
 *   channel and drops what finds it full: a record that finds capacity_events unpolled ones is dropped — the newest goes — and counted
 *   (pg_graph_status_dropped). The count also holds what the device could not keep, which takes a chunk that a mixer's events cut very often: the
 *   exact kernel logs 32 source writes of a voice per launch, and a job of the status kernel has three record slots per source write it can see.
 * pg_graph_set_voice_status: position_emit_seconds = FilePlaybackOptions::playback_pos_emit_rate (<= 0: None, no Position records; > 0: converted as
 *   SampleTimeClock::duration_to_sample_time does, (secs * rate as f64) as u64, time.rs:28-35); report_stopped != 0: Stopped records. Every voice starts
 *   with both off, and a graph that never calls this is what it was without it. Only before the voice has rendered a frame (PG_ERR_STATE afterwards;
 *   PG_ERR_STATE also when status is not enabled on the graph); PG_ERR_NOT_FOUND for an unknown voice; PG_ERR_PARAMETER for a NaN, a null handle, a
 *   host-fed voice and a voice whose source_rate is not the graph's. Owner thread; waits for earlier writes like every graph-changing call.
 * pg_graph_poll_status: copies out up to max_events records, oldest first, and returns how many. They cover every write that has returned (on a
 *   caller's stream, and for pg_graph_set_defer_bus graphs: every write up to the last pg_graph_synchronize / wait for that stream). Order: by
 *   sample_time; then as the reference's write reaches the voices — a mixer's sub-mixers first, in the order they were added, then its sources in its
 *   list's order (sorted by start time, a new source in front of those that start at the same time: mixed.rs:324-329, :505-620); then as one source
 *   write sent them. Owner thread.
 * While a voice that reports is in the graph, writes are rendered chunk by chunk, piece by piece (no launch of several blocks,
 * pg_graph_set_max_blocks_per_launch: the result of those is bit-identical to single launches anyway), pg_playback_status_kernel behind every piece.
 * The audio does not depend on who reports: the same kernels render the same pieces, bit for bit ("Playback status").
 * OUT OF SCOPE: host-fed and rate-converted voices; PlaybackStatusContext payloads (a binding keeps a map from voice id to context); CPU-load
 * measurement; the voices of a sampler (pg_graph_add_sampler: its note layer would forward their events). */
#define PG_STATUS_POSITION 0
#define PG_STATUS_STOPPED  1
typedef struct pg_status_event {
  int32_t  kind;              /* PG_STATUS_* */
  int32_t  voice_id;
  uint64_t sample_time;       /* SourceTime::pos_in_frames of the source write that emitted it */
  uint64_t frame_pos;         /* Position: sample_pos / channel_count (common.rs:195); Stopped: 0 */
  double   position_seconds;  /* frame_pos as f64 / sample_rate as f64 (common.rs:196); Stopped: 0 */
  int32_t  exhausted;         /* Stopped only */
  int32_t  reserved;
} pg_status_event;
int pg_graph_enable_status(pg_graph* g, size_t capacity_events);
int pg_graph_set_voice_status(pg_graph* g, int voice_id, double position_emit_seconds, int report_stopped);
int pg_graph_poll_status(pg_graph* g, pg_status_event* out, size_t max_events);
uint64_t pg_graph_status_dropped(pg_graph* g);

/* Source::write(&mut output, &SourceTime{pos_in_frames}) of the main MixedSource
 * (src/source/mixed.rs:659-719): returns the samples written == n_samples, or 0 when the
 * graph is empty (or after a device failure: GuardedSource, src/source/guarded.rs:87-107).
 * `out` is a host buffer. */
size_t pg_graph_write(pg_graph* g, float* out, size_t n_samples, uint64_t pos_in_frames);
/* Same, output left in device memory (`d_out` = device pointer, >= n_samples floats), enqueued
 * on `hip_stream` (a hipStream_t, NULL = the graph's own stream); asynchronous when a stream is
 * given. Used for the multi-GPU master-bus reduce and by bench.py. */
size_t pg_graph_write_device(pg_graph* g, float* d_out, size_t n_samples, uint64_t pos_in_frames, void* hip_stream);
/* Offline rendering (the reference's WavOutput pull loop, src/output/wav.rs:210-250, has no deadline per block): a write*() call that
 * spans several blocks of max_frames may render up to `n_blocks` of them in ONE launch sequence when nothing is scheduled inside them and
 * every unit is in steady state (MixedSource::write walks its chunks inside one call the same way, src/source/mixed.rs:679-712). All
 * per-chunk semantics (bypass counters, tails, silence gates) stay per chunk of the reference's grid (see pg_graph_create): a launch sequence
 * covers whole chunks, its blocks are their pieces. Default 1; sizes the per-unit output table (max(n_blocks, 4096 / max_frames) x units x
 * max_frames x 8 bytes), allocated at the next graph mutation / first write — call it while building the graph. The result is bit-identical
 * to the same calls without super-block launches.
 * (pg_graph_write with a host buffer renders ONE write call whatever its length: its staging holds whole chunks — at least 4096 frames —
 * and the call is copied out span by span.) */
/* A unit that leaves the steady state while a super-block launch is in flight (the host only launches them for graphs it knows to be
 * steady: this is a consistency violation, PG_DEVERR_SUPER_DEFERRED) would miss its later blocks: the kernels mirror that flag to the host
 * and the NEXT write*() call disables the graph (returns 0 from then on, pg_last_error_message names the flag) — wrong audio is never
 * handed out twice; pg_graph_device_errors reports the flag at any time. */
int pg_graph_set_max_blocks_per_launch(pg_graph* g, int n_blocks);
/* Process-wide counters of the library's own HIP calls: out[0] = allocations (hipMalloc / hipHostMalloc), out[1] = releases, out[2] = host
 * waits for a stream (hipStreamSynchronize), out[3] = blocking copies / fills. The reference runs its audio callback under
 * assert_no_alloc (src/output/cpal.rs:712-715); with these counters a test asserts the same of pg_graph_write*: on a built graph it
 * allocates nothing and frees nothing, and on a caller's stream it never blocks the host. */
void pg_debug_hip_calls(uint64_t out[4]);
/* Measurement hook (tools/sample_buffer_cost.py): hipEvent times in ms of a sample buffer's upload, of pass A (the schedule) and of pass B
 * (interpolation and down-mix) of its conversion; 0 where none ran. The events exist only in a process with PHONIC_DEBUG_HOOKS=1 in its
 * environment: without it pg_graph_add_sample_buffer and the conversion create and record none, and this reads zeros. */
int pg_debug_sample_buffer_times(pg_graph* g, int buffer_id, float out_ms[3]);
/* Measurement hook (tools/waveform_cost.py): hipEvent time in ms of the kernels of the buffer's last pg_graph_sample_buffer_waveform call (without
 * the waits, the allocation and the copy to the host); 0 if none ran. Like the hook above it exists only with PHONIC_DEBUG_HOOKS=1. */
int pg_debug_sample_buffer_waveform_time(pg_graph* g, int buffer_id, float* out_ms);
/* Test hook: the nth launch round from now (process-wide, any graph) fails the way a HIP launch failure does — the graph it hits becomes
 * silent for good: write returns 0, like the reference's GuardedSource after a panic (src/source/guarded.rs:87-107). 0 disarms. Armed only in
 * a process with PHONIC_DEBUG_HOOKS=1 in its environment; a no-op otherwise. */
void pg_debug_fail_launch_round(int nth);
/* Build check hook (tools/check_kernel_resources.py): dynamic LDS bytes of the staged single launch (which 0) / of a fast unit kernel for the
 * effect kinds of kind_mask (which 1) at n_frames frames per block. */
size_t pg_debug_lds_bytes(int which, uint32_t n_frames, uint32_t kind_mask);
/* Sticky consistency flags raised by the kernels (0 = none; see PG_DEVERR_* in phonic_amd/csrc/pg_dev.h): conditions the host-side
 * routing of units to kernel variants must make impossible. Synchronises the graph's own stream. Negative pg_status on failure. */
int pg_graph_device_errors(pg_graph* g);
/* Multi-GPU: when set, bus effects are skipped in write*(): the caller reduces the partial bus of
 * all ranks (RCCL) and then runs them once on the root with pg_graph_process_bus_device(). */
int pg_graph_set_defer_bus(pg_graph* g, int defer);
int pg_graph_process_bus_device(pg_graph* g, float* d_bus, size_t n_samples, uint64_t pos_in_frames, void* hip_stream);
/* One process per GPU: the ranks' `audible` words ride with their partial buses. pg_graph_export_audible writes the words of the LAST
 * pg_graph_write_device call of a deferred-bus graph — ONE PER PIECE the call was rendered in, in order: a chunk of the reference's grid
 * (min(remaining, 4096) frames from the call's start and from every main-mixer event, src/source/mixed.rs:216,679-712) is ceil(chunk / max_frames)
 * pieces, a chunk's flag sits in the word of its last piece; all 0 when that call had nothing to render — as floats (0 / 1) to d_dst, e.g. right
 * behind the call's samples: ONE sum-reduce then carries samples and words (OR = sum > 0). pg_graph_audible_words = how many words the last
 * call left (an event-free call of n frames: one per block of max_frames when max_frames divides 4096); a deferred-bus call leaves at most
 * max(64, 4096 / max_frames) words — a call that would need more is rendered up to there and returns the samples it rendered (the caller goes on
 * with another call). pg_graph_process_bus_device_flags is pg_graph_process_bus_device with those summed words, consumed in the same order: the
 * root's bus chain takes EffectProcessor's decisions (bypass, tails; src/source/mixed/effect.rs:56-145) per chunk as the one main mixer would.
 * The chain walks the SAME chunk grid as the write: it restarts at the main mixer's effect events (queued by the write) and at the offsets where
 * any other main-mixer event cut this graph's own deferred write of the same position. Ranks whose main-mixer SOURCES take events the root's
 * graph does not hold must end their calls there on every rank: pg_graph_next_main_event (drains the control ring — writing thread only —
 * and returns the sample time of the first main-mixer event behind pos_in_frames, UINT64_MAX when there is none) is what a caller min-reduces
 * over the ranks to size the next call (phonic_amd/parallel.py: next_call_frames). */
int pg_graph_export_audible(pg_graph* g, float* d_dst, int n_words, void* hip_stream);
int pg_graph_audible_words(pg_graph* g);
uint64_t pg_graph_next_main_event(pg_graph* g, uint64_t pos_in_frames);
int pg_graph_process_bus_device_flags(pg_graph* g, float* d_bus, size_t n_samples, uint64_t pos_in_frames, void* hip_stream, const float* d_flags, int n_words);
/* Block until all work of the graph's stream has finished. */
int pg_graph_synchronize(pg_graph* g);

/* ---- voice-sharded graph: the same main MixedSource spread over several GPUs of one node (SURVEY.md §8b `n_gpus`, §8e) ----------
 *
 * The reference's parallel axis is independent sub-mixers rendered by worker threads into private buffers which the caller sums
 * (SubMixerThreadPool, src/source/mixed/submixer/thread_pool.rs:92-121,350-412; src/source/mixed.rs:522-536). Here the workers are
 * devices: one handle owns one pg_graph per entry of `devices` (the first is the root). Every sub-mixer of the main mixer — with its
 * effects, sources and nested sub-mixers — and every main-mixer source is placed on the least loaded shard when it is added (the greedy
 * placement of WorkerTaskBatcher) and never moves; effects added to mixer 0 form the bus chain on the root. write = one asynchronous
 * render per shard on its own device and stream, the partial buses summed on the root device, then the bus chain.
 *
 * The handle IS the main MixedSource: it takes every call pg_graph takes (the reference's MixerMessage set, src/source/mixed.rs:124-145,
 * 163-178,422-462) and routes it to the shard that owns the target; ids returned here are global (valid for the pg_sharded_* calls
 * only) and never reused. A write is cut at the main mixer's event times of ALL shards, so every shard splits its chunks where the one
 * mixer would (mixed.rs:679-712); the bus chain gets one `audible_input` per chunk, OR-ed over the shards (mixed.rs:696-706); write
 * returns 0 exactly when pg_graph_write would (mixed.rs:664-670). Threading as for pg_graph: add_* / remove_* / move_* / write from the
 * owner thread, the control calls (schedule_*, set_voice_*, seek, stop_*) from any thread. A device may be listed more than once
 * (several shards on one GPU: how the single-GPU test-suite exercises this path; not with PG_REDUCE_RCCL). Every call that takes the handle
 * answers a null one with PG_ERR_PARAMETER in its own way of reporting an error ("graph handle is null"; pg_sharded_destroy does nothing),
 * behind the argument checks that need no graph. bench.py's measured multi-GPU
 * path is one process per GPU with an RCCL reduce through torch.distributed (phonic_amd/parallel.py); both sit on the same kernels and
 * per-graph host code. */
typedef struct pg_sharded_graph pg_sharded_graph;
pg_sharded_graph* pg_sharded_create(uint32_t sample_rate, uint32_t channel_count, size_t max_frames, const int* devices, int n_devices);
void pg_sharded_destroy(pg_sharded_graph* s);
int pg_sharded_shard_count(pg_sharded_graph* s);
int pg_sharded_set_max_blocks_per_launch(pg_sharded_graph* s, int n_blocks);   /* a write holds at most n_blocks x max_frames frames */
/* How the shards' partial buses meet on the root device.
 *   PG_REDUCE_PEER_COPY (default): hipMemcpyPeerAsync of every partial to the root + one sum kernel, f32 adds in shard order (deterministic).
 *   PG_REDUCE_RCCL: ncclReduce(sum, float32, root = shard 0) over xGMI on the shards' own streams inside one ncclGroupStart/End, the
 *     `audible` words by ncclReduce(max) in the same group (north_star: "RCCL reduce over xGMI for the master-bus sum"). The sum order
 *     is RCCL's, inside the 1e-5 RMS gate. One communicator per shard from ncclCommInitAll over `devices`, created by this call: every
 *     device may be listed once only; RCCL is looked up at run time (librccl.so.1 — the one already in the process, e.g. PyTorch's, else
 *     ROCm's). On failure the call returns PG_ERR_DEVICE / PG_ERR_PARAMETER with RCCL's error text and the mode stays as it was. */
#define PG_REDUCE_PEER_COPY 0
#define PG_REDUCE_RCCL 1
int pg_sharded_set_reduce(pg_sharded_graph* s, int mode);
int pg_sharded_reduce_mode(pg_sharded_graph* s);
int pg_sharded_add_mixer(pg_sharded_graph* s);                                  /* Player::add_mixer(None) */
int pg_sharded_add_mixer_to(pg_sharded_graph* s, int parent_mixer_id);          /* nested: lives on its parent's shard */
int pg_sharded_add_effect(pg_sharded_graph* s, int mixer_id, int kind, const pg_effect_init* init);
int pg_sharded_add_voice(pg_sharded_graph* s, int mixer_id, const float* pcm, size_t n_frames, uint32_t src_channels, uint32_t src_rate,
                         const pg_voice_options* opt);
/* host-fed sources on the sharded mixer: pg_graph_add_stream_voice / feed_voice / end_stream_voice / stream_voice_consumed on the owning shard */
int pg_sharded_add_stream_voice(pg_sharded_graph* s, int mixer_id, uint32_t channels, uint32_t rate, size_t capacity_frames, const pg_voice_options* opt);
int pg_sharded_feed_voice(pg_sharded_graph* s, int voice_id, const float* frames, size_t n_frames);
int pg_sharded_end_stream_voice(pg_sharded_graph* s, int voice_id);
int64_t pg_sharded_stream_voice_consumed(pg_sharded_graph* s, int voice_id);
int pg_sharded_shard_of_mixer(pg_sharded_graph* s, int mixer_id);
/* Player::remove_mixer / remove_effect / move_effect (src/player.rs:825-867,942-990; MixerMessage::RemoveMixer / RemoveEffect / MoveEffect,
 * src/source/mixed.rs:422-462): semantics and errors of pg_graph_remove_mixer / _remove_effect / _move_effect. */
int pg_sharded_remove_mixer(pg_sharded_graph* s, int mixer_id);
int pg_sharded_remove_effect(pg_sharded_graph* s, int effect_id);
int pg_sharded_move_effect(pg_sharded_graph* s, int effect_id, int mixer_id, int movement, int offset);
int pg_sharded_schedule_param(pg_sharded_graph* s, int effect_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time);
int pg_sharded_schedule_reset(pg_sharded_graph* s, int effect_id, uint64_t sample_time);
int pg_sharded_set_voice_volume(pg_sharded_graph* s, int voice_id, float volume, uint64_t sample_time);
int pg_sharded_set_voice_panning(pg_sharded_graph* s, int voice_id, float panning, uint64_t sample_time);
/* FilePlaybackHandle::set_speed / seek (src/player/handles/file.rs:111,150 -> MixerMessage::SetSourceSpeed / SeekSource, mixed.rs:338-383) */
int pg_sharded_set_voice_speed(pg_sharded_graph* s, int voice_id, double speed, float glide_semitones_per_second, uint64_t sample_time);
int pg_sharded_seek_voice(pg_sharded_graph* s, int voice_id, double position_seconds, uint64_t sample_time);
int pg_sharded_stop_voice(pg_sharded_graph* s, int voice_id, uint64_t sample_time);
int pg_sharded_stop_all_voices(pg_sharded_graph* s);
int pg_sharded_remove_voice(pg_sharded_graph* s, int voice_id);
int pg_sharded_is_voice_playing(pg_sharded_graph* s, int voice_id);
/* pg_graph_set_voice_envelope / _release_voice / _voice_envelope_stage (src/utils/ahdsr.rs, src/generator/sampler/voice.rs:181-212) on the voice's shard */
int pg_sharded_set_voice_envelope(pg_sharded_graph* s, int voice_id, const pg_ahdsr_params* p);
int pg_sharded_release_voice(pg_sharded_graph* s, int voice_id, uint64_t sample_time);
int pg_sharded_voice_envelope_stage(pg_sharded_graph* s, int voice_id);
/* pg_graph_add_granular_voice / _voice_grain_state (src/generator/sampler/granular.rs, src/generator/sampler/voice.rs:406-432) on the voice's shard;
 * volume, panning, speed, stop, release, envelope and seek reach a granular voice through the calls above, as on the plain graph */
int pg_sharded_add_granular_voice(pg_sharded_graph* s, int mixer_id, const float* mono_pcm, size_t n_frames, const pg_granular_params* p, const pg_voice_options* opt);
int pg_sharded_voice_grain_state(pg_sharded_graph* s, int voice_id, pg_grain_state* out);
/* pg_graph_set_voice_granular_parameter / _set_voice_grain_loop_range / _voice_granular_params on the voice's shard */
int pg_sharded_set_voice_granular_parameter(pg_sharded_graph* s, int voice_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time);
int pg_sharded_set_voice_grain_loop_range(pg_sharded_graph* s, int voice_id, int has_loop_range, float loop_start, float loop_end, uint64_t sample_time);
int pg_sharded_voice_granular_params(pg_sharded_graph* s, int voice_id, pg_granular_params* out);
/* pg_graph_add_sample_buffer / _release_sample_buffer / _add_voice_from_buffer / _add_granular_voice_from_buffer / _prepare_granular_buffer /
 * _sample_buffer_info / _read_granular_buffer on the sharded mixer. The handle keeps a host copy of the PCM until release; a buffer reaches a
 * shard (one upload) the first time a voice that uses it is placed there, and each shard makes its own granular buffer — the same one, the
 * conversion is deterministic. prepare converts on the shards the buffer has reached (on the root if it has reached none); info sums use_count
 * over the shards; read_granular_buffer reads from shard `shard` (-1: the first that holds the
 * buffer, the root if none does), uploading and converting there if need be. */
int pg_sharded_add_sample_buffer(pg_sharded_graph* s, const float* pcm, size_t n_frames, const pg_sample_buffer_desc* desc);
int pg_sharded_release_sample_buffer(pg_sharded_graph* s, int buffer_id);
int pg_sharded_add_voice_from_buffer(pg_sharded_graph* s, int mixer_id, int buffer_id, const pg_voice_options* opt);
int pg_sharded_add_granular_voice_from_buffer(pg_sharded_graph* s, int mixer_id, int buffer_id, const pg_granular_params* p, const pg_voice_options* opt);
int pg_sharded_prepare_granular_buffer(pg_sharded_graph* s, int buffer_id);
int pg_sharded_sample_buffer_info(pg_sharded_graph* s, int buffer_id, pg_sample_buffer_info* out);
int64_t pg_sharded_read_granular_buffer(pg_sharded_graph* s, int buffer_id, int shard, float* out, size_t cap_frames);
/* pg_graph_set_voice_modulation_matrix / _set_voice_modulation / _clear_voice_modulation / _set_voice_lfo_rate / _set_voice_lfo_waveform /
 * _voice_modulation_state (src/modulation/matrix.rs, src/generator/sampler/modulation.rs) on the voice's shard */
int pg_sharded_set_voice_modulation_matrix(pg_sharded_graph* s, int voice_id, const pg_modulation_params* p);
int pg_sharded_set_voice_modulation(pg_sharded_graph* s, int voice_id, int source, int target, float amount, int bipolar, uint64_t sample_time);
int pg_sharded_clear_voice_modulation(pg_sharded_graph* s, int voice_id, int source, int target, uint64_t sample_time);
int pg_sharded_set_voice_lfo_rate(pg_sharded_graph* s, int voice_id, int lfo, float rate_hz, uint64_t sample_time);
int pg_sharded_set_voice_lfo_waveform(pg_sharded_graph* s, int voice_id, int lfo, int waveform, uint64_t sample_time);
int pg_sharded_voice_modulation_state(pg_sharded_graph* s, int voice_id, pg_modulation_state* out);
/* pg_graph_set_metering / pg_graph_mixer_audio_level on the one mixer: a sub-mixer's level comes from its shard; mixer 0's is measured on the root
 * behind the bus chain, one record per pg_sharded_write* call (src/source/metered.rs:75-143) */
int pg_sharded_set_metering(pg_sharded_graph* s, double interval_seconds);
int pg_sharded_mixer_audio_level(pg_sharded_graph* s, int mixer_id, pg_audio_level* out);
/* pg_graph_enable_status / _set_voice_status / _poll_status / _status_dropped on the one mixer (src/source/status.rs, src/source/file/common.rs:171-221):
 * the shard that owns a voice decides its records; every shard keeps a ring of capacity_events records of its own. Voice ids are the handle's; a
 * poll merges the shards' records into the order of pg_graph_poll_status — the main mixer's sub-mixers in the order they were added, whatever shard
 * holds them, then its sources in its list's order — and the dropped count is the shards' sum. */
int pg_sharded_enable_status(pg_sharded_graph* s, size_t capacity_events);
int pg_sharded_set_voice_status(pg_sharded_graph* s, int voice_id, double position_emit_seconds, int report_stopped);
int pg_sharded_poll_status(pg_sharded_graph* s, pg_status_event* out, size_t max_events);
uint64_t pg_sharded_status_dropped(pg_sharded_graph* s);
/* Source::write: host buffer (waits for the result) / buffer on the root device (asynchronous on the shards' streams, several calls may be
 * enqueued before pg_sharded_synchronize). A call of ANY length is ONE write of the one main mixer — messages processed once on every shard,
 * one call end — walked on the reference's chunk grid (min(remaining, 4096) frames from the call's start and from every main-mixer event of
 * any shard, src/source/mixed.rs:216,679-712) whatever max_blocks x max_frames is. Both return the samples written, or 0 when
 * the main mixer has nothing to do (mixed.rs:664-670: no playing source, sub-mixer or pending event on any shard and no effect on
 * mixer 0; the host learns that sources have ended from the device after a pg_sharded_write, as pg_graph_write does). */
size_t pg_sharded_write(pg_sharded_graph* s, float* out, size_t n_samples, uint64_t pos_in_frames);
size_t pg_sharded_write_device(pg_sharded_graph* s, float* d_out, size_t n_samples, uint64_t pos_in_frames);
int pg_sharded_synchronize(pg_sharded_graph* s);
int pg_sharded_device_errors(pg_sharded_graph* s);

/* Introspection used by the harness */
int pg_graph_voice_count(pg_graph* g);
int pg_graph_is_voice_playing(pg_graph* g, int voice_id);
/* Number of units (sub-mixers and main-mixer sources) the time-parallel kernels handed to the exact serial kernel in the last launch
 * round that had any to hand over or to check (ramping parameters, a command inside the block, a chain without a time-parallel
 * path); 0 in steady state. Synchronises the graph's own stream: call it after pg_graph_write, or after the caller synchronised the
 * stream given to pg_graph_write_device. */
int pg_graph_deferred_units(pg_graph* g);
/* Average device time (ms) of the dominant kernel launch(es) (see pg_graph_dominant_kernel) over the launches
 * since the last call with reset != 0, measured with hipEvents on the graph's stream; launches = count. */
double pg_graph_kernel_ms(pg_graph* g, int reset, uint64_t* launches);
/* The same measurement as sums: total device time (ms) of the timed launches, their count, and the number of max_frames blocks they
 * rendered (a super-block launch renders several blocks per unit). Waits for the timed launches (also on a caller's stream). */
int pg_graph_kernel_stats(pg_graph* g, int reset, double* total_ms, uint64_t* launches, uint64_t* blocks);
/* The same for the launches of the main mixer's effect chain (one workgroup per effect behind the sum: a latency chain — for graphs whose
 * work is mostly on the bus, BASELINE configs 2 and 4, it is the launch that dominates by GPU time), and its name. */
int pg_graph_bus_kernel_stats(pg_graph* g, int reset, double* total_ms, uint64_t* launches, uint64_t* blocks);
/* What a workload off the steady state costs (events, voices that start and end, ramps): out[0] = unit-blocks rendered since the last reset
 * (units x blocks of max_frames), out[1] = unit-blocks that left the time-parallel kernels for the generic kernel, out[2] = generic launches
 * issued, out[3] = those that found work; *generic_ms / *generic_timed = GPU time and count of the generic launches that were hipEvent-timed
 * (pg_graph_set_timing_period). Waits for the graph's stream. Measurement only (bench.py --workload dyn). */
int pg_graph_dynamic_stats(pg_graph* g, int reset, uint64_t out[4], double* generic_ms, uint64_t* generic_timed);
const char* pg_graph_bus_kernel(pg_graph* g);
/* The hipEvent pair behind pg_graph_kernel_ms costs ~8 us of stream time per round: time every n-th round only (default 1 = every
 * round, 0 = never). pg_graph_kernel_ms then averages over the timed rounds and reports their count. */
int pg_graph_set_timing_period(pg_graph* g, int every_n_rounds);
/* Name(s) of the kernel launch(es) the pg_graph_kernel_ms events bracket for this graph (static string). */
const char* pg_graph_dominant_kernel(pg_graph* g);
/* 0 = exact serial filters, 1 = time-parallel (blocked) evaluation of linear filters (default) */
int pg_graph_set_fast_math(pg_graph* g, int level);
/* How sub-mixers whose chain ends in a Reverb behind Gain / Panning (and, in mode 1, Filter / Eq5 / Delay / Distortion) effects
 * are rendered: 1 (default) = staged kernel (stage functions over a per-stage LDS plan in one launch, four workgroups per CU),
 * 2 = one launch per stage (profiling; Gain / Panning chains only), 0 = the fused fast kernel. Same stage functions in every mode: results agree up to f64 rounding. */
int pg_graph_set_staged(pg_graph* g, int mode);

#ifdef __cplusplus
}
#endif
#endif /* PHONIC_GPU_H */
