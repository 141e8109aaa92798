// Device-resident state of the phonic DSP hot path (HBM layout). Plain-old-data, shared by the host
// side (graph construction, C ABI) and the gfx950 kernels. All delay lines keep the reference's f64
// ring layout and index arithmetic (reference src/utils/dsp/delay.rs) so state is comparable with the
// CPU oracle after every block.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define PG_USIZE_MAX 0xFFFFFFFFFFFFFFFFull
#define PG_MAX_FRAMES 4096  // MixedSource::MAX_MIX_BUFFER_SAMPLES / 2 (src/source/mixed.rs:216)
// Semantic chunks and kernel pieces. MixedSource::write walks a call in chunks of min(remaining, PG_MAX_FRAMES) frames from the call's
// start and from every event (mixed.rs:679-712); sources, effect processors and sub-mixers are called once per chunk and take their
// per-call decisions (bypass, tails, silence gates, block-end bookkeeping) there. The kernels render a chunk as PIECES of at most the
// graph's max_frames frames (LDS-resident, <= 1024 for the staged kernels): per-chunk decisions are taken at a chunk's first piece, kept in
// the unit / effect / voice records and closed at its last piece, so the chunk grid is the reference's whatever max_frames is.

enum PgSmoothKind { SM_EXP = 0, SM_LIN = 1, SM_SPRING = 2 };

// ExponentialSmoothedValue / LinearSmoothedValue / SpringSmoothedValue (src/utils/smoothing.rs)
struct PgSmooth {
  int32_t kind;
  float current, target;
  float a;      // inertia | step | omega
  float b;      // -       | current_step | velocity
  float comp;   // 44100 / sample_rate
  uint32_t pending;  // linear: num_pending_steps
};

// BiquadFilterCoefficients (src/utils/dsp/filters/biquad.rs:31-43)
struct PgBiquadCoef {
  int32_t type;
  uint32_t sample_rate;
  float cutoff, q, gain;
  int32_t pad;
  double a1, a2, a3, m0, m1, m2;
};
// SvfFilterCoefficients (src/utils/dsp/filters/svf.rs:30-41)
struct PgSvfCoef {
  int32_t type;
  uint32_t sample_rate;
  float cutoff, resonance;
  double g, k, a1, a2, a3;
};
struct PgState2 { double ic1eq, ic2eq; };      // BiquadFilter / SvfFilter state
struct PgDc { double y1, x1, r; };             // DcFilter (src/utils/dsp/filters/dc.rs:35-39)
struct PgLfo { float phase, phase_inc; int32_t waveform; };  // Lfo (src/utils/dsp/lfo.rs:52-60), deterministic shapes

struct PgGain {  // GainEffect (src/effect/gain.rs:47-55)
  PgSmooth gain;
  int32_t dc_mode;  // 0 Off, 1 Slow, 2 Default, 3 Fast
  PgDc dc[2];
};
struct PgPan {  // PanningEffect (src/effect/pan.rs)
  PgSmooth pan, width;
  int32_t invert_l, invert_r;
};
struct PgFilter {  // FilterEffect (src/effect/filter.rs:47-56)
  PgBiquadCoef coef;
  PgState2 st[2];
  int32_t type;  // FilterEffectType
  PgSmooth cutoff, q;
};
struct PgEq5 {  // Eq5Effect (src/effect/eq5.rs:18-28)
  PgSmooth gains[5], freqs[5], bws[5];
  PgBiquadCoef coef[5];
  PgState2 st[2][5];
};
struct PgDelay {  // DelayEffect (src/effect/delay.rs:88-116)
  int32_t mode, filter_type, lfo_shape;
  PgSmooth delay_time, feedback, cutoff, drive, wet, width, lfo_rate, d_time, d_feedback, d_filter;
  double* line[2];  // InterpolatedDelayLine<1> left/right
  uint32_t mask, write_pos[2];
  PgLfo lfo;
  PgSvfCoef coef;
  PgState2 flt[2];
  PgDc dc[2];
  float fb[2];
  // Lfo's random shapes (lfo.rs:56-59): sample & hold value, the two ends of the smooth-random segment, and the generator —
  // rand ^0.9 SmallRng = Xoshiro256++, its state an explicit input (pg_effect_init::lfo_rng_state)
  float lfo_sample_hold, lfo_jitter_current, lfo_jitter_target, lfo_pad;
  uint64_t lfo_rng[4];
};
struct PgReverbLine {  // ReverbDelayLine<2> (src/effect/reverb.rs:518-529)
  double* buf;         // [(size+1)][2]
  uint32_t frames, count, delay, pad;
  double feedback[2];
  double depth;
  double vib_phase[2];
};
struct PgAllpass {  // AllpassDelayLine<2> (src/utils/dsp/delay.rs:283-287)
  double* buf;      // [size][2]
  uint32_t frames, delay, write_pos, pad;
};
struct PgReverb {  // ReverbEffect (src/effect/reverb.rs:41-73)
  PgSmooth room, wet;
  PgBiquadCoef ca, cb, cc;
  PgState2 sa[2], sb[2], sc[2];
  uint32_t fpd_l, fpd_r;
  PgReverbLine line[8];
  PgAllpass ap[4];
  double* pre;  // DelayLine<2>, pow2 4096 frames
  uint32_t pre_mask, pre_write_pos;
  // block parameters of the steady state (fast path): valid while room/wet targets are unchanged
  float cache_room, cache_wet;
  int32_t cache_valid;
  uint32_t c_predelay;
  double c_blend, c_regen;
  const double* vib_tab;  // [8][129][2]: cos(j*d_i), sin(j*d_i) of the per-frame vibrato increment d_i = depth_i * 0.1 (shared, read-only)
};
struct PgChorus {  // ChorusEffect (src/effect/chorus.rs:47-75)
  PgSmooth rate, phase, depth, feedback, delay, wet, freq, res;
  int32_t filter_type;
  float lfo_range;
  double current_phase;
  PgLfo osc[2];
  double* line[2];
  uint32_t mask, write_pos[2];
  PgSvfCoef coef;
  PgState2 flt[2];
};
struct PgComp {  // CompressorEffect (src/effect/compressor.rs:24-38)
  float threshold, ratio, knee, attack, release, lookahead;
  PgSmooth makeup;
  float env_current, env_attack, env_release;
  double* line;  // LookupDelayLine<2>
  uint32_t line_frames;  // allocated frames (pow2 >= ceil(0.2*sr))
  uint32_t mask, delay_frames, write_pos, peak_pos;
  double peak_value;
};
struct PgGate {  // GateEffect (src/effect/gate.rs)
  float threshold, attack, hold, release, range;
  float env_current, env_attack, env_release;
  uint32_t hold_counter;
  float gate_gain_db, attack_coeff, release_coeff;
};
struct PgDist {  // DistortionEffect (src/effect/distortion.rs:194-204)
  int32_t type;
  PgSmooth drive, mix;
  const float* luts;  // [5][256], shared, built on the host at create
};

struct PgFx {
  int32_t kind;
  uint32_t sample_rate;
  // EffectProcessor (src/source/mixed/effect.rs:12-17)
  int32_t bypassed;
  int32_t standalone;  // 1: plain Effect::process without the processor's bypass logic
  uint64_t tail_counter, silence_counter;
  // the process call (semantic chunk) in progress, across its pieces: frames the effect has rendered so far and — while the processor
  // watches for silence (unknown tail, effect.rs:128-144) — the peak of what it put out
  uint32_t call_frames;
  float call_max;
  // ... and the branch the effect's process() took where the call began: FilterEffect and Eq5Effect test `value_need_ramp` once per call
  // (filter.rs:167, eq5.rs:298-303) and keep recomputing their coefficients from the smoothers for the rest of it — a smoother that stops
  // ramping inside the call then hands out its TARGET, while the other branch runs on the coefficients the last ramp frame left (from the
  // smoother's `current`, up to the ramp threshold away): the branch must not change between the pieces of a call
  uint32_t call_ramp;
  uint32_t pad_call;
  union {
    PgGain gain; PgPan pan; PgFilter filter; PgEq5 eq5; PgDelay delay; PgReverb reverb; PgChorus chorus; PgComp comp; PgGate gate; PgDist dist;
  } u;
};

// PreloadedFileSource + ChannelMapped + Amplified + Panned + PlayingSource (one "voice")
struct PgVoice {
  const float* pcm;        // device copy of AudioFileBuffer (+1 zero frame)
  uint64_t n_samples;      // buffer.len()
  uint32_t channels;       // file channels (1 or 2)
  uint32_t src_rate, out_rate;
  // CubicInterpolator per channel (src/utils/resampler/cubic.rs:10-15)
  float input[2][4];
  float sub_pos[2];
  float ratio;
  int32_t initialized[2];
  // PreloadedFileSource (src/source/file/preloaded.rs:29-37)
  uint64_t playback_pos, repeat, repeat_count;
  int32_t pos_eof, finished;
  int32_t has_loop;
  uint64_t loop_start, loop_end;  // frames
  // VolumeFader (src/utils/fader.rs:27-34)
  int32_t fader_state;  // 0 Stopped 1 Running 2 Finished
  float fader_current, fader_target, fader_inertia;
  float fade_out_seconds;
  // AmplifiedSource / PannedSource smoothers
  PgSmooth volume, panning;
  // PlayingSource (src/source/mixed.rs:34-42)
  uint64_t start_time, stop_time;
  int32_t has_stop, active;
  // speed / glide (FileSourceImpl, src/source/file/common.rs:47-52)
  double current_speed, target_speed;
  float speed_glide_rate;
  uint32_t samples_to_next_speed_update;
  int32_t sched_class, sched_rep;  // resampler schedule cache: class of voices sharing a ratio; 1 = this voice publishes the schedule
  int32_t sched_hit;               // device: how the last resampling piece got its schedule: 0 serial replay, 1 schedule cache, 2 time-parallel
  uint32_t stop_pos_lo;            // device: playback_pos (low word; stop_pos_hi below) as the source write that reached the voice's stop time left it — the next
                                   // write begins there with the Stop message (mixed.rs:584-603) and moves playback_pos on; playback status reads it (pg_k_status.hip)
  // ResampledSource around the file source (src/source/resampled.rs:27-98), present when the file source runs at a rate (`out_rate`) other
  // than the mixer's (pg_voice_options::source_rate): cubic interpolator state per channel + the two 512-frame TempBuffers
  int32_t outer_on, outer_pending_stop;
  int32_t outer_init[2];
  float outer_ratio;
  uint32_t stop_pos_hi;            // (see stop_pos_lo)
  float outer_sub_pos[2];
  float outer_input[2][4];
  uint32_t in_start, in_end, out_start, out_end;  // TempBuffer ranges (samples)
  float* stage_in;   // device memory: 512 * channels floats each
  float* stage_out;
  // Host-fed source (pg_graph_add_stream_voice): `pcm` is a device ring of stream_cap frames that the host fills (pg_graph_feed_voice),
  // playback_pos counts the frames read; stream_fed = frames fed so far, bit 63 = the host has ended the stream
  int32_t stream_on;
  uint32_t stream_cap;
  uint64_t stream_fed;
  // MixedSource::process_sources marks an exhausted transient source inactive but keeps calling it for the rest of the write; it is removed
  // when the write ends (mixed.rs:612-616, 715). Only a ResampledSource makes that audible (asked again, it refills its stale input range and
  // plays on): the end position of the write in which such a voice was marked.
  uint64_t zombie_end;
  // process_sources leaves a source alone for the rest of a chunk once a write returned nothing (`written == 0` -> break 'source,
  // mixed.rs:617-620): set when that happens in a piece, cleared at the first piece of the mixer's next chunk
  int32_t chunk_skip;
  int32_t persistent;  // host: !PlayingSource::is_transient — an exhausted source stays in the mixer's list (mixed.rs:612-620)
};

// AhdsrEnvelope + AhdsrParameters of one voice (src/utils/ahdsr.rs:26-39, :367-373): the sampler's volume envelope around the voice chain
// (src/generator/sampler/voice.rs:28-30, :469-486). Kept in a side table indexed by the voice's device index (PgLaunch::env) — PgVoice is
// staged in LDS one dword per lane by every kernel and does not grow for a feature only the exact kernel renders.
enum PgAhdsrStage { PG_AHDSR_IDLE = 0, PG_AHDSR_ATTACK = 1, PG_AHDSR_HOLD = 2, PG_AHDSR_DECAY = 3, PG_AHDSR_SUSTAIN = 4, PG_AHDSR_RELEASE = 5 };
enum { PG_AHDSR_HOLD_ZERO = 1, PG_AHDSR_DECAY_ZERO = 2, PG_AHDSR_RELEASE_ZERO = 4 };   // PgEnvParams::zero_times: `Duration::is_zero()` of the three times
struct PgEnvState {  // AhdsrEnvelope
  int32_t stage;
  float target_volume, hold_samples_remaining, release_output, output;
};
struct PgEnvParams {  // AhdsrParameters after set_sample_rate(graph rate); a zero attack / decay / release time is a rate of f32::MAX
  float attack_rate, decay_rate, release_rate;
  float attack_scaling, decay_scaling, release_scaling;
  float sustain_level;
  float hold_samples;   // hold_time.as_secs_f32() * sample_rate as f32
  int32_t zero_times;
};
struct PgEnv {
  int32_t on;           // 0: the voice has no envelope
  PgEnvState state;
  PgEnvParams params;
  int32_t pad;
};
// The side table in device memory: this header, then one PgEnv per voice, indexed like PgLaunch::voices. `done`: one word per voice in mapped
// host memory that the exact kernel sets when an enveloped voice has ended — the host then takes the voice's unit off the exact kernel again.
struct PgGrainVoice;
struct PgStatVoice;
struct PgSamplerTab;
struct PgEnvTable {
  int32_t* done;
  uint64_t cap;         // entries behind the header: the kernel takes no entry at or beyond it
  // granular voices (pg_graph_add_granular_voice): the per-voice side table travels behind the same word of PgLaunch. grain_of_voice[v] (v < cap):
  // index of voice v's record in `grains`, -1 for every other voice; nullptr: the graph never had a granular voice.
  const int32_t* grain_of_voice;
  PgGrainVoice* grains;
  uint32_t n_grains;    // records `grains` holds: no record at or beyond it is taken
  // playback status (pg_graph_set_voice_status): stat_of_voice[v] (v < cap) = index of voice v's record in `stats`, -1 for every other voice;
  // nullptr: status was never enabled on the graph. The exact kernel logs the source writes of such a voice there (PgStatVoice below).
  uint32_t n_stats;     // records `stats` holds: no record at or beyond it is taken
  const int32_t* stat_of_voice;
  PgStatVoice* stats;
  // samplers (pg_graph_add_sampler): the records of the note layer (PgSamplerTab below) travel behind the same word; nullptr: the graph never had one
  PgSamplerTab* samplers;
};
static_assert(sizeof(PgEnv) == 64 && sizeof(PgEnvTable) == 64, "the entries follow the header, 16-byte aligned");

// ---- the Sampler's note layer (pg_graph_add_sampler; pg_note_dev.h, pg_sampler_dev.h): notes, voice allocation and stealing (src/generator/sampler.rs) ----
// A sampler is a pool of n_voices file voices (ordinary PgVoice records, device indices voice0 .. voice0 + n_voices - 1, + a PgEnv each when it has
// an envelope) in ONE sub-mixer unit: the exact kernel's workgroup of that unit applies the sampler's commands in front of their frames, from the
// state its source stage left in the pool's voices. Slot i is ACTIVE (SamplerVoice::is_active, voice.rs:100-102) iff its voice is `active` and
// not `finished`: voice_process marks the voice finished in the source write that exhausts the file, lets the fader arrive or finds the
// envelope Idle — the write in which SamplerVoice::process resets the voice (voice.rs:488-502).
#define PG_SAMPLER_MAX_VOICES 64   // one wave lane per slot (the reference takes any count, generator.rs:48-72)
struct PgSamplerSlot {             // the per-note part of SamplerVoice (voice.rs:28-60)
  uint64_t note_id;                // of the last note the slot was started with (0: none yet); what the voice holds says whether it still plays
  uint64_t release_start_frame;    // Some(frame) of SamplerVoice::stop (voice.rs:202), UINT64_MAX: None
  float note_volume, note_panning;
  int32_t note, pad;
};
// The generator's output stage of a sampler that sits on the MAIN mixer (pg_graph_add_sampler_to_main): AmplifiedSource(options.volume) and
// PannedSource(options.panning) over the Sampler's sum (player.rs:1048-1133), rendered behind the voice loop of the sampler's source unit
// (pg_sampler_dev.h: genout_*). `flags` is decided once per Sampler::write, in front of the source stage of the chunk's first piece.
enum { PG_GENOUT_DELIVERS = 1,     // the write in progress returned its whole buffer (sampler.rs:974-981): the stage runs over it
       PG_GENOUT_VOLUME_RAMPS = 2, // apply_smoothed_gain found need_ramp() at the top of the write: one next() per sample of the write
       PG_GENOUT_PAN_RAMPS = 4 };  // apply_smoothed_panning likewise: one next() per frame
struct PgGenOut {
  PgSmooth volume, panning;
  int32_t on;                      // 1: the sampler is a source of the main mixer; 0: a pool in a sub-mixer, which has no sum of its own to scale
  int32_t flags;                   // PG_GENOUT_*
};
struct PgSamplerRec {
  int32_t unit;                    // unit slot of the owning sub-mixer; of the sampler's own source unit on the main mixer
  int32_t voice0, n_voices;
  int32_t has_envelope, transient;
  int32_t stopping, stopped;       // sampler.rs:733-738, :1011-1024
  int32_t transpose, finetune;     // base parameters (sampler.rs:1076-1120) ...
  float base_volume, base_panning;
  int32_t pad;
  double pitch_factor;             // ... and 2^(transpose / 12 + finetune / 1200) as the host's libm gives it (voice.rs:146-147)
  PgSamplerSlot slots[PG_SAMPLER_MAX_VOICES];
  PgGenOut out;                    // (a granular sampler's too: the record is inert for its notes, n_voices 0, but holds its output stage)
};
struct PgGSampler;
struct PgSamplerTab {
  uint32_t n, pad;                 // records behind the header: no record at or beyond it is taken
  const double* speed_tab;         // speed_from_note(0 .. 255) (utils.rs:67-78), host-computed
  int32_t* stopped;                // mapped host memory, one word per record: set with PgSamplerRec::stopped
  const PgGSampler* gsamp;         // the granular-mode samplers' records, indexed like the ones behind the header (nullptr: the graph has none)
};
static_assert(sizeof(PgSmooth) == 28 && sizeof(PgGenOut) == 64, "host and device agree on the layout");
static_assert(sizeof(PgSamplerSlot) == 32 && sizeof(PgSamplerRec) == 56 + 32 * PG_SAMPLER_MAX_VOICES + 64 && sizeof(PgSamplerTab) == 32, "host and device agree on the layout");

// ---- playback status events (pg_graph_set_voice_status; pg_k_status.hip) ----
// PlaybackStatusEvent::Position / Stopped are decided once per Source::write call of the voice (src/source/file/preloaded.rs:396-475,
// src/source/file/common.rs:171-221, src/generator/sampler/voice.rs:434-502). pg_playback_status_kernel runs behind every launch of a level that holds
// such a voice and keeps one PgStatVoice per voice: the emit clock, the voice's state as the launch before left it, and the source write in
// progress. A launch of the time-parallel kernels holds one segment per unit: one source write (or part of one) per voice, or two where the
// voice's stop time lies inside the launch — the status kernel reads what the last one left in PgVoice, and playback_pos behind the one that
// ended at the stop time in PgVoice::stop_pos_lo / _hi, which every kernel's voice_process leaves there. The exact kernel can render several source writes of a voice in one launch (a chunk cut
// by events, a stop time inside the piece): it logs every write that ENDS in the launch here, and stamps the record with the launch's round.
#define PG_STAT_LOG 32                   // source writes of one voice the exact kernel can log per launch; later ones are counted in `lost`
enum { PG_SW_EOF = 1,                    // playback_pos_eof behind the write
       PG_SW_FINISHED = 2,               // playback_finished behind the write (for a sampler voice: the voice was reset, voice.rs:488-495)
       PG_SW_SKIPPED = 4,                // the source was finished when the write began: it returned at once (preloaded.rs:400-403), nothing is sent
       PG_SW_KILLED = 8,                 // a stop without a fade-out, taken by process_messages in front of the write: Stopped, then nothing (preloaded.rs:196-208)
       PG_SW_EOF_BEFORE = 16 };          // playback_pos_eof as the write began (what that Stopped carries)
struct PgStatWrite {
  uint64_t time;                         // SourceTime::pos_in_frames of the write
  uint64_t pos;                          // sample_pos behind it: playback_pos, or the grain pool's (voice.rs:463)
  int32_t flags, pad;
};
enum { PG_SV_POSITION = 1,               // playback_pos_emit_rate is Some(emit_rate)
       PG_SV_STOPPED = 2,                // Stopped records are wanted
       PG_SV_GRANULAR = 4,               // a sampler voice in granular mode: start event, position from the pool, two Stopped records
       PG_SV_STARTED = 8 };              // grain_pool_started (voice.rs:169, :456-457): the next Position is a start event
struct PgStatVoice {
  int32_t voice;                         // device index of the voice (PgLaunch::voices)
  int32_t voice_id;                      // the id the host knows it by (what the records carry)
  int32_t flags;                         // PG_SV_*
  uint32_t log_round;                    // PgLaunch::round of the last launch in which the exact kernel rendered the voice's unit
  uint64_t emit_rate;                    // playback_pos_emit_rate in frames
  uint64_t clock_start;                  // SampleTimeClock::start_time of playback_pos_sample_time_clock (time.rs:19-55)
  uint32_t channels, rate;               // channel_count and sample_rate of the FILE buffer (common.rs:195-196)
  uint64_t buffer_len;                   // granular voices: file_buffer.buffer().len() (voice.rs:463)
  // the voice as the last launch left it (what the next launch's source write finds)
  int32_t prev_active, prev_finished, prev_has_stop, prev_pos_eof, prev_chunk_skip, pad_prev;
  uint64_t prev_stop_time;
  // the source write in progress: begun in an earlier launch of the chunk, it goes on in the next one
  int32_t open, open_flags;
  uint64_t open_time;
  int32_t n_log, lost;                   // entries of `log` the exact kernel left in the current launch; writes it could not log
  PgStatWrite log[PG_STAT_LOG];
};
static_assert(sizeof(PgStatWrite) == 24 && sizeof(PgStatVoice) % 8 == 0, "host and device agree on the layout");
// One lane of pg_playback_status_kernel: the record it works on, where the launch sits, and the fixed slots its records go to. The jobs and the slots are
// mapped host memory: the kernel fills the slots, then `count`; the host compacts the slots after the call (pg_status_host.h).
struct PgStatJob {
  int32_t rec;                           // index into the graph's PgStatVoice records
  int32_t slot0, n_slots;                // the job's record slots
  int32_t count;                         // device: records written (-1 until the kernel has run), ...
  int32_t lost;                          // ... records that found no slot + source writes the exact kernel could not log
  uint32_t round;                        // PgLaunch::round of the launch this job stands behind
  uint64_t t0;                           // position of the launch's first frame
  uint32_t n;                            // frames of the launch
  int32_t first;                         // the launch is the first piece of its chunk of the main mixer
  uint64_t chunk_end;                    // position at which that chunk ends
  // host only: where the voice stands in the reference's traversal of that write, and the sub-mixer of the main mixer it sits under (0: none)
  uint32_t rank;
  int32_t top;
};
static_assert(sizeof(PgStatJob) == 56, "host and device agree on the layout");

// ---- granular voices: GrainPool<100> of a sampler voice (src/generator/sampler/granular.rs), see pg_grain_dev.h / pg_k_grain.hip ----
#define PG_GRAIN_POOL 100      // Sampler's GrainPool<100>: concurrent grains of one voice
#define PG_GRAIN_LUT_N 2048    // GRAIN_WINDOW_LUT: GrainWindow<2048> (granular.rs:221)
#define PG_GRAIN_WINDOWS 8     // GrainWindowMode::COUNT
struct PgGrain {               // Grain (granular.rs:961-985)
  double position, increment, window_phase, window_increment;
  double loop_start, loop_end;         // loop_range: Some((start, end)) when has_loop
  uint64_t samples_remaining;
  float volume, panning;
  int32_t active, window_mode, has_loop, pad;
};
struct PgGrainPool {           // the mutable scalars of GrainPool (granular.rs:345-377)
  uint64_t rng[4];             // SmallRng = Xoshiro256++
  double speed;
  float trigger_phase, playhead, volume, panning;
  int32_t playing_loop_range, trigger_new_grains, primary /* primary_grain_index, -1: None */;
  int32_t overlap_mode;        // the pool's own copy (granular.rs:346): Cloud from GrainPool::new until the first frame's try_trigger_grain takes the parameters' (:535-538)
};
struct PgGrainParams {         // GranularParameters (granular.rs:241-266) + GrainPool::sample_loop_range; CMD_VOICE_GRAIN_PARAM / _LOOP change them while the voice plays
  int32_t overlap_mode, window;
  float size, density, variation, spray, pan_spread;
  int32_t direction;
  float position, step;
  int32_t has_loop;
  float loop_start, loop_end;
  int32_t pad;
};
// The ModulationMatrix of a granular sampler voice (src/modulation/matrix.rs, src/generator/sampler/modulation.rs): two LFO slots, the velocity
// and the keytracking slot, routed to the seven granular targets of Sampler::modulation_config (sampler.rs:392-427).
#define PG_GMOD_SOURCES 4      // slot order: LFO 1, LFO 2, velocity, keytracking
#define PG_GMOD_TARGETS 7      // GRAIN_SIZE, _DENSITY, _VARIATION, _SPRAY, _PAN_SPREAD, _POSITION, _STEP
struct PgModLfo {              // Lfo (src/utils/dsp/lfo.rs:52-60), all seven shapes, with its generator (SmallRng = Xoshiro256++)
  float phase, phase_inc;
  int32_t waveform;            // LfoWaveform 0..6
  float sample_hold, jitter_current, jitter_target;
  int32_t pad[2];
  uint64_t rng[4];
};
struct PgGrainMod {
  int32_t on, pad;
  float velocity, note_pitch;  // VelocityModulationProcessor::velocity, KeytrackingModulationProcessor::note_pitch (processor.rs:236-244, :292-298)
  PgModLfo lfo[2];
  float amount[PG_GMOD_SOURCES][PG_GMOD_TARGETS];     // the slot's target for the parameter (matrix.rs:60-83): 0.0 = none (a route's |amount| is >= 0.001)
  int32_t bipolar[PG_GMOD_SOURCES][PG_GMOD_TARGETS];
  float last[PG_GMOD_TARGETS]; // the seven sums of the last rendered frame (voice.rs:435-446 reads the position's)
  int32_t pad_last;
};
struct PgGrainVoice {
  PgGrainParams params;
  PgGrainPool pool;
  const float* pcm;            // GrainPool::sample_buffer: mono f32 at the graph's rate
  uint64_t n_frames;
  float* staged;               // PG_MAX_FRAMES interleaved stereo frames: what pg_grain_kernel rendered of the main mixer's current chunk ...
  uint64_t stage_pos;          // ... whose frame 0 is this position
  uint64_t start_time;         // the voice's start time: no frame in front of it is rendered
  uint64_t stop_time;          // StopSource: GrainPool::stop() in front of the first frame at or behind it (UINT64_MAX: none)
  uint64_t exhausted_at;       // position of the frame behind which GrainPool::is_exhausted() first held (UINT64_MAX: not yet)
  int32_t voice;               // device index of the voice (PgLaunch::voices)
  int32_t has_env;             // the voice has a volume envelope: CMD_VOICE_RELEASE is its note_off, not a stop
  float* pos_trace;            // playback status (pg_graph_set_voice_status): PG_MAX_FRAMES floats, GrainPool::playback_position behind every rendered frame of
                               // the staged chunk (frame f of the chunk in word f); nullptr: the voice reports nothing and pg_grain_kernel leaves it out
  PgGrain grains[PG_GRAIN_POOL];
  PgGrainMod mod;              // the voice's ModulationMatrix (pg_graph_set_voice_modulation_matrix); mod.on == 0: none, every `*_mod` is left out
};
static_assert(sizeof(PgGrain) == 80 && sizeof(PgGrainPool) == 72 && sizeof(PgGrainParams) == 56 && sizeof(PgGrainVoice) % 8 == 0, "host and device agree on the layout");
static_assert(sizeof(PgModLfo) == 64 && sizeof(PgGrainMod) == 400 && offsetof(PgGrainVoice, mod) % 8 == 0, "host and device agree on the layout");

// ---- granular-mode samplers (pg_graph_add_granular_sampler; pg_gsampler_dev.h / pg_k_gsampler.hip): Sampler::with_granular_playback ----
// A pool of note.n_voices granular voices that notes start, steal and release. Slot k renders through PgGrainVoice record grain0 + k (pg_grain_kernel)
// into that record's staging buffer; the sub-mixer unit takes the frames through PgVoice note.voice0 + k, which is always `active` and carries no
// envelope of the unit kernel's: whether a slot plays, its envelope and its end are THIS record's, decided by pg_gsampler_kernel between the
// grain launches of consecutive Sampler::write spans. The sampler's PgSamplerRec in PgSamplerTab (same index: CMD_SAMPLER_*'s target) has
// n_voices 0, so the unit kernel's sampler_command leaves its commands alone. A FREE slot's grain record has start_time UINT64_MAX.
struct PgGSampler {
  PgSamplerRec note;               // as for a file sampler; note.unit = the owning sub-mixer's unit slot
  int32_t grain0;                  // slot 0's record in the graph's PgGrainVoice table
  int32_t index;                   // CMD_SAMPLER_*'s target
  uint64_t start_time;             // the mixer calls the sampler from here on
  uint64_t span_t0;                // first frame of the Sampler::write span that is open (UINT64_MAX: none)
  PgEnvParams env_params;          // with note.has_envelope
  int32_t delivers;                // the Sampler::write that began at the last boundary returns its whole buffer (sampler.rs:974-981): not stopped, and a slot
                                   // is active or the sampler is stopping, the messages of that frame applied. What the output stage of a main-mixer sampler asks.
  PgEnvState env[PG_SAMPLER_MAX_VOICES];
  int32_t active[PG_SAMPLER_MAX_VOICES];   // SamplerVoice::is_active (voice.rs:100-102)
};
static_assert(sizeof(PgGSampler) % 8 == 0, "host and device agree on the layout");
struct PgCmd;
struct PgGSamplerLaunch {
  PgGSampler* recs;                // the graph's granular-sampler records ...
  const int32_t* live;             // ... and the ones workgroup b of the launch works on: live[b]
  uint32_t n_recs;                 // records `recs` holds: no record at or beyond it is taken
  uint32_t n_live;
  uint32_t n_grains;               // records `grains` holds: no record at or beyond it is taken
  PgGrainVoice* grains;
  const PgCmd* cmds;               // the command list of the piece that holds frame `t` (PgLaunch::cmds) ...
  int32_t n_cmds;
  uint32_t frame;                  // ... and t relative to that piece's first frame
  uint64_t t;                      // position of the boundary: the spans that end here are closed, the messages due here applied
  uint64_t chunk_t0;               // position of frame 0 of the staging buffers: the start of the main mixer's chunk
  int32_t chunk_first;             // t is the chunk's first frame: a boundary of every sampler
  int32_t closing;                 // t is the chunk's end: close only
  const double* speed_tab;         // PgSamplerTab::speed_tab
  int32_t* stopped;                // PgSamplerTab::stopped (mapped host memory, indexed by PgGSampler::index)
};

// Parameter indices per effect kind = order of `Effect::parameters()` in the reference.
enum { P_GAIN_GAIN = 0, P_GAIN_DCFM };
enum { P_PAN_PAN = 0, P_PAN_WIDTH, P_PAN_INVL, P_PAN_INVR };
enum { P_FILTER_TYPE = 0, P_FILTER_CUTOFF, P_FILTER_Q };
// Eq5: index = band * 3 + {0 gain, 1 frequency, 2 bandwidth}
enum { P_DELAY_MODE = 0, P_DELAY_TIME, P_DELAY_FEEDBACK, P_DELAY_FTYPE, P_DELAY_CUTOFF, P_DELAY_DRIVE, P_DELAY_WET, P_DELAY_WIDTH,
       P_DELAY_LFO_RATE, P_DELAY_LFO_SHAPE, P_DELAY_D_TIME, P_DELAY_D_FEEDBACK, P_DELAY_D_FILTER };
enum { P_REVERB_ROOM = 0, P_REVERB_WET };
enum { P_CHORUS_RATE = 0, P_CHORUS_DEPTH, P_CHORUS_FEEDBACK, P_CHORUS_DELAY, P_CHORUS_WET, P_CHORUS_PHASE, P_CHORUS_FTYPE, P_CHORUS_FREQ,
       P_CHORUS_RES };
enum { P_COMP_THRESHOLD = 0, P_COMP_RATIO, P_COMP_KNEE, P_COMP_ATTACK, P_COMP_RELEASE, P_COMP_MAKEUP, P_COMP_LOOKAHEAD };
enum { P_GATE_THRESHOLD = 0, P_GATE_ATTACK, P_GATE_HOLD, P_GATE_RELEASE, P_GATE_RANGE };
enum { P_DIST_TYPE = 0, P_DIST_DRIVE, P_DIST_MIX };

// Resampler schedule cache. The f32 `sub_pos` recurrence of the cubic resampler depends only on (ratio, sub_pos, number of
// output frames) — not on the audio — so voices that run in lock step (same ratio, same state) share one schedule: the
// class representative computes the NEXT block's schedule at the end of its workgroup and every voice whose state
// matches the key bit for bit copies it instead of replaying the serial recurrence (any mismatch -> own replay).
#define PG_SCHED_CAP 1024
struct PgSchedEntry {
  uint32_t ratio_bits, subpos_in_bits;  // key
  int32_t piece, valid;
  uint32_t subpos_out_bits;             // state after the piece
  int32_t c_total;                      // input frames consumed by the piece
  uint16_t sched_c[PG_SCHED_CAP];
  float sched_f[PG_SCHED_CAP];
};

enum PgUnitKind { UNIT_SUBMIXER = 0, UNIT_SOURCE = 1, UNIT_BUS = 2, UNIT_EFFECT = 3 };

struct PgUnit {
  int32_t kind;
  int32_t n_voices, voice_off;  // into the voice index table
  int32_t n_fx, fx_off;         // into the fx index table
  int32_t effects_bypassed;     // MixedSource::effects_bypassed (src/source/mixed.rs:202)
  uint64_t silence_counter;     // SubMixerProcessor (src/source/mixed/submixer.rs:23)
  int32_t audible;              // result of the last chunk: contributes to the parent's `audible_input`
  int32_t deferred;             // set by the fast kernel when the unit must be rendered by the generic kernel
  int32_t static_defer;         // host: the chain holds an effect kind without a time-parallel path -> always generic kernel (no stock kind or layout sets it any more)
  int32_t maybe_ramping;        // device: a parameter command was applied and some smoother may still ramp (cleared by the generic
                                // kernel once every effect of the unit is back in steady state)
  int32_t voice0;               // host: device index of the unit's first voice (skips one dependent load at kernel start)
  int32_t fx0;                  // host: device index of the unit's first effect (prefetched during the source stage)
  int32_t staged;               // host: reverb-terminated chain, eligible for the staged pipeline: 1 lean, 2 wide leading effects, 3 wide + source adapters (pg_stage_body.inl)
  int32_t stage_flags;          // device: hand-over between the stage kernels of one block (PG_STAGE_*)
  int32_t child_off, n_children;  // host: nested sub-mixers of this mixer, entries of PgLaunch::child_rows (summed before the sources)
  int32_t seg_idx;              // device: semantic chunks this mixer has begun in the main mixer's current chunk, minus one (indexes its sub-mixers' call_audible)
  uint64_t call_audible;        // device: bit k = result of SubMixerProcessor::process for the k-th call of the main mixer's current chunk (a parent
                                // with events inside it calls its sub-mixers once per segment, mixed.rs:679-712)
  // device: the chunk (this mixer's own MixedSource::write chunk) and the call (SubMixerProcessor::process of its parent) in progress, across pieces
  int32_t chunk_audible_input;  // audible_input of the chunk, decided at its first piece (process_effects and every processor of the chain use it)
  int32_t chunk_any_audible;    // main-mixer sources: OR of `produced_output` over the pieces so far
  float call_max;               // peak of the call's output so far (submixer.rs:57: max_abs over the whole call)
  uint32_t call_frames;         // frames of the call rendered in earlier pieces
  int32_t call_idx;             // calls finished in the main mixer's current chunk
  int32_t sampler;              // host, a source unit: index + 1 of the sampler whose whole pool the unit holds (pg_graph_add_sampler_to_main); 0: none
};
enum { PG_STAGE_ACTIVE = 1, PG_STAGE_INPUT_BYPASSED = 2, PG_STAGE_ALL_BYPASSED = 4, PG_STAGE_AUDIBLE = 8, PG_STAGE_SKIPPED = 16,
       PG_STAGE_FIRST = 32, PG_STAGE_LAST = 64 };  // the block is the first / last piece of its chunk

enum PgCmdType {
  CMD_FX_PARAM = 0,     // target = fx index, param = parameter index, value = raw (already denormalized/clamped) value
  CMD_FX_RESET = 1,
  CMD_VOICE_VOLUME = 2, // target = voice index
  CMD_VOICE_PAN = 3,
  CMD_VOICE_STOP = 4,   // sets stop_time = value64
  CMD_VOICE_SPEED = 5,  // value64 = f64 bits of the speed, value = glide (semitones/s, <= 0: none)
  CMD_VOICE_SEEK = 6,   // value64 = f64 bits of the position in seconds
  CMD_CALL_SPLIT = 7,   // nested sub-mixers: an ancestor splits its block at `frame` -> this unit's write() call ends there and a new one begins
  CMD_NOP = 8,          // an event whose effect was removed before it came due: nothing to apply, but the mixer's block still ends a segment at its
                        // time (the reference pops the event, logs "not found" and carries on, mixed.rs:862-924 — per-call logic counts calls)
  // Markers (frame = the launch's frame count: never applied, never a split): where the unit's current chunk / call ends when that is NOT the
  // end of the main mixer's chunk — the unit (CHUNK_END) or one of its ancestors (CALL_END) has its next event at position value64, inside the
  // main chunk but beyond this piece. The kernels close per-chunk / per-call state at a piece's end when the marker's position is that end.
  CMD_CHUNK_END = 9,
  CMD_CALL_END = 10,
  CMD_VOICE_RELEASE = 11,  // target = voice index: AhdsrEnvelope::note_off at `frame`; a voice without an envelope stops (stop_time = value64), voice.rs:196-212
  // the modulation matrix of a granular voice (target = voice index; pg_grain_kernel applies them in front of `frame`, the unit kernels ignore them):
  CMD_VOICE_MOD_ROUTE = 12,     // value = amount (0.0: remove the route), value64 = source | target << 8 | bipolar << 16   (ModulationMatrixSlot::update_target)
  CMD_VOICE_LFO_RATE = 13,      // value = phase_inc = (rate as f64 / sample_rate as f64) as f32, value64 = lfo                (Lfo::set_rate)
  CMD_VOICE_LFO_WAVEFORM = 14,  // value64 = lfo | waveform << 8                                                               (Lfo::set_waveform)
  // the granular parameters and loop range of a granular voice (target = voice index; pg_grain_kernel applies them in front of `frame`, the unit
  // kernels ignore them):
  CMD_VOICE_GRAIN_PARAM = 15,   // value = the raw value (an enum's index as a float), value64 = index in Sampler::granular_parameters() order   (Sampler::set_granular_parameter)
  CMD_VOICE_GRAIN_LOOP = 16,    // value = loop_start, value64 = has_loop | f32 bits of loop_end << 32                          (GrainPool::set_loop_range)
  // the messages of a sampler (target = index of its PgSamplerRec; pg_note_dev.h applies them, for a file sampler in pg_unit_kernel, in front of `frame`). A note id
  // travels in `param`: the host hands out ids below 2^31.
  CMD_SAMPLER_NOTE_ON = 17,       // param = note id, value = volume, value64 = pg_note_on_pack(note, panning)                  (Sampler::trigger_note_on)
  CMD_SAMPLER_NOTE_OFF = 18,      // param = note id                                                                            (trigger_note_off)
  CMD_SAMPLER_ALL_NOTES_OFF = 19, //                                                                                            (trigger_all_notes_off)
  CMD_SAMPLER_NOTE_SPEED = 20,    // param = note id, value = glide (semitones/s, <= 0: none), value64 = f64 bits of the speed  (trigger_set_speed)
  CMD_SAMPLER_NOTE_VOLUME = 21,   // param = note id, value                                                                     (trigger_set_volume)
  CMD_SAMPLER_NOTE_PAN = 22,      // param = note id, value                                                                     (trigger_set_panning)
  CMD_SAMPLER_PARAM = 23,         // param = PG_SP_*, value = the resolved raw value, value64 = f64 bits of the new pitch factor (TRANSPOSE / FINETUNE)
  CMD_SAMPLER_STOP = 24,          //                                                                                            (Sampler::stop)
  // a granular-mode sampler only (pg_graph_add_granular_sampler; pg_gsampler_kernel applies it, the unit kernels ignore it but end a segment at it):
  CMD_SAMPLER_GRAIN_PARAM = 25,   // param = PG_GP_*, value = the resolved raw value (an enum's index as a float)               (Sampler::set_granular_parameter)
  // what changes every voice of the pool while notes sound. The envelope command is a file sampler's (pg_unit_kernel) and a granular one's
  // (pg_gsampler_kernel); the other four are a granular sampler's only and carry what the lone voices' commands of the same name carry:
  CMD_SAMPLER_ENV_PARAM = 26,     // param = PG_SE_*, value = the field that changes (a rate, hold_samples, the sustain level), value64 = the new zero_times (AhdsrParameters::set_*)
  CMD_SAMPLER_MOD_ROUTE = 27,     // as CMD_VOICE_MOD_ROUTE, for every slot                                                     (ModulationMatrixSlot::update_target)
  CMD_SAMPLER_LFO_RATE = 28,      // as CMD_VOICE_LFO_RATE, for every slot                                                      (Lfo::set_rate)
  CMD_SAMPLER_LFO_WAVEFORM = 29,  // as CMD_VOICE_LFO_WAVEFORM, for every slot                                                  (Lfo::set_waveform)
  CMD_SAMPLER_GRAIN_LOOP = 30,    // as CMD_VOICE_GRAIN_LOOP, for every slot                                                    (GrainPool::set_loop_range)
  // the generator's output stage of a main-mixer sampler (target = index of its PgSamplerRec; pg_unit_kernel applies them in front of `frame`):
  CMD_SAMPLER_OUT_VOLUME = 31,    // value = volume                                                                             (MixerEvent::SetSourceVolume)
  CMD_SAMPLER_OUT_PAN = 32,       // value = panning                                                                            (MixerEvent::SetSourcePanning)
};
// CMD_SAMPLER_ENV_PARAM's index: Sampler::envelope_parameters() (sampler.rs:173-181)
enum { PG_SE_ATTACK = 0, PG_SE_HOLD, PG_SE_DECAY, PG_SE_SUSTAIN, PG_SE_RELEASE, PG_SE_COUNT };
enum { PG_SP_TRANSPOSE = 0, PG_SP_FINETUNE, PG_SP_VOLUME, PG_SP_PANNING, PG_SP_COUNT };   // CMD_SAMPLER_PARAM's index: Sampler::base_parameters() (sampler.rs:120-127)
// CMD_VOICE_GRAIN_PARAM's index: Sampler::granular_parameters() (sampler.rs:283-296)
enum { PG_GP_OVERLAP_MODE = 0, PG_GP_WINDOW, PG_GP_SIZE, PG_GP_DENSITY, PG_GP_VARIATION, PG_GP_SPRAY, PG_GP_PAN_SPREAD, PG_GP_DIRECTION, PG_GP_POSITION, PG_GP_STEP, PG_GP_COUNT };
#define PG_MAX_CALLS 64  // calls of one sub-mixer per launch round (bits of PgUnit::call_audible); the host bounds the round accordingly
struct PgCmd {
  int32_t type, unit, target, param;
  uint32_t frame;  // offset in frames from the start of this launch at which the command applies
  float value;
  uint64_t value64;
};
#ifdef __HIP__
#define PG_HD __host__ __device__
#else
#define PG_HD
#endif
// A sampler's message: every CMD_SAMPLER_* (the host retires them with their sampler, pg_gsampler_kernel filters its command list by it) ...
PG_HD inline bool pg_cmd_is_sampler_message(int type) { return type >= CMD_SAMPLER_NOTE_ON && type <= CMD_SAMPLER_GRAIN_LOOP; }
// ... the two of a main-mixer sampler's output stage: events of the main mixer addressed to the sampler's unit, not messages of the Sampler ...
PG_HD inline bool pg_cmd_is_sampler_output(int type) { return type == CMD_SAMPLER_OUT_VOLUME || type == CMD_SAMPLER_OUT_PAN; }
// ... and the ones pg_unit_kernel's note layer applies to a file sampler: the granular-only ones are not among them
PG_HD inline bool pg_cmd_is_unit_note_message(int type) { return (type >= CMD_SAMPLER_NOTE_ON && type <= CMD_SAMPLER_STOP) || type == CMD_SAMPLER_ENV_PARAM; }
// CMD_SAMPLER_NOTE_ON's value64: note | f32 bits of panning << 32
PG_HD inline uint64_t pg_note_on_pack(int note, float panning) { uint32_t pan; __builtin_memcpy(&pan, &panning, 4); return (uint64_t)(note & 0xff) | ((uint64_t)pan << 32); }
PG_HD inline int pg_note_on_note(uint64_t value64) { return (int)(value64 & 0xff); }
PG_HD inline float pg_note_on_panning(uint64_t value64) { const uint32_t pan = (uint32_t)(value64 >> 32); float panning; __builtin_memcpy(&panning, &pan, 4); return panning; }

// A round's command list as a kernel argument of the decision-scan kernel (rounds of at most PG_CMD_PACK commands: nearly all of them): the scan
// reads its commands from here and leaves them in the device ring for the kernels behind it — no copy kernel in front of the round (5-6 us on
// the stream in a kernel trace of the dynamic rounds).
#define PG_CMD_PACK 16
struct PgCmdPack { PgCmd c[PG_CMD_PACK]; int32_t n; int32_t pad[3]; };
#define PG_BUS_PIPELINE_MAX 16  // effects of a bus chain the pipelined launch takes (one workgroup each); longer chains stay one workgroup
struct PgLaunch {
  PgUnit* units;
  PgVoice* voices;
  PgFx* fx;
  const int32_t* voice_index;
  const int32_t* fx_index;
  const PgCmd* cmds;
  int32_t n_cmds;
  int32_t n_units;
  int32_t unit_base;      // first unit slot this launch processes (when unit_order == nullptr)
  const int32_t* unit_order;  // block b processes unit slot unit_order[b] and writes row b of unit_out
  uint32_t n_frames;      // frames of this launch (<= PG_MAX_FRAMES)
  uint64_t pos;           // SourceTime.pos_in_frames of the first frame
  uint32_t sample_rate;
  int32_t fast;           // 1: time-parallel paths enabled
  int32_t wide;           // fast kernel variant: 0 = lean (Gain/Panning/Reverb), 1 = all fast-capable kinds, 2 = all but Reverb / Compressor (four workgroups per CU)
  int32_t mode;           // 0: generic kernel, all units; 1: fast kernel (defers ineligible units); 2: generic kernel, deferred units only;
                          // 3: generic kernel, the bus chain behind a super-block as a pipeline: workgroup f = effect f of unit `unit_base`
  float* unit_out;        // [n_units][out_stride] per-unit output (sub-mixer / source results)
  uint32_t out_stride;    // floats per unit row
  float* bus;             // bus / external signal for UNIT_BUS and UNIT_EFFECT (in place); unit slot b of the launch: bus + b * bus_unit_stride
  int32_t* bus_audible;   // input flag for UNIT_BUS (1 = audible input)
  PgSchedEntry* sched;    // [n_classes][2 banks]; nullptr disables the schedule cache
  int32_t sched_bank;     // bank read by this launch; the representatives write bank ^ 1
  unsigned long long* diag;  // diagnostic builds (-DPG_DIAG): shader-clock stamps of workgroup 0, else unused
  double* stage_buf;      // [n_units][PG_STAGE_BUF_DOUBLES] f64 hand-over buffer of the staged pipeline (nullptr: pipeline off)
  const int4* slot_info;  // [n_units] per launch slot: {unit slot, device index of the first voice, device index of the last effect, number of voices | PgUnit::staged << 24}
  int32_t* defer_count;   // fast kernels append the launch slots they defer: count of this round ...
  int32_t* defer_list;    // ... and the slots; the generic kernel (mode 2) walks the list
  int32_t* defer_reset;   // the other round's counter, zeroed by the generic kernel for the next round
  int32_t* defer_state;   // pre-scanned rounds: how many of the deferred units were deferred for their STATE (static_defer / maybe_ramping) rather than for a command
  int32_t* defer_state_reset;   // ... in this round (the scan kernel counts, the generic kernel reports it: host_feedback[3]); the other round's word, zeroed like defer_reset
  unsigned long long* host_feedback;  // pinned host word: the generic kernel reports (round << 32 | units it found deferred)
  uint32_t round;         // launch counter of this round
  int32_t staged_on;      // units whose `staged` level is 1 .. staged_on are rendered by the stage kernels of this round, the fused fast kernel skips them
  uint64_t call_end;      // position at which the MixedSource::write call this launch belongs to ends (see PgVoice::zombie_end)
  const float* rows_base; // nested sub-mixers: row 0 of the per-unit output table (unit_out points at this launch's level) ...
  const int2* child_rows; // ... and {row, unit slot} of every nested sub-mixer, indexed by PgUnit::child_off
  // Super-block launch (steady state, no command inside): every workgroup of the fast / staged kernels renders n_chunks consecutive
  // blocks of n_frames for its unit — block c covers frames [pos + c * n_frames, +n_frames) and goes to unit_out + c * chunk_stride —
  // with all per-block decisions (bypass counters, silence gates, tails) taken per block exactly as in n_chunks single launches.
  // Workgroups are independent until the mixer sum, so they drift out of lock-step across the blocks. 0 / 1: one block.
  int32_t n_chunks;
  int32_t pad_chunks;
  uint64_t chunk_stride;  // floats between the per-unit output tables of consecutive blocks
  int32_t* error_word;    // device word of sticky consistency flags (PG_DEVERR_*), nullptr: not collected
  uint32_t fast_scratch_bytes;  // host: LDS arena of the fast kernels for the effect kinds this graph holds (0: the full arena)
  uint32_t pad_scratch;
  // One pointer, two launch families (the staged kernels keep a copy of this record in LDS — it must not grow): a standalone effect's launches
  // (voices == nullptr, pg_effect.hip) may carry the index log; a graph's launches (voices != nullptr) the envelope table. pg_unit_kernel only.
  union {
    int32_t* index_log;   // test hook (see FastCtx::idx_log): read indices of the time-parallel delay-line paths
    PgEnvTable* env;      // volume envelopes (pg_graph_set_voice_envelope); nullptr: no voice of the graph ever had one
  };
  // Per-block `audible` results of this level's units: block c of launch slot b -> audible_tab[c * audible_stride + b]. PgUnit::audible holds
  // the last block only; the mixer sum ORs one row of this table per block (audible_input of process_effects, mixed.rs:696-706), so the bus
  // chain behind a super-block launch sees every block's own flag. nullptr: not collected (standalone effects, bus launches).
  int32_t* audible_tab;
  uint64_t audible_stride;
  unsigned long long* bus_progress;  // mode 3 (pipelined bus chain): [PG_BUS_PIPELINE_MAX] words (round << 32 | `active` flags of the last 24 blocks << 8 | blocks done), then
                                     // [PG_BUS_PIPELINE_MAX] words with one `active` flag per block of the launch; device memory
  const int2* slot_fx;    // [n_units] per launch slot: device indices of the unit's first two effects (-1: none) — with slot_info the fast kernels
                          // request unit record, first voice and the first two effect states side by side instead of one after the other
  const int4* slot_lead;  // [n_units] per launch slot, staged units: device indices of the first three effects in FRONT of the reverb (-1: none) —
                          // stage 1 requests their state blocks when the workgroup starts (LDS-DMA), under the source stage
  uint64_t bus_unit_stride;  // floats between the external buffers of consecutive units of the launch (a standalone effect with more than two
                             // channels runs one stereo unit per channel pair); 0 for the bus
  // Chunk grid of the main mixer (see PG_MAX_FRAMES): block 0 of the launch starts grid_off frames behind a chunk start, chunks of
  // PG_MAX_FRAMES follow each other from there until grid_span frames behind that chunk start (the end of the write call or the next
  // main-mixer event). grid_span == 0: every block is a chunk of its own (standalone effects, launches of one whole chunk).
  uint32_t grid_off, grid_span;
};
// Where block c of a launch sits in the main mixer's chunk grid.
struct PgPiece {
  bool first, last;       // first / last piece of its chunk
  int c_last;             // block (relative to the launch's block 0) that holds the chunk's last frame
  uint64_t chunk_end;     // position (frames) at which the chunk ends
};
// PgLaunch::error_word bits: conditions the host's routing must make impossible; a set bit means wrong audio, never a crash.
enum { PG_DEVERR_FAST_DECLINED = 1,   // a kernel without serial effect code met an effect state its time-parallel path does not take
       PG_DEVERR_SUPER_DEFERRED = 2,  // a unit wanted the generic kernel inside a super-block launch
       PG_DEVERR_BUS_STALLED = 4 };   // a stage of the pipelined bus chain gave up waiting for the stage in front of it
constexpr int PG_STAGE_BUF_DOUBLES = 2 * 1024 + 128 + 8;
