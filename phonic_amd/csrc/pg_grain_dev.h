// Granular playback of a sampler voice: GrainPool<100>, Grain and GrainWindow<2048> of the reference (src/generator/sampler/granular.rs),
// driven as SamplerVoice::process drives them (src/generator/sampler/voice.rs:406-432). The arithmetic of one frame, cut along the three
// phases of pg_grain_kernel (pg_k_grain.hip):
//   grain_sched_frame   the scheduler of one frame — try_trigger_grain (:524-603), update_trigger_phase (:788-809), activate_new_grain
//                       (:813-897) with Grain::activate (:1025-1067), advance_playhead (:607-640) — a non-associative f32 / f64 recurrence with
//                       integer decisions and the RNG draws in the reference's order: one lane walks it;
//   grain_step          Grain::process's recurrences of one slot (:1081-1120): position and window phase in f64, the loop-range and [0, 1]
//                       wraps, samples_remaining — one lane per slot walks them frame by frame (position + k * increment would round
//                       differently, and the read point is (position as f32) * (len - 1), :906);
//   grain_term          what dominates: the window lookup (:201-215), sample_at_position's four reads and Catmull-Rom (:901-933), the
//                       ENVELOPE_THRESHOLD test and the two stereo terms (:717-724) — independent per (frame, grain).
// Everything is compiled with contraction off, f32 where the reference has f32 and f64 where it has f64: each grain's per-frame terms are the
// reference's bits; only the order of the f32 sum over the grains of a frame is this implementation's (ascending slot index).
//
// The modulation matrix (pg_graph_set_voice_modulation_matrix): a voice that has one hands the frame's seven sums (GrainModFrame, formed by
// phase 0 of pg_grain_kernel) to grain_sched_frame<true>, which applies them as the reference writes them, `x + 0.0` and `x * (1.0 + 0.0)` of
// a matrix without routes included. A voice without one takes grain_sched_frame<false>: every `*_mod` argument of try_trigger_grain /
// advance_playhead is 0.0 there, and since `x + 0.0` and `x * (1.0 + 0.0)` leave every finite x as it is those operations are left out.
// The granular parameters and the loop range change while the voice plays (pg_graph_set_voice_granular_parameter / _grain_loop_range): the
// scheduler lane applies the commands to GrainSched::p in front of their frames; what a change makes live is in grain_sched_frame (the pool's own
// overlap_mode, the crossfade point of the current window) and in the activation (the grain keeps the window and loop range it was born with).
// Out of scope (include/phonic_gpu.h says so too): playback-position status events.
//
// Random draws are rand 0.9's on SmallRng = Xoshiro256++ as rand's documentation describes them (unverified against the crate's source, which
// this project does not hold): random::<f32>() = (next_u64 >> 40) * 2^-24 (rng_random_f32), random::<f64>() = (next_u64 >> 11) * 2^-53,
// random::<bool>() = the top bit of next_u64.
#pragma once
#include "pg_dsp_dev.h"

namespace pgd {

#define PG_GRAIN_TILE 32              // frames per tile of pg_grain_kernel (its LDS: 12 bytes per slot and frame)
#define PG_GRAIN_INACTIVE 0xffffffffu // phase 2's marker: the slot holds no active grain at this frame
constexpr float GRAIN_ENVELOPE_THRESHOLD = 0.001f;   // GrainPool::ENVELOPE_THRESHOLD (granular.rs:381)

DEV double grain_random_f64(uint64_t* s) { return (double)(xoshiro256pp_next(s) >> 11) * (1.0 / 9007199254740992.0); }
DEV bool grain_random_bool(uint64_t* s) { return (xoshiro256pp_next(s) >> 63) != 0; }

// 2.0_f64.powf(a) for the pitch variation's |a| <= 1/16 (half a semitone is 1/24 of an octave): exp(a ln 2) as a double-double Taylor sum whose
// error in front of the one final rounding is below 2^-68 — the correctly rounded result but for one argument in some 2^15. (The device's
// own pow is good to an ulp or two, a libm's to ~0.5 ulp: neither is a bit-exact definition. tests/granular_model.py uses decimal arithmetic.)
DEV double grain_pow2_small(double a) {
  if (a == 0.0) return 1.0;
  const double LN2_H = 0x1.62e42fefa39efp-1, LN2_L = 0x1.abc9e3b39803fp-56;
  double th = a * LN2_H;
  double tl = fma(a, LN2_H, -th) + a * LN2_L;
  { const double s = th + tl; tl = tl - (s - th); th = s; }
  const double qh = th * th;                                   // t^2 = qh + ql
  const double ql = fma(th, th, -qh) + 2.0 * th * tl;
  double p = 1.0 / 39916800.0;                                 // t^3/3! + ... + t^11/11!: plain f64 (t^3/6 < 5e-6, its rounding error < 2^-69)
  p = p * th + 1.0 / 3628800.0;
  p = p * th + 1.0 / 362880.0;
  p = p * th + 1.0 / 40320.0;
  p = p * th + 1.0 / 5040.0;
  p = p * th + 1.0 / 720.0;
  p = p * th + 1.0 / 120.0;
  p = p * th + 1.0 / 24.0;
  p = p * th + 1.0 / 6.0;
  const double tail = th * th * th * p;
  const double lo = tl + (0.5 * ql + tail);
  const double mid = 0.5 * qh;
  const double a1 = 1.0 + th, b1 = th - (a1 - 1.0);            // fast two-sum: 1 > |th|
  const double a2 = a1 + mid, b2 = mid - (a2 - a1);            // a1 > mid
  return a2 + ((b1 + b2) + lo);
}

DEV double grain_rem_euclid(double a, double b) {  // f64::rem_euclid: fmod is exact
  const double r = fmod(a, b);
  return r < 0.0 ? r + fabs(b) : r;
}
DEV double grain_fold_into_loop_range(double position, double loop_start, double loop_end) {  // granular.rs:433-440
  const double loop_len = loop_end - loop_start;
  return loop_len > 0.0 ? loop_start + grain_rem_euclid(position - loop_start, loop_len) : loop_start;
}
DEV float grain_crossfade_point(int window) { return window <= 3 ? 0.5f : (window == 4 ? 0.9f : 0.8f); }  // sequential_crossfade_point (:78-94)

// What the scheduler lane needs of one voice beyond the pool: the constants, and the frame at which every slot stops being active
// (`end[s]`, relative to the tile: the slot is inactive at frame f iff end[s] <= f — samples_remaining only counts down, so the slot lanes
// need not run ahead of the scheduler).
struct GrainSched {
  PgGrainParams p;
  PgGrainPool pool;
  uint64_t n_frames;      // sample_buffer.len()
  uint32_t sample_rate;
  // Sequential mode: the primary grain's window phase, walked with the slot lane's own operations (Grain::process: window_phase += window_increment)
  double prim_phase, prim_inc;
};

// Grain::activate's result for one slot, handed from the scheduler lane to the slot's lane.
struct GrainActivation {
  double position, increment, window_increment, loop_start, loop_end;
  uint64_t samples_remaining;
  float volume, panning;
  int32_t slot;           // -1: no activation at this frame
  int16_t has_loop;
  int16_t window;         // parameters.window as the grain is activated (:823): the grain's own for its whole life
};

// The seven sums of the matrix for one frame, in the targets' order (SamplerVoiceModulationState::output, sampler/modulation.rs:237-247).
// `p` points at the frame's GRAIN_SIZE sum, the other targets follow PG_GRAIN_TILE floats apart (pg_grain_kernel's s_mod[target][frame]); each is
// read where the reference uses it.
struct GrainModFrame {
  const float* p;
  DEV float size() const { return p[0]; }
  DEV float density() const { return p[PG_GRAIN_TILE]; }
  DEV float variation() const { return p[2 * PG_GRAIN_TILE]; }
  DEV float spray() const { return p[3 * PG_GRAIN_TILE]; }
  DEV float pan_spread() const { return p[4 * PG_GRAIN_TILE]; }
  DEV float position() const { return p[5 * PG_GRAIN_TILE]; }
  DEV float speed() const { return p[6 * PG_GRAIN_TILE]; }
};

// One LFO frame with all seven shapes: Lfo::process (lfo.rs:172-231) with advance_phase / advance_phase_random (:233-252).
DEV float mod_lfo_run(PgModLfo& m) {
  PgLfo l = {m.phase, m.phase_inc, m.waveform};
  float v;
  if (m.waveform < 5) v = lfo_run(l);
  else {
    if (m.waveform == 5) v = m.sample_hold;
    else {
      const float p = 1.57079632679489661923f - l.phase * F32_PI;   // FRAC_PI_2 - phase * PI
      const float t = (1.0f - sine_approx(p)) * 0.5f;
      v = m.jitter_current + t * (m.jitter_target - m.jitter_current);
    }
    l.phase += l.phase_inc;
    if (l.phase >= 1.0f) {
      l.phase -= 1.0f;
      m.sample_hold = lfo_random_bipolar(m.rng);
      m.jitter_current = m.jitter_target;
      m.jitter_target = lfo_random_bipolar(m.rng);
    }
  }
  m.phase = l.phase;
  return v;
}
// Lfo::reset (lfo.rs:89-99): the phase restarts; the random shapes draw again
DEV void mod_lfo_reset(PgModLfo& m) {
  m.phase = 0.0f;
  if (m.waveform >= 5) {
    m.sample_hold = lfo_random_bipolar(m.rng);
    m.jitter_current = m.jitter_target;
    m.jitter_target = lfo_random_bipolar(m.rng);
  }
}
// Sampler::set_granular_parameter (sampler.rs:299-360): the host has resolved the update to a raw value inside the descriptor's range
DEVO void grain_set_parameter(PgGrainParams& p, uint32_t index, float value) {
  switch (index) {
    case PG_GP_OVERLAP_MODE: p.overlap_mode = (int32_t)value & 1; break;
    case PG_GP_WINDOW: p.window = (int32_t)value & (PG_GRAIN_WINDOWS - 1); break;
    case PG_GP_SIZE: p.size = value; break;
    case PG_GP_DENSITY: p.density = value; break;
    case PG_GP_VARIATION: p.variation = value; break;
    case PG_GP_SPRAY: p.spray = value; break;
    case PG_GP_PAN_SPREAD: p.pan_spread = value; break;
    case PG_GP_DIRECTION: { const int32_t d = (int32_t)value; p.direction = d < 0 ? 0 : (d > 2 ? 2 : d); } break;
    case PG_GP_POSITION: p.position = value; break;
    case PG_GP_STEP: p.step = value; break;
    default: break;
  }
}
// What a matrix or loop-range command does, for a lone voice (CMD_VOICE_*, pg_grain_kernel) and for every slot of a granular sampler
// (CMD_SAMPLER_*, pg_gsampler_kernel) alike: the two kinds carry the same words.
// A route command's source and target, -1 when either is out of range (the host checks them: nothing out of range indexes the table)
DEVO int grain_route_source(const PgCmd& c) { const uint32_t s = (uint32_t)(c.value64 & 0xff); return s < PG_GMOD_SOURCES ? (int)s : -1; }
DEVO int grain_route_target(const PgCmd& c) { const uint32_t t = (uint32_t)((c.value64 >> 8) & 0xff); return t < PG_GMOD_TARGETS ? (int)t : -1; }
// ModulationMatrixSlot::update_target (matrix.rs:60-83): the host has turned an amount below the threshold into 0.0, which removes the route
DEVO void grain_route_apply(const PgCmd& c, float (*amount)[PG_GMOD_TARGETS], int32_t (*bipolar)[PG_GMOD_TARGETS]) {
  const int sr = grain_route_source(c), tg = grain_route_target(c);
  if (sr >= 0 && tg >= 0) { amount[sr][tg] = c.value; bipolar[sr][tg] = c.value != 0.0f && ((c.value64 >> 16) & 1) ? 1 : 0; }
}
// Lfo::set_rate / set_waveform (lfo.rs:102-119) of LFO `l`, if the command is that LFO's: nothing else of the LFO changes
DEVO void grain_lfo_apply(const PgCmd& c, bool is_rate, int l, PgModLfo& m) {
  if ((int)(c.value64 & 0xff) != l) return;
  if (is_rate) m.phase_inc = c.value;
  else { const uint32_t w = (uint32_t)((c.value64 >> 8) & 0xff); if (w < 7) m.waveform = (int32_t)w; }
}
// GrainPool::set_loop_range (granular.rs:516-518): playing_loop_range, the playhead and living grains keep what they have
DEVO void grain_loop_apply(const PgCmd& c, PgGrainParams& p) {
  p.has_loop = (int32_t)(c.value64 & 1); p.loop_start = c.value; p.loop_end = __uint_as_float((uint32_t)(c.value64 >> 32));
}
// One slot's contribution to a target's sum (ModulationMatrix::output, matrix.rs:201-231): LFOs are bipolar sources, velocity and keytracking
// unipolar ones.
DEV float mod_bipolar_source(float v, int bipolar) { return bipolar ? v : (v + 1.0f) / 2.0f; }
DEV float mod_unipolar_source(float v, int bipolar) { return bipolar ? (v - 0.5f) * 2.0f : v; }

template <bool MOD>
DEV float grain_playback_position(const GrainSched& S, float position_mod) {  // granular.rs:446-472
  float base = S.p.step == 0.0f ? S.p.position : S.pool.playhead;
  if (MOD) { if (position_mod != 0.0f) base += position_mod; }
  if (S.pool.playing_loop_range && S.p.has_loop) base = (float)grain_fold_into_loop_range((double)base, (double)S.p.loop_start, (double)S.p.loop_end);
  const float r = fmodf(base, 1.0f);   // f32::rem_euclid(1.0)
  return r < 0.0f ? r + 1.0f : r;
}

// One frame of the scheduler, in front of the frame's grains: try_trigger_grain, then advance_playhead when step != 0 (granular.rs:693-711).
// `end`: see GrainSched. Returns the activation (slot == -1: none).
// MOD: the voice has a modulation matrix and `m` holds the frame's sums; without one `m` is not looked at.
template <bool MOD, typename EndArray>
DEV void grain_sched_frame(GrainSched& S, EndArray end, int f, GrainActivation& act, const GrainModFrame& m) {
  act.slot = -1;
  PgGrainPool& P = S.pool;
  const PgGrainParams& p = S.p;
  if (P.overlap_mode != p.overlap_mode) { P.overlap_mode = p.overlap_mode; P.primary = -1; }   // detect mode changes (:535-538)
  const bool sequential = P.overlap_mode == 1;   // (the pool's copy: :541, :794, :596)
  bool trigger = true;
  if (sequential && P.primary >= 0 && end[P.primary] > f) {
    if (S.prim_phase < (double)grain_crossfade_point(p.window)) trigger = false;   // block the new grain until the primary reaches its crossfade point
  }
  if (trigger && !P.trigger_new_grains) trigger = false;
  if (trigger && !sequential) {  // update_trigger_phase
    float density = MOD ? p.density * (1.0f + m.density()) : p.density;
    density = density < 1.0f ? 1.0f : (density > 100.0f ? 100.0f : density);
    P.trigger_phase += density / (float)S.sample_rate;
    if (P.trigger_phase >= 1.0f) P.trigger_phase -= 1.0f; else trigger = false;
  }
  if (trigger) {
    // spray: +/- 1 s at 1.0 (:562-571) — drawn whether or not a slot is free
    const double file_duration = (double)S.n_frames / (double)S.sample_rate;
    float spray = MOD ? p.spray + m.spray() : p.spray;
    spray = spray < 0.0f ? 0.0f : (spray > 1.0f ? 1.0f : spray);
    const double spray_seconds = (double)spray * 2.0 * (grain_random_f64(P.rng) - 0.5);
    const double spray_variation = spray_seconds / file_duration;
    double grain_position = (double)grain_playback_position<MOD>(S, MOD ? m.position() : 0.0f) + spray_variation;
    if (P.playing_loop_range && p.has_loop) grain_position = grain_fold_into_loop_range(grain_position, (double)p.loop_start, (double)p.loop_end);
    grain_position = grain_rem_euclid(grain_position, 1.0);
    // activate_new_grain: the first inactive slot (:821)
    int index = -1;
    for (int s = 0; s < PG_GRAIN_POOL; ++s) if (end[s] <= f) { index = s; break; }
    if (index >= 0) {
      float variation = MOD ? p.variation + m.variation() : p.variation;
      variation = variation < 0.0f ? 0.0f : (variation > 1.0f ? 1.0f : variation);
      const float volume_scale = 1.0f - (variation * rng_random_f32(P.rng));
      const float volume = P.volume * volume_scale;
      const double random_semitones = (double)variation * (grain_random_f64(P.rng) - 0.5);
      const double speed = random_semitones != 0.0 ? P.speed * grain_pow2_small(random_semitones / 12.0) : P.speed;
      const float min_scale = 1.0f - (0.75f * variation);
      const float max_scale = 1.0f + (2.0f * variation);
      const float size_scale = min_scale + (max_scale - min_scale) * rng_random_f32(P.rng);
      float grain_size_ms = MOD ? p.size * (1.0f + m.size()) : p.size;
      grain_size_ms = grain_size_ms < 1.0f ? 1.0f : (grain_size_ms > 1000.0f ? 1000.0f : grain_size_ms);
      const float size_f = grain_size_ms * size_scale * (float)S.sample_rate / 1000.0f;
      uint64_t grain_size = size_f > 0.0f ? (uint64_t)size_f : 0;   // `as usize` saturates
      if (grain_size < 2) grain_size = 2;
      float pan_spread = MOD ? p.pan_spread + m.pan_spread() : p.pan_spread;
      pan_spread = pan_spread < 0.0f ? 0.0f : (pan_spread > 1.0f ? 1.0f : pan_spread);
      const float panning_spread = pan_spread * (rng_random_f32(P.rng) * 2.0f - 1.0f);
      float panning = P.panning + panning_spread;
      panning = panning < -1.0f ? -1.0f : (panning > 1.0f ? 1.0f : panning);
      const float pitch_variation_semitones = variation * (rng_random_f32(P.rng) * 2.0f - 1.0f) * 0.5f;
      const double varied_speed = speed * grain_pow2_small((double)pitch_variation_semitones / 12.0);
      const bool reverse = p.direction == 0 ? false : (p.direction == 1 ? true : grain_random_bool(P.rng));
      // Grain::activate (:1025-1067)
      act.slot = index;
      act.position = grain_position < 0.0 ? 0.0 : (grain_position > 1.0 ? 1.0 : grain_position);
      act.volume = volume < 0.0f ? 0.0f : (volume > 100.0f ? 100.0f : volume);
      act.panning = panning;
      act.samples_remaining = grain_size;
      const bool has_loop = P.playing_loop_range && p.has_loop;
      act.has_loop = has_loop ? 1 : 0;
      act.window = (int16_t)(p.window & (PG_GRAIN_WINDOWS - 1));
      act.loop_start = has_loop ? (double)p.loop_start : 0.0;
      act.loop_end = has_loop ? (double)p.loop_end : 0.0;
      act.increment = (varied_speed / (double)S.n_frames) * (reverse ? -1.0 : 1.0);
      act.window_increment = 1.0 / (double)grain_size;
      end[index] = f + (int)(grain_size < 0x3fffffffull ? grain_size : 0x3fffffffull);
      if (sequential) { P.primary = index; S.prim_phase = 0.0; S.prim_inc = act.window_increment; }
    }
  }
  if (p.step != 0.0f) {  // advance_playhead (:607-640)
    const float modulated_step = MOD ? p.step * (1.0f + m.speed()) : p.step;
    P.playhead += modulated_step / (float)S.n_frames;
    if (p.has_loop) {
      if (P.playing_loop_range) P.playhead = (float)grain_fold_into_loop_range((double)P.playhead, (double)p.loop_start, (double)p.loop_end);
      else if (P.playhead >= p.loop_start && P.playhead < p.loop_end) P.playing_loop_range = 1;
      else if (P.playhead >= 1.0f) P.playhead -= 1.0f;
      else if (P.playhead < 0.0f) P.playhead += 1.0f;
    } else if (P.playhead >= 1.0f) P.playhead -= 1.0f;
    else if (P.playhead < 0.0f) P.playhead += 1.0f;
  }
  // the primary grain's Grain::process of this frame
  if (sequential && P.primary >= 0 && end[P.primary] > f) S.prim_phase += S.prim_inc;
}

DEV void grain_take_activation(PgGrain& g, const GrainActivation& a) {
  g.active = 1; g.window_mode = a.window;
  g.position = a.position; g.volume = a.volume; g.panning = a.panning;
  g.samples_remaining = a.samples_remaining;
  g.has_loop = a.has_loop; g.loop_start = a.loop_start; g.loop_end = a.loop_end;
  g.increment = a.increment;
  g.window_phase = 0.0; g.window_increment = a.window_increment;
}

// Grain::process without its table lookups (:1081-1120): the position to read at, the window table's index and fraction (GrainWindow::sample's
// f64 part, :204-206), then the step.
DEV void grain_step(PgGrain& g, float& position, uint32_t& index, float& fraction) {
  const double index_float = g.window_phase * (double)(PG_GRAIN_LUT_N - 1);
  index = (uint32_t)((uint64_t)index_float & (uint64_t)(PG_GRAIN_LUT_N - 1));
  fraction = (float)(index_float - trunc(index_float));
  position = (float)g.position;
  g.position += g.increment;
  g.window_phase += g.window_increment;
  g.samples_remaining = g.samples_remaining ? g.samples_remaining - 1 : 0;
  if (g.has_loop) {
    const double loop_len = g.loop_end - g.loop_start;
    if (loop_len > 0.0) g.position = g.loop_start + grain_rem_euclid(g.position - g.loop_start, loop_len);
  } else if (g.position < 0.0) g.position += 1.0;
  else if (g.position > 1.0) g.position -= 1.0;
  if (g.samples_remaining == 0) g.active = 0;
}

// GrainWindow::sample's f32 part (:207-215): `lut` is the row of the grain's window_mode.
template <typename Lut>
DEV float grain_window_value(Lut lut, uint32_t index, float fraction) {
  const uint32_t next_index = (index + 1) & (PG_GRAIN_LUT_N - 1);
  return index < PG_GRAIN_LUT_N - 1 ? lut[index] * (1.0f - fraction) + lut[next_index] * fraction : lut[PG_GRAIN_LUT_N - 1];
}
// The two stereo terms of one grain at one frame (granular.rs:717-724): `envelope_value` is the grain's window at the frame, `pcm` the voice's buffer
// of `len` >= 1 frames.
DEV void grain_term(float envelope_value, const float* pcm, uint64_t len, float position, float volume, float panning, float& left, float& right) {
  left = 0.0f; right = 0.0f;
  const float envelope = envelope_value * volume;
  if (!(envelope > GRAIN_ENVELOPE_THRESHOLD)) return;
  // sample_at_position (:901-933)
  const uint64_t max_index = len - 1;
  const float float_index = position * (float)max_index;
  uint64_t i1 = float_index > 0.0f ? (uint64_t)float_index : 0;   // `as usize` saturates
  if (i1 > max_index) i1 = max_index;
  const float fr = float_index - (float)i1;
  const uint64_t i2 = i1 < max_index ? i1 + 1 : 0;
  const uint64_t i0 = i1 > 0 ? i1 - 1 : max_index;
  const uint64_t i3 = i2 < max_index ? i2 + 1 : 0;
  const float y0 = pcm[i0], y1 = pcm[i1], y2 = pcm[i2], y3 = pcm[i3];
  const float a = -0.5f * y0 + 1.5f * y1 - 1.5f * y2 + 0.5f * y3;
  const float b = y0 - 2.5f * y1 + 2.0f * y2 - 0.5f * y3;
  const float c = -0.5f * y0 + 0.5f * y2;
  const float sample = a * fr * fr * fr + b * fr * fr + c * fr + y1;
  const float windowed_sample = sample * envelope;
  left = windowed_sample * ((1.0f - panning) * 0.5f);
  right = windowed_sample * ((1.0f + panning) * 0.5f);
}

// GrainWindow::new (granular.rs:112-196) for entry i of the eight tables, with the reference's f32 expressions; cos / exp are evaluated in
// f64 and rounded once — the correctly rounded f32 value. Host only (the table is built once per graph and uploaded).
inline void grain_window_entry(int i, float out[PG_GRAIN_WINDOWS]) {
  auto cosf_cr = [](float x) { return (float)cos((double)x); };
  const float PI = 3.14159265358979323846f;
  const float phase = (float)i / (float)PG_GRAIN_LUT_N;
  out[0] = 0.5f * (1.0f - cosf_cr(2.0f * PI * phase));
  const float pi_phase = PI * phase;
  out[1] = 0.42f - 0.5f * cosf_cr(2.0f * pi_phase) + 0.08f * cosf_cr(4.0f * pi_phase);
  out[2] = phase < 0.5f ? 2.0f * phase : 2.0f * (1.0f - phase);
  const float width = 0.5f / 2.0f;
  if (phase < width) out[3] = 0.5f * (1.0f - cosf_cr(PI * (phase / width)));
  else if (phase > 1.0f - width) out[3] = 0.5f * (1.0f - cosf_cr(PI * ((1.0f - phase) / width)));
  else out[3] = 1.0f;
  const float ramp_width = 0.1f;
  if (phase < ramp_width) out[4] = phase / ramp_width;
  else if (phase > 1.0f - ramp_width) out[4] = (1.0f - phase) / ramp_width;
  else out[4] = 1.0f;
  out[5] = (float)exp((double)(-6.0f * fabsf(phase - 0.5f)));
  if (phase < 0.9f) out[6] = phase / 0.9f;
  else out[6] = 0.5f * (1.0f + cosf_cr(PI * ((phase - 0.9f) / 0.1f)));
  if (phase < 0.1f) out[7] = 0.5f * (1.0f - cosf_cr(PI * (phase / 0.1f)));
  else out[7] = 1.0f - ((phase - 0.1f) / 0.9f);
}

}  // namespace pgd
