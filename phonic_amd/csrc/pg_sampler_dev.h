// A file sampler's pool under the Sampler's note layer (pg_note_dev.h; src/generator/sampler.rs:656-860, src/generator/sampler/voice.rs:122-310):
// the pool's adapter, note-on with its voice's reset, and the entry points the exact kernel (pg_unit_kernel) calls in its command loop, in front of
// the frame a message lands on, and behind a chunk's last source stage. The workgroup that renders the sampler's sub-mixer renders all of its pool voices, so
// in front of that frame the records it reads here hold exactly what the reference's Sampler sees at the top of the `write` the owning mixer
// cut at the message's sample time: which slots are active, which envelopes are in Release, which faders run.
// Wave 0 of the workgroup calls sampler_command (all 64 lanes): allocation takes one lane per slot, everything else runs on lane 0.
#pragma once
#include "pg_note_dev.h"

namespace pgd {

DEVO PgSamplerRec* sampler_rec(const PgLaunch& L, int index) {
  if (!L.voices || !L.env || !L.env->samplers) return nullptr;
  PgSamplerTab* const tab = L.env->samplers;
  return (uint32_t)index < tab->n ? (PgSamplerRec*)(tab + 1) + index : nullptr;
}
// The pool as the host describes it lies inside the tables (the envelope table has an entry for every voice of the graph): anything else is left alone
DEVO bool sampler_pool_ok(const PgLaunch& L, const PgSamplerRec& r) {
  return r.n_voices >= 1 && r.n_voices <= PG_SAMPLER_MAX_VOICES && r.voice0 >= 0 && (uint64_t)r.voice0 + (uint64_t)r.n_voices <= L.env->cap;
}
// SamplerVoice::is_active (voice.rs:100-102): a note was started in the slot and no source write has ended it since (see PgSamplerRec)
DEVO bool sampler_slot_active(const PgVoice& v) { return v.active != 0 && v.finished == 0; }

// The note layer's view of the pool (pg_note_dev.h): slot i is PgVoice voice0 + i, with the PgEnv of the same index when the sampler has an envelope
struct FilePool {
  const PgLaunch& L;
  PgSamplerRec& r;
  DEVO PgSamplerRec& rec() const { return r; }
  DEVO PgVoice* voice(int i) const { return &L.voices[r.voice0 + i]; }
  DEVO PgEnv* env(int i) const { return r.has_envelope && (uint64_t)(r.voice0 + i) < L.env->cap ? (PgEnv*)(L.env + 1) + (r.voice0 + i) : nullptr; }
  DEVO bool active(int i) const { return sampler_slot_active(*voice(i)); }
  DEVO bool releasing(int i) const { const PgEnv* const e = env(i); return e != nullptr && e->state.stage == PG_AHDSR_RELEASE; }
  // SamplerVoice::stop (voice.rs:196-219): an active slot only; the release start moves also when the slot releases already
  DEVO void stop(int i, uint64_t now) const {
    PgVoice* const v = voice(i);
    if (!sampler_slot_active(*v)) return;
    r.slots[i].release_start_frame = now;
    PgEnv* const e = env(i);
    if (e) { PgEnvState st = e->state; ahdsr_note_off(st, e->params); e->state = st; }
    else { v->has_stop = 1; v->stop_time = now; }   // PreloadedFileSource::stop in front of the next source write: the 50 ms fade-out (sampler.rs:513-514)
  }
  DEVO void set_speed(int i, double speed, float glide) const { voice_set_speed(voice(i), speed, glide); }
  DEVO void set_volume(int i, float v) const { sm_set_target(voice(i)->volume, v); }
  DEVO void set_panning(int i, float p) const { sm_set_target(voice(i)->panning, p); }
  DEVO void env_param(const PgCmd& cmd) const {   // here every slot's copy of the parameters, playing or free
    for (int i = 0; i < r.n_voices; ++i) {
      PgEnv* const e = env(i);
      if (e) { PgEnvParams p = e->params; ahdsr_set_param(p, cmd); e->params = p; }
    }
  }
  DEVO double note_speed(int note) const { return L.env->samplers->speed_tab[note & 255]; }
};

// SamplerVoice::start (voice.rs:122-193) on lane 0. reset() (:222-236) runs PreloadedFileSource::reset only if the slot was active
// (preloaded.rs:212-230: a kill without a fade, then positions, resampler and fader as new); a slot that is not active was reset by the write
// that ended its note (voice.rs:488-495) — the same fields, so both cases write them. The two smoothers keep their current values: a reused
// slot ramps from where the previous note left them (amplified.rs:60-62, panned.rs).
DEVO void sampler_voice_start(const FilePool& pool, int slot, const PgCmd& cmd, uint64_t now) {
  PgVoice* const v = pool.voice(slot);
  for (int c = 0; c < 2; ++c) { for (int k = 0; k < 4; ++k) v->input[c][k] = 0.0f; v->sub_pos[c] = 0.0f; v->initialized[c] = 0; }
  v->playback_pos = 0; v->repeat_count = v->repeat; v->pos_eof = 0; v->finished = 0;
  v->fader_state = 0; v->fader_current = 1.0f; v->fader_target = 1.0f; v->fader_inertia = 1.0f;
  v->has_stop = 0; v->stop_time = 0; v->chunk_skip = 0; v->zombie_end = 0;
  v->start_time = now;
  v->active = 1;
  note_slot_start(pool, slot, cmd);
  PgEnv* const e = pool.env(slot);
  if (e) { PgEnvState st = e->state; ahdsr_note_on(st, e->params, 1.0f); e->state = st; }
}

// One sampler command in front of frame `now` (Sampler::process_playback_messages, sampler.rs:656-731). Called by every lane of wave 0.
DEVO void sampler_command(const PgLaunch& L, const PgCmd& cmd, uint64_t now) {
  PgSamplerRec* const rp = sampler_rec(L, cmd.target);
  if (rp == nullptr || !sampler_pool_ok(L, *rp)) return;
  const FilePool pool{L, *rp};
  const bool lane0 = (threadIdx.x & 63) == 0;
  if (note_dropped(*rp, cmd)) return;
  if (cmd.type == CMD_SAMPLER_NOTE_ON) {
    const int slot = note_alloc(pool);
    if (lane0) sampler_voice_start(pool, slot, cmd, now);
  } else if (lane0) note_message(pool, cmd, now);
}

// Behind the source stage of a segment that ends a chunk of unit `u`: the end of a Sampler::write (note_end_of_write) for the unit's samplers
// that were told to stop — a sub-mixer's (`only` < 0: every record of the table that names the unit) or the one sampler `only` whose pool a source
// unit of the main mixer holds. Lane 0 of the workgroup.
DEVO void sampler_end_of_write(const PgLaunch& L, int u, int only = -1) {
  if (!L.voices || !L.env || !L.env->samplers) return;
  PgSamplerTab* const tab = L.env->samplers;
  const uint32_t k0 = only < 0 ? 0u : (uint32_t)only, k1 = only < 0 ? tab->n : ((uint32_t)only < tab->n ? (uint32_t)only + 1u : 0u);
  for (uint32_t k = k0; k < k1; ++k) {
    PgSamplerRec& r = ((PgSamplerRec*)(tab + 1))[k];
    if (r.unit != u || !r.stopping || r.stopped || !sampler_pool_ok(L, r)) continue;
    note_end_of_write(FilePool{L, r}, tab->stopped + k);
  }
}

// ---- the generator's output stage of a main-mixer sampler: AmplifiedSource(options.volume) -> PannedSource(options.panning) over the Sampler's
// sum (player.rs:1048-1133; amplified.rs:93-104, panned.rs:93-104; apply_smoothed_gain / _panning, smoothing.rs:59-125). The smoothers and the pan law
// are the voices' own (pg_dsp_dev.h: sm_set_target, sm_need_ramp, sm_sequence, panning_factors); here: what a Sampler::write decides once, and the
// walk over a piece of its buffer. ----
// The record of sampler `index` if it is a source of the main mixer
DEVO PgGenOut* genout_rec(const PgLaunch& L, int index) {
  PgSamplerRec* const rp = sampler_rec(L, index);
  return (rp != nullptr && rp->out.on) ? &rp->out : nullptr;
}
// A SetSourceVolume / SetSourcePanning event in front of its frame: the wrapper's process_messages at the top of its write, whatever the Sampler
// then returns (amplified.rs:64-73). One lane.
DEVO void genout_command(const PgLaunch& L, const PgCmd& cmd) {
  PgGenOut* const o = genout_rec(L, cmd.target);
  if (o == nullptr) return;
  PgSmooth s = cmd.type == CMD_SAMPLER_OUT_VOLUME ? o->volume : o->panning;
  sm_set_target(s, cmd.value);
  if (cmd.type == CMD_SAMPLER_OUT_VOLUME) o->volume = s; else o->panning = s;
}
// The top of a Sampler::write, the messages of its first frame applied: does it return its buffer (sampler.rs:974-981: not stopped, and a slot is
// active or the sampler is stopping), and do the two smoothers ramp over it — need_ramp() is asked ONCE per write (smoothing.rs:60, :80), and a
// write of the main mixer's chunk is rendered as several pieces. Called by all 64 lanes of wave 0 in front of the source stage of the chunk's
// first piece: the pieces behind it, and every lane of this one behind a barrier, read the decision from the record.
// A file pool: one lane per slot asks its voice. A granular pool: pg_gsampler_kernel left the answer at the boundary that opened the write.
DEVO void genout_begin_write(const PgLaunch& L, int index) {
  PgSamplerRec* const rp = sampler_rec(L, index);
  if (rp == nullptr || !rp->out.on) return;
  const int lane = (int)(threadIdx.x & 63);
  int delivers = 0;
  if (sampler_pool_ok(L, *rp)) {
    const bool active = lane < rp->n_voices && sampler_slot_active(L.voices[rp->voice0 + lane]);
    delivers = (!rp->stopped && (__ballot(active) != 0ull || rp->stopping)) ? 1 : 0;
  } else if (rp->n_voices == 0 && rp->unit == -1 && L.env->samplers->gsamp != nullptr) delivers = L.env->samplers->gsamp[index].delivers != 0 ? 1 : 0;   // (a granular sampler's inert record: its own record of that index exists)
  if (lane == 0)
    rp->out.flags = !delivers ? 0 : (PG_GENOUT_DELIVERS | (sm_need_ramp(rp->out.volume) ? PG_GENOUT_VOLUME_RAMPS : 0) | (sm_need_ramp(rp->out.panning) ? PG_GENOUT_PAN_RAMPS : 0));
}
// `frames` stereo frames of the write's buffer at `buf` (LDS), by every lane of the workgroup; `seq`: room for 2 * frames floats (LDS). Which branch
// runs was decided by genout_begin_write, in front of at least one barrier: no lane reads a smoother here that lane 0 rewrites in the same branch
// (ADVICE.md on voice_write: a wave that evaluates need_ramp behind lane 0's store takes the other branch and misses the barriers).
// While a smoother ramps one lane lays out its value sequence and all lanes apply it, like voice_write; behind the ramp's end sm_sequence hands
// out the target, which is what next() returns to the reference's loop for the rest of the write.
DEVO void genout_apply(PgGenOut& o, float* buf, int frames, float* seq) {
  const int tid = pg_tid(), nt = blockDim.x, written = 2 * frames;
  const int flags = o.flags;
  if (!(flags & PG_GENOUT_DELIVERS)) return;   // the smoothers stand still over a write that returned 0
  if (flags & PG_GENOUT_VOLUME_RAMPS) {   // one next() per interleaved sample
    if (tid == 0) { PgSmooth s = o.volume; sm_sequence(s, seq, written); o.volume = s; }
    __syncthreads();
    for (int i = tid; i < written; i += nt) buf[i] *= seq[i];
  } else {
    const float gain = o.volume.target;
    if (fabsf(1.0f - gain) > 0.000001f) for (int i = tid; i < written; i += nt) buf[i] = buf[i] * gain;
  }
  __syncthreads();
  if (flags & PG_GENOUT_PAN_RAMPS) {   // one next() per frame
    if (tid == 0) { PgSmooth s = o.panning; sm_sequence(s, seq, frames); o.panning = s; }
    __syncthreads();
    for (int f = tid; f < frames; f += nt) { float l, r; panning_factors(seq[f], l, r); buf[2 * f] *= l; buf[2 * f + 1] *= r; }
  } else {
    const float pan = o.panning.target;
    if (fabsf(pan) > 0.000001f) {
      float l, r;
      panning_factors(pan, l, r);
      for (int i = tid; i < written; i += nt) buf[i] *= (i & 1) ? r : l;
    }
  }
  __syncthreads();
}

}  // namespace pgd
