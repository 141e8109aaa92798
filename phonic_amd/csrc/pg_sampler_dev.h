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
// that were told to stop. Lane 0 of the workgroup.
DEVO void sampler_end_of_write(const PgLaunch& L, int u) {
  if (!L.voices || !L.env || !L.env->samplers) return;
  PgSamplerTab* const tab = L.env->samplers;
  for (uint32_t k = 0; k < tab->n; ++k) {
    PgSamplerRec& r = ((PgSamplerRec*)(tab + 1))[k];
    if (r.unit != u || !r.stopping || r.stopped || !sampler_pool_ok(L, r)) continue;
    note_end_of_write(FilePool{L, r}, tab->stopped + k);
  }
}

}  // namespace pgd
