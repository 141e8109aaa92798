// The Sampler's note layer on the device (src/generator/sampler.rs:656-860, src/generator/sampler/voice.rs:122-310): note-on with voice
// allocation and stealing, note-off, the per-note setters, the base and the envelope parameters and stop, applied by the exact kernel (pg_unit_kernel) in its
// command loop, in front of the frame a message lands on. The workgroup that renders the sampler's sub-mixer renders all of its pool voices, so
// in front of that frame the records it reads here hold exactly what the reference's Sampler sees at the top of the `write` the owning mixer
// cut at the message's sample time: which slots are active, which envelopes are in Release, which faders run.
// Wave 0 of the workgroup calls sampler_command (all 64 lanes): allocation takes one lane per slot, everything else runs on lane 0.
#pragma once
#include "pg_source_dev.h"

namespace pgd {

DEVO PgSamplerRec* sampler_rec(const PgLaunch& L, int index) {
  if (!L.voices || !L.env || !L.env->samplers) return nullptr;
  PgSamplerTab* const tab = L.env->samplers;
  return (uint32_t)index < tab->n ? (PgSamplerRec*)(tab + 1) + index : nullptr;
}
DEVO PgEnv* sampler_env(const PgLaunch& L, const PgSamplerRec& r, int slot) {
  if (!r.has_envelope) return nullptr;
  const uint64_t v = (uint64_t)(r.voice0 + slot);
  return v < L.env->cap ? (PgEnv*)(L.env + 1) + v : nullptr;
}
// The pool as the host describes it lies inside the tables (the envelope table has an entry for every voice of the graph): anything else is left alone
DEVO bool sampler_pool_ok(const PgLaunch& L, const PgSamplerRec& r) {
  return r.n_voices >= 1 && r.n_voices <= PG_SAMPLER_MAX_VOICES && r.voice0 >= 0 && (uint64_t)r.voice0 + (uint64_t)r.n_voices <= L.env->cap;
}
// SamplerVoice::is_active (voice.rs:100-102): a note was started in the slot and no source write has ended it since (see PgSamplerRec)
DEVO bool sampler_slot_active(const PgVoice& v) { return v.active != 0 && v.finished == 0; }

// AhdsrEnvelope::note_on (ahdsr.rs:402-419)
DEVO void ahdsr_note_on(PgEnvState& st, const PgEnvParams& p, float volume) {
  st.target_volume = volume;
  if (p.attack_rate == 3.402823466e+38f) {
    st.output = volume;
    if (!(p.zero_times & PG_AHDSR_HOLD_ZERO)) { st.stage = PG_AHDSR_HOLD; st.hold_samples_remaining = p.hold_samples; }
    else st.stage = PG_AHDSR_DECAY;
  } else { st.output = 0.0f; st.stage = PG_AHDSR_ATTACK; }
}

// AhdsrParameters::set_attack_time / set_hold_time / set_decay_time / set_sustain_level / set_release_time (ahdsr.rs:143-249) as the host has
// resolved them in time order (pg_sampler.hip: sampler_stage_command): the one field the setter writes, and which of the times are zero now.
// Nothing of a running envelope's state changes: a Hold in progress keeps its hold_samples_remaining.
DEVO void ahdsr_set_param(PgEnvParams& p, const PgCmd& cmd) {
  if (cmd.param == PG_SE_ATTACK) p.attack_rate = cmd.value;
  else if (cmd.param == PG_SE_HOLD) p.hold_samples = cmd.value;
  else if (cmd.param == PG_SE_DECAY) p.decay_rate = cmd.value;
  else if (cmd.param == PG_SE_SUSTAIN) p.sustain_level = cmd.value;
  else if (cmd.param == PG_SE_RELEASE) p.release_rate = cmd.value;
  else return;
  p.zero_times = (int32_t)(cmd.value64 & (PG_AHDSR_HOLD_ZERO | PG_AHDSR_DECAY_ZERO | PG_AHDSR_RELEASE_ZERO));
}

// Sampler::next_free_voice_index (sampler.rs:826-860), one lane per slot (all lanes of the wave call; every lane gets the result):
// the first slot that is not active; else — only with an envelope — the slot in Release with the smallest release_start_frame; else the active
// slot with the smallest note id. The reference's strict `<` keeps the first of equals: ties go to the lower slot.
DEVO int sampler_alloc(const PgLaunch& L, const PgSamplerRec& r) {
  const int lane = (int)(threadIdx.x & 63);
  const bool mine = lane < r.n_voices;
  bool active = false, releasing = false;
  if (mine) {
    active = sampler_slot_active(L.voices[r.voice0 + lane]);
    const PgEnv* const e = sampler_env(L, r, lane);
    releasing = active && e != nullptr && e->state.stage == PG_AHDSR_RELEASE && r.slots[lane].release_start_frame != PG_USIZE_MAX;
  }
  const unsigned long long free_mask = __ballot(mine && !active);
  if (free_mask) return __ffsll((long long)free_mask) - 1;
  // two wave min-reductions over (key, slot): the slot breaks ties towards the lower index
  const bool any_releasing = __ballot(releasing) != 0ull;
  unsigned long long key = PG_USIZE_MAX;
  if (mine && (any_releasing ? releasing : true)) key = any_releasing ? r.slots[lane].release_start_frame : r.slots[lane].note_id;
  int slot = mine ? lane : 64;
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long ok = __shfl_xor(key, off, 64);
    const int os = __shfl_xor(slot, off, 64);
    if (ok < key || (ok == key && os < slot)) { key = ok; slot = os; }
  }
  return slot < r.n_voices ? slot : 0;
}

DEVO float sampler_clamp_pan(float p) { return fminf(fmaxf(p, -1.0f), 1.0f); }

// SamplerVoice::start (voice.rs:122-193) on lane 0. reset() (:222-236) runs PreloadedFileSource::reset only if the slot was active
// (preloaded.rs:212-230: a kill without a fade, then positions, resampler and fader as new); a slot that is not active was reset by the write
// that ended its note (voice.rs:488-495) — the same fields, so both cases write them. The two smoothers keep their current values: a reused
// slot ramps from where the previous note left them (amplified.rs:60-62, panned.rs).
DEVO void sampler_voice_start(PgVoice* v, PgEnv* e, PgSamplerSlot& s, const PgSamplerRec& r, const double* speed_tab, int note_id, int note, float volume, float panning, uint64_t now) {
  for (int c = 0; c < 2; ++c) { for (int k = 0; k < 4; ++k) v->input[c][k] = 0.0f; v->sub_pos[c] = 0.0f; v->initialized[c] = 0; }
  v->playback_pos = 0; v->repeat_count = v->repeat; v->pos_eof = 0; v->finished = 0;
  v->fader_state = 0; v->fader_current = 1.0f; v->fader_target = 1.0f; v->fader_inertia = 1.0f;
  v->has_stop = 0; v->stop_time = 0; v->chunk_skip = 0; v->zombie_end = 0;
  v->start_time = now;
  v->active = 1;
  s.note_id = (uint64_t)note_id; s.note = note; s.note_volume = volume; s.note_panning = panning; s.release_start_frame = PG_USIZE_MAX;
  voice_set_speed(v, speed_tab[note & 255] * r.pitch_factor, 0.0f);
  sm_set_target(v->volume, r.base_volume * volume);
  sm_set_target(v->panning, sampler_clamp_pan(r.base_panning + panning));
  if (e) { PgEnvState st = e->state; ahdsr_note_on(st, e->params, 1.0f); e->state = st; }
}
// SamplerVoice::stop (voice.rs:196-219) on lane 0: an active slot only; the release start moves also when the slot releases already
DEVO void sampler_voice_stop(PgVoice* v, PgEnv* e, PgSamplerSlot& s, uint64_t now) {
  if (!sampler_slot_active(*v)) return;
  s.release_start_frame = now;
  if (e) { PgEnvState st = e->state; ahdsr_note_off(st, e->params); e->state = st; }
  else { v->has_stop = 1; v->stop_time = now; }   // PreloadedFileSource::stop in front of the next source write: the 50 ms fade-out (sampler.rs:513-514)
}
// The first slot in index order that plays note `note_id` (sampler.rs:776-822), -1: none
DEVO int sampler_find(const PgLaunch& L, const PgSamplerRec& r, int note_id) {
  for (int i = 0; i < r.n_voices; ++i) if (r.slots[i].note_id == (uint64_t)note_id && sampler_slot_active(L.voices[r.voice0 + i])) return i;
  return -1;
}

// One sampler command in front of frame `now` (Sampler::process_playback_messages, sampler.rs:656-731). Called by every lane of wave 0.
DEVO void sampler_command(const PgLaunch& L, const PgCmd& cmd, uint64_t now) {
  PgSamplerRec* const rp = sampler_rec(L, cmd.target);
  if (rp == nullptr) return;
  PgSamplerRec& r = *rp;
  if (!sampler_pool_ok(L, r)) return;
  const bool lane0 = (threadIdx.x & 63) == 0;
  if (cmd.type == CMD_SAMPLER_STOP) {   // Sampler::stop (:733-738): taken also while stopping
    if (lane0) {
      r.stopping = r.transient;
      for (int i = 0; i < r.n_voices; ++i) sampler_voice_stop(&L.voices[r.voice0 + i], sampler_env(L, r, i), r.slots[i], now);
    }
    return;
  }
  if (r.stopping) return;   // every trigger is dropped while the sampler stops (:663-664)
  if (cmd.type == CMD_SAMPLER_NOTE_ON) {
    const int slot = sampler_alloc(L, r);
    if (lane0) sampler_voice_start(&L.voices[r.voice0 + slot], sampler_env(L, r, slot), r.slots[slot], r, L.env->samplers->speed_tab, cmd.param, (int)(cmd.value64 & 0xff), cmd.value,
                                   __uint_as_float((uint32_t)(cmd.value64 >> 32)), now);
    return;
  }
  if (!lane0) return;
  if (cmd.type == CMD_SAMPLER_ALL_NOTES_OFF) {
    for (int i = 0; i < r.n_voices; ++i) sampler_voice_stop(&L.voices[r.voice0 + i], sampler_env(L, r, i), r.slots[i], now);
  } else if (cmd.type == CMD_SAMPLER_ENV_PARAM) {   // set_envelope_parameter (:184-217, :1122-1131): the pool's one AhdsrParameters — here every slot's copy, playing or free
    for (int i = 0; i < r.n_voices; ++i) {
      PgEnv* const e = sampler_env(L, r, i);
      if (e) { PgEnvParams p = e->params; ahdsr_set_param(p, cmd); e->params = p; }
    }
  } else if (cmd.type == CMD_SAMPLER_PARAM) {   // process_parameter_update (:1076-1120): the stored base value, then every ACTIVE voice
    if (cmd.param == PG_SP_TRANSPOSE || cmd.param == PG_SP_FINETUNE) {
      if (cmd.param == PG_SP_TRANSPOSE) r.transpose = (int)cmd.value; else r.finetune = (int)cmd.value;
      r.pitch_factor = __longlong_as_double((long long)cmd.value64);
    } else if (cmd.param == PG_SP_VOLUME) r.base_volume = cmd.value;
    else if (cmd.param == PG_SP_PANNING) r.base_panning = cmd.value;
    for (int i = 0; i < r.n_voices; ++i) {
      PgVoice* const v = &L.voices[r.voice0 + i];
      if (!sampler_slot_active(*v)) continue;
      if (cmd.param == PG_SP_TRANSPOSE || cmd.param == PG_SP_FINETUNE) voice_set_speed(v, L.env->samplers->speed_tab[r.slots[i].note & 255] * r.pitch_factor, 0.0f);   // set_base_pitch: no glide
      else if (cmd.param == PG_SP_VOLUME) sm_set_target(v->volume, r.base_volume * r.slots[i].note_volume);
      else if (cmd.param == PG_SP_PANNING) sm_set_target(v->panning, sampler_clamp_pan(r.base_panning + r.slots[i].note_panning));
    }
  } else {
    const int i = sampler_find(L, r, cmd.param);
    if (i < 0) return;   // an unknown or ended note: ignored
    PgVoice* const v = &L.voices[r.voice0 + i];
    if (cmd.type == CMD_SAMPLER_NOTE_OFF) sampler_voice_stop(v, sampler_env(L, r, i), r.slots[i], now);
    else if (cmd.type == CMD_SAMPLER_NOTE_SPEED) voice_set_speed(v, __longlong_as_double((long long)cmd.value64) * r.pitch_factor, cmd.value);
    else if (cmd.type == CMD_SAMPLER_NOTE_VOLUME) { r.slots[i].note_volume = cmd.value; sm_set_target(v->volume, r.base_volume * cmd.value); }
    else if (cmd.type == CMD_SAMPLER_NOTE_PAN) { r.slots[i].note_panning = cmd.value; sm_set_target(v->panning, sampler_clamp_pan(r.base_panning + cmd.value)); }
  }
}

// Behind the source stage of a segment that ends a chunk of unit `u` (the end of a Sampler::write, sampler.rs:1008-1024): a sampler that was
// told to stop and has no active slot left is stopped — the host, which polls the mapped word at the top of a write, takes the pool out of the
// mixer then. Lane 0 of the workgroup.
DEVO void sampler_end_of_write(const PgLaunch& L, int u) {
  if (!L.voices || !L.env || !L.env->samplers) return;
  PgSamplerTab* const tab = L.env->samplers;
  for (uint32_t k = 0; k < tab->n; ++k) {
    PgSamplerRec& r = ((PgSamplerRec*)(tab + 1))[k];
    if (r.unit != u || !r.stopping || r.stopped || !sampler_pool_ok(L, r)) continue;
    int active = 0;
    for (int i = 0; i < r.n_voices; ++i) active += sampler_slot_active(L.voices[r.voice0 + i]) ? 1 : 0;
    if (active == 0) { r.stopped = 1; *(volatile int32_t*)(tab->stopped + k) = 1; __threadfence_system(); }
  }
}

}  // namespace pgd
