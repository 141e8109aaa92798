// The Sampler's note layer (src/generator/sampler.rs:656-860, :1008-1024, :1076-1131), written once for both kinds of pool: which slot a note gets,
// what every message but a note-on does, what a slot holds of its note, and when a stopping sampler is stopped. What differs between a pool of file
// voices and a pool of grain pools stands behind a small adapter `Pool` (pg_sampler_dev.h: FilePool, pg_gsampler_dev.h: GrainPools):
//   rec()                      the pool's PgSamplerRec;            note_speed(note)   speed_from_note(note)
//   active(i), stop(i, now)    SamplerVoice::is_active / ::stop of slot i (stop: an active slot only);   releasing(i)   its envelope is in Release
//   set_speed(i, speed, glide), set_volume(i, v), set_panning(i, p)   where the three values of slot i's voice land
//   env_param(cmd)             a CMD_SAMPLER_ENV_PARAM on the pool's AhdsrParameters
// Nothing here holds state or takes a barrier; every function but note_alloc runs on one lane.
#pragma once
#include "pg_source_dev.h"

namespace pgd {

DEVO float sampler_clamp_pan(float p) { return fminf(fmaxf(p, -1.0f), 1.0f); }

// Every message but the stop is dropped while the sampler stops (sampler.rs:663-664, :733-738). Both callers ask in front of everything else.
DEVO bool note_dropped(const PgSamplerRec& r, const PgCmd& cmd) { return r.stopping != 0 && cmd.type != CMD_SAMPLER_STOP; }

// Sampler::next_free_voice_index (sampler.rs:826-860), one lane per slot (all 64 lanes of the wave call; every lane gets the result): the first
// slot that is not active; else — only with an envelope — the slot in Release with the smallest release_start_frame; else the active slot with the
// smallest note id. The reference's strict `<` keeps the first of equals: ties go to the lower slot.
template <class Pool>
DEVO int note_alloc(const Pool& pool) {
  const PgSamplerRec& r = pool.rec();
  const int lane = (int)(threadIdx.x & 63);
  const bool mine = lane < r.n_voices;
  const bool active = mine && pool.active(lane);
  const bool releasing = active && pool.releasing(lane) && r.slots[lane].release_start_frame != PG_USIZE_MAX;
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

// What slot `slot` holds of the note a CMD_SAMPLER_NOTE_ON starts in it, and the note's speed, volume and panning on its voice (voice.rs:140-160)
template <class Pool>
DEVO void note_slot_start(const Pool& pool, int slot, const PgCmd& cmd) {
  PgSamplerRec& r = pool.rec();
  PgSamplerSlot& s = r.slots[slot];
  const int note = pg_note_on_note(cmd.value64);
  const float volume = cmd.value, panning = pg_note_on_panning(cmd.value64);
  s.note_id = (uint64_t)cmd.param; s.note = note; s.note_volume = volume; s.note_panning = panning; s.release_start_frame = PG_USIZE_MAX;
  pool.set_speed(slot, pool.note_speed(note) * r.pitch_factor, 0.0f);
  pool.set_volume(slot, r.base_volume * volume);
  pool.set_panning(slot, sampler_clamp_pan(r.base_panning + panning));
}

// One message but a note-on in front of frame `now` (Sampler::process_playback_messages, sampler.rs:656-731), on one lane; not a dropped one (note_dropped)
template <class Pool>
DEVO void note_message(const Pool& pool, const PgCmd& cmd, uint64_t now) {
  PgSamplerRec& r = pool.rec();
  if (cmd.type == CMD_SAMPLER_STOP) {   // Sampler::stop (:733-738): taken also while stopping
    r.stopping = r.transient;
    for (int i = 0; i < r.n_voices; ++i) pool.stop(i, now);
    return;
  }
  if (cmd.type == CMD_SAMPLER_ALL_NOTES_OFF) {
    for (int i = 0; i < r.n_voices; ++i) pool.stop(i, now);
  } else if (cmd.type == CMD_SAMPLER_ENV_PARAM) {   // set_envelope_parameter (:184-217, :1122-1131): the pool's one AhdsrParameters
    pool.env_param(cmd);
  } else if (cmd.type == CMD_SAMPLER_PARAM) {   // process_parameter_update (:1076-1120): the stored base value, then every ACTIVE voice
    const bool pitch = cmd.param == PG_SP_TRANSPOSE || cmd.param == PG_SP_FINETUNE;
    if (pitch) {
      if (cmd.param == PG_SP_TRANSPOSE) r.transpose = (int)cmd.value; else r.finetune = (int)cmd.value;
      r.pitch_factor = __longlong_as_double((long long)cmd.value64);
    } else if (cmd.param == PG_SP_VOLUME) r.base_volume = cmd.value;
    else if (cmd.param == PG_SP_PANNING) r.base_panning = cmd.value;
    for (int i = 0; i < r.n_voices; ++i) {
      if (!pool.active(i)) continue;
      if (pitch) pool.set_speed(i, pool.note_speed(r.slots[i].note) * r.pitch_factor, 0.0f);   // set_base_pitch: no glide
      else if (cmd.param == PG_SP_VOLUME) pool.set_volume(i, r.base_volume * r.slots[i].note_volume);
      else if (cmd.param == PG_SP_PANNING) pool.set_panning(i, sampler_clamp_pan(r.base_panning + r.slots[i].note_panning));
    }
  } else if (cmd.type >= CMD_SAMPLER_NOTE_OFF && cmd.type <= CMD_SAMPLER_NOTE_PAN) {
    int i = 0;   // the first slot in index order that plays note `cmd.param` (sampler.rs:776-822); an unknown or ended note: ignored
    while (i < r.n_voices && !(r.slots[i].note_id == (uint64_t)cmd.param && pool.active(i))) ++i;
    if (i == r.n_voices) return;
    if (cmd.type == CMD_SAMPLER_NOTE_OFF) pool.stop(i, now);
    else if (cmd.type == CMD_SAMPLER_NOTE_SPEED) pool.set_speed(i, __longlong_as_double((long long)cmd.value64) * r.pitch_factor, cmd.value);
    else if (cmd.type == CMD_SAMPLER_NOTE_VOLUME) { r.slots[i].note_volume = cmd.value; pool.set_volume(i, r.base_volume * cmd.value); }
    else if (cmd.type == CMD_SAMPLER_NOTE_PAN) { r.slots[i].note_panning = cmd.value; pool.set_panning(i, sampler_clamp_pan(r.base_panning + cmd.value)); }
  }
}

// The end of Sampler::write (sampler.rs:1008-1024) on one lane, for a sampler that was told to stop and is not stopped yet: with no active slot left
// it is stopped — the host, which polls the mapped word `stopped_word` at the top of a write, takes the pool out of its mixer then
template <class Pool>
DEVO void note_end_of_write(const Pool& pool, int32_t* stopped_word) {
  PgSamplerRec& r = pool.rec();
  int active = 0;
  for (int i = 0; i < r.n_voices; ++i) active += pool.active(i) ? 1 : 0;
  if (active == 0) { r.stopped = 1; *(volatile int32_t*)stopped_word = 1; __threadfence_system(); }
}

}  // namespace pgd
