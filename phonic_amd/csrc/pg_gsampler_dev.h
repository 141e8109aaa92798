// The note layer of a granular-mode Sampler (Sampler::with_granular_playback, src/generator/sampler.rs:598-637) on the device: what
// Sampler::write does around its voices' grain pools (sampler.rs:656-731, :974-1028; src/generator/sampler/voice.rs:122-310, :469-502), cut into
// the two halves pg_gsampler_kernel (pg_k_gsampler.hip) runs between the grain launches of consecutive Sampler::write spans:
//   gs_close   the end of SamplerVoice::process for every slot that was active over the span that ends — the AHDSR envelope over the span's staged
//              frames, then the voice's end: the pool ran dry inside the span or the envelope ended it Idle -> the slot is free and its pool reset;
//              a stopping sampler without an active slot is stopped; the staged frames of a slot that was free over the span become zero;
//   gs_open    process_playback_messages in front of the span that begins: note-on with next_free_voice_index, note-off, the per-note setters,
//              the base parameters, the granular parameters, stop — and what changes every voice while notes sound: the envelope's parameters,
//              the matrix's routes and LFOs, the loop range.
// One workgroup per sampler. Decisions take one lane per slot (wave 0); a record is changed by one lane (or one lane per slot / per grain) and
// read again only behind a barrier.
#pragma once
#include "pg_sampler_dev.h"   // ahdsr_note_on, sampler_clamp_pan; through pg_source_dev.h: ahdsr_sequence, ahdsr_scaled, ahdsr_note_off
#include "pg_grain_dev.h"     // mod_lfo_reset, grain_set_parameter

namespace pgd {

#define PG_GS_ENV_TILE 32   // frames per envelope tile: 64 slots x 32 raw outputs are ahdsr_sequence's AHDSR_TILE floats, their stages the AHDSR_TILE behind
static_assert(PG_SAMPLER_MAX_VOICES * PG_GS_ENV_TILE == AHDSR_TILE, "slot s writes its raw outputs at s * PG_GS_ENV_TILE and its stages AHDSR_TILE words behind them");

// What the kernel keeps in LDS
struct GsShared {
  float seq[2 * AHDSR_TILE];                 // ahdsr_sequence's raw outputs and stages of one tile, PG_GS_ENV_TILE per slot
  float gain[PG_SAMPLER_MAX_VOICES];         // Sustain / Idle: the one value of scale_buffer
  float tv_attack[PG_SAMPLER_MAX_VOICES], tv_decay[PG_SAMPLER_MAX_VOICES];
  int32_t flat[PG_SAMPLER_MAX_VOICES];       // the slot's tile is one multiplication (Sustain / Idle as the tile began)
  int32_t act[PG_SAMPLER_MAX_VOICES];        // the slot was active over the span being closed
  int32_t end[PG_SAMPLER_MAX_VOICES];        // ... and ends with it
  int32_t result;
};

DEVO bool gs_cmd_is_message(int type) { return (type >= CMD_SAMPLER_NOTE_ON && type <= CMD_SAMPLER_STOP) || (type >= CMD_SAMPLER_GRAIN_PARAM && type <= CMD_SAMPLER_GRAIN_LOOP); }
DEVO PgGrainVoice* gs_grain(const PgGSamplerLaunch& L, const PgGSampler& r, int slot) { return L.grains + r.grain0 + slot; }
// The record as the host describes it lies inside the tables: anything else is left alone
DEVO bool gs_pool_ok(const PgGSamplerLaunch& L, const PgGSampler& r) {
  return r.note.n_voices >= 1 && r.note.n_voices <= PG_SAMPLER_MAX_VOICES && r.grain0 >= 0 && (uint64_t)r.grain0 + (uint64_t)r.note.n_voices <= (uint64_t)L.n_grains;
}

// GrainPool::reset (granular.rs:495-502) by every lane of the workgroup: each grain deactivated (Grain::deactivate, :1071-1074), the primary
// cleared, triggering on. The generator is NOT reseeded. Also what this implementation keeps beside the pool: no exhaustion, no stop time.
DEVO void gs_pool_reset(PgGrainVoice* V) {
  for (int i = (int)threadIdx.x; i < PG_GRAIN_POOL; i += (int)blockDim.x) { V->grains[i].active = 0; V->grains[i].samples_remaining = 0; }
  if (threadIdx.x == 0) { V->pool.primary = -1; V->pool.trigger_new_grains = 1; V->exhausted_at = PG_USIZE_MAX; V->stop_time = PG_USIZE_MAX; }
}

// Sampler::next_free_voice_index (sampler.rs:826-860) with one lane per slot, as sampler_alloc (pg_sampler_dev.h) has it for file voices: the first
// slot that is not active; else — only with an envelope — the slot in Release with the smallest release_start_frame; else the active slot with the
// smallest note id; ties go to the lower slot. Every lane of the workgroup calls and gets the result.
DEVO int gs_alloc(const PgGSampler& r, GsShared& S) {
  if (threadIdx.x < 64) {
    const int lane = (int)threadIdx.x, n = r.note.n_voices;
    const bool mine = lane < n;
    bool active = false, releasing = false;
    if (mine) {
      active = r.active[lane] != 0;
      releasing = active && r.note.has_envelope && r.env[lane].stage == PG_AHDSR_RELEASE && r.note.slots[lane].release_start_frame != PG_USIZE_MAX;
    }
    int slot;
    const unsigned long long free_mask = __ballot(mine && !active);
    if (free_mask) slot = __ffsll((long long)free_mask) - 1;
    else {
      const bool any_releasing = __ballot(releasing) != 0ull;
      unsigned long long key = PG_USIZE_MAX;
      if (mine && (any_releasing ? releasing : true)) key = any_releasing ? r.note.slots[lane].release_start_frame : r.note.slots[lane].note_id;
      slot = mine ? lane : 64;
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(key, off, 64);
        const int os = __shfl_xor(slot, off, 64);
        if (ok < key || (ok == key && os < slot)) { key = ok; slot = os; }
      }
      if (slot >= n) slot = 0;
    }
    if (lane == 0) S.result = slot;
  }
  __syncthreads();
  const int slot = S.result;
  __syncthreads();
  return slot;
}

// SamplerVoice::start for a granular voice (voice.rs:122-193), every lane of the workgroup: reset() resets the pool only if the slot was active
// (:222-236); GrainPool::start (granular.rs:474-489) sets its values directly — a pool has no smoothers; AhdsrEnvelope::note_on(params, 1.0);
// ModulationMatrix::note_on(note, volume) (matrix.rs:394-408): both LFOs as Lfo::reset leaves them, velocity = the NOTE's volume, keytracking =
// note / 127. The slot's three generators carry on where they are.
DEVO void gs_voice_start(const PgGSamplerLaunch& L, PgGSampler& r, int slot, const PgCmd& cmd, uint64_t now) {
  PgGrainVoice* const V = gs_grain(L, r, slot);
  if (r.active[slot] != 0) gs_pool_reset(V);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int note = (int)(cmd.value64 & 0xff);
    const float volume = cmd.value, panning = __uint_as_float((uint32_t)(cmd.value64 >> 32));
    PgSamplerSlot& s = r.note.slots[slot];
    s.note_id = (uint64_t)cmd.param; s.note = note; s.note_volume = volume; s.note_panning = panning; s.release_start_frame = PG_USIZE_MAX;
    PgGrainPool& P = V->pool;
    P.trigger_new_grains = 1; P.trigger_phase = 1.0f;
    P.speed = L.speed_tab[note & 255] * r.note.pitch_factor;
    P.volume = r.note.base_volume * volume;
    P.panning = sampler_clamp_pan(r.note.base_panning + panning);
    P.playhead = V->params.position; P.playing_loop_range = 0;
    V->start_time = now; V->stop_time = PG_USIZE_MAX; V->exhausted_at = PG_USIZE_MAX;
    if (r.note.has_envelope) { PgEnvState st = r.env[slot]; ahdsr_note_on(st, r.env_params, 1.0f); r.env[slot] = st; }
    if (V->mod.on) {
      for (int l = 0; l < 2; ++l) { PgModLfo m = V->mod.lfo[l]; mod_lfo_reset(m); V->mod.lfo[l] = m; }
      V->mod.velocity = volume;
      V->mod.note_pitch = (float)note / 127.0f;
    }
    r.active[slot] = 1;
  }
  __syncthreads();
}
// SamplerVoice::stop (voice.rs:196-219) on one lane: an active slot only; with an envelope note_off alone — the pool goes on triggering — without
// one GrainPool::stop (the file source behind the voice is never written in this mode: its stop() starts a fade that never runs, and it is
// never exhausted).
DEVO void gs_voice_stop(const PgGSamplerLaunch& L, PgGSampler& r, int slot, uint64_t now) {
  if (r.active[slot] == 0) return;
  r.note.slots[slot].release_start_frame = now;
  if (r.note.has_envelope) { PgEnvState st = r.env[slot]; ahdsr_note_off(st, r.env_params); r.env[slot] = st; }
  else gs_grain(L, r, slot)->pool.trigger_new_grains = 0;
}
// The first slot in index order that plays note `note_id` (sampler.rs:776-822), -1: none
DEVO int gs_find(const PgGSampler& r, int note_id) {
  for (int i = 0; i < r.note.n_voices; ++i) if (r.active[i] != 0 && r.note.slots[i].note_id == (uint64_t)note_id) return i;
  return -1;
}

// process_playback_messages (sampler.rs:656-731) in front of frame L.t: the sampler's commands of that frame, in list order. Every lane of the
// workgroup walks the list; a barrier stands behind every command.
DEVO void gs_open(const PgGSamplerLaunch& L, PgGSampler& r, GsShared& S) {
  const int tid = (int)threadIdx.x, n = r.note.n_voices;
  const uint64_t now = L.t;
  for (int ci = 0; ci < L.n_cmds; ++ci) {
    const PgCmd cmd = L.cmds[ci];
    if (cmd.unit != r.note.unit || cmd.frame != L.frame || cmd.target != r.index || !gs_cmd_is_message(cmd.type)) continue;
    if (cmd.type == CMD_SAMPLER_STOP) {   // Sampler::stop (:733-738): taken also while stopping
      if (tid == 0) { r.note.stopping = r.note.transient; for (int i = 0; i < n; ++i) gs_voice_stop(L, r, i, now); }
      __syncthreads();
      continue;
    }
    if (r.note.stopping) continue;   // every trigger is dropped while the sampler stops (:663-664)
    if (cmd.type == CMD_SAMPLER_NOTE_ON) {
      const int slot = gs_alloc(r, S);
      gs_voice_start(L, r, slot, cmd, now);
      continue;
    }
    if (cmd.type == CMD_SAMPLER_GRAIN_PARAM) {   // Sampler::set_granular_parameter (:299-360): the sampler's ONE parameter set — here every slot's copy of it
      if (tid < n) { PgGrainParams p = gs_grain(L, r, tid)->params; grain_set_parameter(p, (uint32_t)cmd.param, cmd.value); gs_grain(L, r, tid)->params = p; }
    } else if (cmd.type == CMD_SAMPLER_MOD_ROUTE || cmd.type == CMD_SAMPLER_LFO_RATE || cmd.type == CMD_SAMPLER_LFO_WAVEFORM) {
      // SetModulation / ClearModulation, ML1R / ML2R / ML1W / ML2W (:704-720, :1148-1186, :1210-1244): the matrix of EVERY voice, playing or free. The LFOs
      // draw nothing and keep their phases; a later note's reset keeps what is written here.
      if (tid < n) {
        PgGrainMod& m = gs_grain(L, r, tid)->mod;
        if (m.on) {
          if (cmd.type == CMD_SAMPLER_MOD_ROUTE) grain_route_apply(cmd, m.amount, m.bipolar);
          else for (int l = 0; l < 2; ++l) grain_lfo_apply(cmd, cmd.type == CMD_SAMPLER_LFO_RATE, l, m.lfo[l]);
        }
      }
    } else if (cmd.type == CMD_SAMPLER_GRAIN_LOOP) {   // SamplerMessage::SetLoopRange (:1246-1271, voice.rs:312-339): every voice's pool
      if (tid < n) { PgGrainParams p = gs_grain(L, r, tid)->params; grain_loop_apply(cmd, p); gs_grain(L, r, tid)->params = p; }
    } else if (cmd.type == CMD_SAMPLER_ENV_PARAM) {   // set_envelope_parameter (:184-217, :1122-1131): the pool's one AhdsrParameters; gs_close reads it once per span
      if (tid == 0 && r.note.has_envelope) { PgEnvParams p = r.env_params; ahdsr_set_param(p, cmd); r.env_params = p; }
    } else if (tid == 0) {
      if (cmd.type == CMD_SAMPLER_ALL_NOTES_OFF) {
        for (int i = 0; i < n; ++i) gs_voice_stop(L, r, i, now);
      } else if (cmd.type == CMD_SAMPLER_PARAM) {   // process_parameter_update (:1076-1120): the stored base value, then every ACTIVE voice's pool, directly
        if (cmd.param == PG_SP_TRANSPOSE || cmd.param == PG_SP_FINETUNE) {
          if (cmd.param == PG_SP_TRANSPOSE) r.note.transpose = (int)cmd.value; else r.note.finetune = (int)cmd.value;
          r.note.pitch_factor = __longlong_as_double((long long)cmd.value64);
        } else if (cmd.param == PG_SP_VOLUME) r.note.base_volume = cmd.value;
        else if (cmd.param == PG_SP_PANNING) r.note.base_panning = cmd.value;
        for (int i = 0; i < n; ++i) {
          if (r.active[i] == 0) continue;
          PgGrainPool& P = gs_grain(L, r, i)->pool;
          if (cmd.param == PG_SP_TRANSPOSE || cmd.param == PG_SP_FINETUNE) P.speed = L.speed_tab[r.note.slots[i].note & 255] * r.note.pitch_factor;
          else if (cmd.param == PG_SP_VOLUME) P.volume = r.note.base_volume * r.note.slots[i].note_volume;
          else if (cmd.param == PG_SP_PANNING) P.panning = sampler_clamp_pan(r.note.base_panning + r.note.slots[i].note_panning);
        }
      } else {
        const int i = gs_find(r, cmd.param);
        if (i >= 0) {   // (an unknown or ended note: ignored)
          PgGrainPool& P = gs_grain(L, r, i)->pool;
          if (cmd.type == CMD_SAMPLER_NOTE_OFF) gs_voice_stop(L, r, i, now);
          else if (cmd.type == CMD_SAMPLER_NOTE_SPEED) P.speed = __longlong_as_double((long long)cmd.value64) * r.note.pitch_factor;   // (no glide: the pool gets the speed alone)
          else if (cmd.type == CMD_SAMPLER_NOTE_VOLUME) { r.note.slots[i].note_volume = cmd.value; P.volume = r.note.base_volume * cmd.value; }
          else if (cmd.type == CMD_SAMPLER_NOTE_PAN) { r.note.slots[i].note_panning = cmd.value; P.panning = sampler_clamp_pan(r.note.base_panning + cmd.value); }
        }
      }
    }
    __syncthreads();
  }
}

// The end of SamplerVoice::process (voice.rs:469-502) and of Sampler::write (sampler.rs:1008-1024) for the span [t0, t1). Every lane of the workgroup.
DEVO void gs_close(const PgGSamplerLaunch& L, PgGSampler& r, uint64_t t0, uint64_t t1, GsShared& S) {
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x, n = r.note.n_voices;
  // the span's frames in the staging buffers (the host stages one chunk of the main mixer at most: anything else is left alone)
  const bool staged_ok = t0 >= L.chunk_t0 && t1 > t0 && t1 - L.chunk_t0 <= (uint64_t)PG_MAX_FRAMES;
  const uint64_t off = t0 - L.chunk_t0;
  const int frames = staged_ok ? (int)(t1 - t0) : 0;
  if (tid < PG_SAMPLER_MAX_VOICES) { S.act[tid] = tid < n ? r.active[tid] : 0; S.end[tid] = 0; }
  __syncthreads();
  // 1. the envelope over the span's frames (voice.rs:469-486): a tile that begins in Sustain or Idle is one multiplication by output() — the
  //    reference's scale_buffer branch, and what its per-frame walk hands out from there on; any other tile is walked frame by frame by the
  //    slot's lane (ahdsr_sequence) and scaled by all lanes (ahdsr_scaled)
  if (r.note.has_envelope) {
    const PgEnvParams p = r.env_params;
    for (int base = 0; base < frames; base += PG_GS_ENV_TILE) {
      const int tn = frames - base < PG_GS_ENV_TILE ? frames - base : PG_GS_ENV_TILE;
      if (tid < n && S.act[tid]) {
        PgEnvState st = r.env[tid];
        if (st.stage == PG_AHDSR_SUSTAIN || st.stage == PG_AHDSR_IDLE) { S.flat[tid] = 1; S.gain[tid] = st.output; }
        else {
          S.flat[tid] = 0;
          S.tv_attack[tid] = st.target_volume;
          ahdsr_sequence(st, p, S.seq + tid * PG_GS_ENV_TILE, tn);
          S.tv_decay[tid] = st.target_volume;
          r.env[tid] = st;
        }
      }
      __syncthreads();
      for (int i = tid; i < n * PG_GS_ENV_TILE; i += nt) {
        const int s = i / PG_GS_ENV_TILE, f = i % PG_GS_ENV_TILE;
        if (f >= tn || !S.act[s]) continue;
        float val;
        if (S.flat[s]) val = S.gain[s];
        else {
          const int stage = ((const int*)S.seq + AHDSR_TILE)[s * PG_GS_ENV_TILE + f];
          val = ahdsr_scaled(stage, S.seq[s * PG_GS_ENV_TILE + f], stage == PG_AHDSR_ATTACK ? S.tv_attack[s] : S.tv_decay[s], p);
        }
        float* const fr = gs_grain(L, r, s)->staged + (off + (uint64_t)(base + f)) * 2;
        fr[0] *= val; fr[1] *= val;
      }
      __syncthreads();
    }
  }
  // 2. the voice's end (voice.rs:488-502): the pool became exhausted inside the span, or the envelope ended it Idle
  //    INVARIANT the unit kernel relies on (voice_write's granular branch, pg_source_dev.h): behind the chunk's closing launch no slot's record holds an
  //    exhausted_at inside the chunk — the unit kernel would mark the pool voice finished for good. So this step does not depend on staged_ok, every
  //    chunk ends with a closing launch in front of its unit kernels (render_chunk), and gs_pool_reset clears the word.
  if (tid < n && S.act[tid]) S.end[tid] = (gs_grain(L, r, tid)->exhausted_at < t1 || (r.note.has_envelope && r.env[tid].stage == PG_AHDSR_IDLE)) ? 1 : 0;
  __syncthreads();
  for (int s = 0; s < n; ++s) {
    if (!S.end[s]) continue;
    PgGrainVoice* const V = gs_grain(L, r, s);
    gs_pool_reset(V);
    if (tid == 0) { V->start_time = PG_USIZE_MAX; r.active[s] = 0; r.note.slots[s].release_start_frame = PG_USIZE_MAX; }
  }
  // 3. a slot that was free over the span delivered nothing: its staged frames are zero, whatever an earlier note left there
  for (int s = 0; s < n; ++s) {
    if (S.act[s]) continue;
    PgGrainVoice* const V = gs_grain(L, r, s);
    float* const fr = V->staged + off * 2;
    for (int i = tid; i < 2 * frames; i += nt) fr[i] = 0.0f;
    if (tid == 0 && staged_ok) V->stage_pos = L.chunk_t0;
  }
  __syncthreads();
  // 4. the end of Sampler::write (sampler.rs:1008-1024): a sampler that was told to stop and has no active slot left is stopped
  if (tid == 0 && r.note.stopping && !r.note.stopped) {
    int active = 0;
    for (int s = 0; s < n; ++s) active += r.active[s] != 0 ? 1 : 0;
    if (active == 0) { r.note.stopped = 1; *(volatile int32_t*)(L.stopped + r.index) = 1; __threadfence_system(); }
  }
  __syncthreads();
}

}  // namespace pgd
