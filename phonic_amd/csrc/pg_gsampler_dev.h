// A granular-mode Sampler (Sampler::with_granular_playback, src/generator/sampler.rs:598-637) under the note layer (pg_note_dev.h) on the device: what
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
#include "pg_note_dev.h"      // note_alloc, note_slot_start, note_message, note_end_of_write; pg_source_dev.h: ahdsr_*
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

// The note layer's view of the pool (pg_note_dev.h): slot i is grain record grain0 + i; its envelope and whether it plays are the sampler record's
struct GrainPools {
  const PgGSamplerLaunch& L;
  PgGSampler& r;
  DEVO PgSamplerRec& rec() const { return r.note; }
  DEVO bool active(int i) const { return r.active[i] != 0; }
  DEVO bool releasing(int i) const { return r.note.has_envelope && r.env[i].stage == PG_AHDSR_RELEASE; }
  // SamplerVoice::stop (voice.rs:196-219): an active slot only; with an envelope note_off alone — the pool goes on triggering — without one
  // GrainPool::stop (the file source behind the voice is never written in this mode: its stop() starts a fade that never runs, and it is
  // never exhausted).
  DEVO void stop(int i, uint64_t now) const {
    if (r.active[i] == 0) return;
    r.note.slots[i].release_start_frame = now;
    if (r.note.has_envelope) { PgEnvState st = r.env[i]; ahdsr_note_off(st, r.env_params); r.env[i] = st; }
    else gs_grain(L, r, i)->pool.trigger_new_grains = 0;
  }
  // GrainPool::start / set_speed / set_volume / set_panning set the values directly: a pool has no smoothers and gets the speed without the glide
  DEVO void set_speed(int i, double speed, float) const { gs_grain(L, r, i)->pool.speed = speed; }
  DEVO void set_volume(int i, float v) const { gs_grain(L, r, i)->pool.volume = v; }
  DEVO void set_panning(int i, float p) const { gs_grain(L, r, i)->pool.panning = p; }
  DEVO void env_param(const PgCmd& cmd) const {   // gs_close reads the parameters once per span
    if (r.note.has_envelope) { PgEnvParams p = r.env_params; ahdsr_set_param(p, cmd); r.env_params = p; }
  }
  DEVO double note_speed(int note) const { return L.speed_tab[note & 255]; }
};

// Sampler::next_free_voice_index with one lane per slot of wave 0 (note_alloc). Every lane of the workgroup calls and gets the result.
DEVO int gs_alloc(const GrainPools& pool, GsShared& S) {
  if (threadIdx.x < 64) { const int slot = note_alloc(pool); if (threadIdx.x == 0) S.result = slot; }
  __syncthreads();
  const int slot = S.result;
  __syncthreads();
  return slot;
}

// SamplerVoice::start for a granular voice (voice.rs:122-193), every lane of the workgroup: reset() resets the pool only if the slot was active
// (:222-236); GrainPool::start (granular.rs:474-489) sets its values directly; AhdsrEnvelope::note_on(params, 1.0);
// ModulationMatrix::note_on(note, volume) (matrix.rs:394-408): both LFOs as Lfo::reset leaves them, velocity = the NOTE's volume, keytracking =
// note / 127. The slot's three generators carry on where they are.
DEVO void gs_voice_start(const GrainPools& pool, int slot, const PgCmd& cmd, uint64_t now) {
  PgGSampler& r = pool.r;
  PgGrainVoice* const V = gs_grain(pool.L, r, slot);
  if (r.active[slot] != 0) gs_pool_reset(V);
  __syncthreads();
  if (threadIdx.x == 0) {
    note_slot_start(pool, slot, cmd);
    PgGrainPool& P = V->pool;
    P.trigger_new_grains = 1; P.trigger_phase = 1.0f;
    P.playhead = V->params.position; P.playing_loop_range = 0;
    V->start_time = now; V->stop_time = PG_USIZE_MAX; V->exhausted_at = PG_USIZE_MAX;
    if (r.note.has_envelope) { PgEnvState st = r.env[slot]; ahdsr_note_on(st, r.env_params, 1.0f); r.env[slot] = st; }
    if (V->mod.on) {
      for (int l = 0; l < 2; ++l) { PgModLfo m = V->mod.lfo[l]; mod_lfo_reset(m); V->mod.lfo[l] = m; }
      V->mod.velocity = cmd.value;
      V->mod.note_pitch = (float)pg_note_on_note(cmd.value64) / 127.0f;
    }
    r.active[slot] = 1;
  }
  __syncthreads();
}

// process_playback_messages (sampler.rs:656-731) in front of frame L.t: the sampler's commands of that frame, in list order. Every lane of the
// workgroup walks the list; a barrier stands behind every command.
DEVO void gs_open(const PgGSamplerLaunch& L, PgGSampler& r, GsShared& S) {
  const int tid = (int)threadIdx.x, n = r.note.n_voices;
  const GrainPools pool{L, r};
  for (int ci = 0; ci < L.n_cmds; ++ci) {
    const PgCmd cmd = L.cmds[ci];
    if (cmd.unit != r.note.unit || cmd.frame != L.frame || cmd.target != r.index || !pg_cmd_is_sampler_message(cmd.type)) continue;
    if (note_dropped(r.note, cmd)) continue;   // (by every lane: no barrier behind a dropped message)
    if (cmd.type == CMD_SAMPLER_NOTE_ON) {
      const int slot = gs_alloc(pool, S);
      gs_voice_start(pool, slot, cmd, L.t);
      continue;
    }
    // the note layer's messages run on one lane; the granular-only ones change every slot's record, playing or free, one lane per slot
    if (cmd.type < CMD_SAMPLER_GRAIN_PARAM || cmd.type == CMD_SAMPLER_ENV_PARAM) { if (tid == 0) note_message(pool, cmd, L.t); }
    else if (tid < n) {
      PgGrainVoice& V = *gs_grain(L, r, tid);
      if (cmd.type == CMD_SAMPLER_GRAIN_PARAM) {   // Sampler::set_granular_parameter (:299-360): the sampler's ONE parameter set — here every slot's copy of it
        PgGrainParams p = V.params; grain_set_parameter(p, (uint32_t)cmd.param, cmd.value); V.params = p;
      } else if (cmd.type == CMD_SAMPLER_GRAIN_LOOP) {   // SamplerMessage::SetLoopRange (:1246-1271, voice.rs:312-339): every voice's pool
        PgGrainParams p = V.params; grain_loop_apply(cmd, p); V.params = p;
      } else if (V.mod.on) {
        // SetModulation / ClearModulation, ML1R / ML2R / ML1W / ML2W (:704-720, :1148-1186, :1210-1244): the matrix of EVERY voice. The LFOs
        // draw nothing and keep their phases; a later note's reset keeps what is written here.
        if (cmd.type == CMD_SAMPLER_MOD_ROUTE) grain_route_apply(cmd, V.mod.amount, V.mod.bipolar);
        else for (int l = 0; l < 2; ++l) grain_lfo_apply(cmd, cmd.type == CMD_SAMPLER_LFO_RATE, l, V.mod.lfo[l]);
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
  if (tid == 0 && r.note.stopping && !r.note.stopped) note_end_of_write(GrainPools{L, r}, L.stopped + r.index);
  __syncthreads();
}

}  // namespace pgd
