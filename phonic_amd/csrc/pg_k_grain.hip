// pg_grain_kernel: the grain engine of the sampler's granular voices (GrainPool<100>, src/generator/sampler/granular.rs) — one workgroup per
// living granular voice, launched on the write's stream in front of the unit kernels of a chunk's piece. It renders the voice's frames of the
// piece as interleaved stereo f32 into the voice's staging buffer; the exact unit kernel takes them as the voice's source output (a plain copy
// in its source stage, pg_source_dev.h) and puts the volume envelope on top. Commands of the piece (volume, panning, speed, stop, release, the
// matrix's, the granular parameters and the loop range) are read from the launch's command list and applied at their frames.
//
// Per tile of PG_GRAIN_TILE frames (pg_grain_dev.h has the arithmetic):
//   0  voices with a modulation matrix only (pg_graph_set_voice_modulation_matrix): one lane per LFO walks its f32 phase recurrence, wraps and
//      draws over the tile's rendered frames and leaves the raw values in LDS; then one lane per (target, frame) forms the target's sum in slot
//      order from the 4 x 7 routing table as of its frame. Phase 1 reads seven floats per frame, nothing else of the matrix is in its walk;
//   1  lane 0 walks the scheduler frame by frame — the voice's parameters and loop range as of each frame (CMD_VOICE_GRAIN_PARAM / _LOOP act in
//      front of theirs) — and leaves the activations, one slot per frame at most, in LDS;
//   2  lane s walks slot s: takes its activations at their frames, steps Grain::process's f64 recurrences and leaves, per frame, the f32 read
//      position and the window table's index and fraction in LDS (12 bytes per slot and frame: 38 KB for 100 slots x 32 frames); the slot's
//      record stays in the lane's registers for the whole launch. Slots without an active grain in the tile are left out of what follows;
//   3  all lanes, spread over (active slot, frame): window lookup in the row of the grain's own window_mode — the row of the voice's window as the
//      launch began is staged in LDS, a grain born under another window reads the global table — the four reads of the buffer, Catmull-Rom,
//      the threshold test, the two stereo terms — written over the slot's LDS words; then one lane per (frame, channel) adds the terms in
//      ascending slot order and stores the frame.
// State does not depend on how a render is cut into launches or tiles: every recurrence is walked frame by frame in the reference's order.
#include "pg_host_internal.h"
#include "pg_grain_dev.h"

using namespace pgd;

#define GT PG_GRAIN_TILE
#define GRAIN_CMD_CAP 64

__device__ __forceinline__ bool grain_cmd_matches(const PgCmd& c, int voice) {
  return c.target == voice && (c.type == CMD_VOICE_VOLUME || c.type == CMD_VOICE_PAN || c.type == CMD_VOICE_SPEED || c.type == CMD_VOICE_STOP || c.type == CMD_VOICE_RELEASE ||
                               c.type == CMD_VOICE_MOD_ROUTE || c.type == CMD_VOICE_LFO_RATE || c.type == CMD_VOICE_LFO_WAVEFORM || c.type == CMD_VOICE_GRAIN_PARAM ||
                               c.type == CMD_VOICE_GRAIN_LOOP);
}

__global__ void __launch_bounds__(256) pg_grain_kernel(PgGrainLaunch L) {
  __shared__ float s_lut[PG_GRAIN_LUT_N];
  __shared__ float s_pos[PG_GRAIN_POOL * GT];     // phase 2: read position; phase 3: the left term
  __shared__ float s_frac[PG_GRAIN_POOL * GT];    // phase 2: window fraction; phase 3: the right term
  __shared__ uint32_t s_ti[PG_GRAIN_POOL * GT];   // window index | (1 + frame of the activation the grain's volume / panning come from, 0: the slot's as the tile began) << 16 | the grain's window_mode << 24
  __shared__ GrainActivation s_act[GT];
  __shared__ int s_end[PG_GRAIN_POOL];
  __shared__ float s_vol[PG_GRAIN_POOL], s_pan[PG_GRAIN_POOL];
  __shared__ int s_touched[PG_GRAIN_POOL];
  __shared__ int s_live[PG_GRAIN_POOL];
  __shared__ int s_wcnt[2];
  __shared__ int s_cmd[GRAIN_CMD_CAP];
  __shared__ int s_ncmd;
  // phase 0 (voices with a modulation matrix): the LFOs' raw values and the targets' sums of the tile, the routing table and the LFO records
  __shared__ float s_lfo[2][GT];
  __shared__ float s_mod[PG_GMOD_TARGETS][GT];
  __shared__ float s_ramt[PG_GMOD_SOURCES][PG_GMOD_TARGETS];
  __shared__ int s_rbip[PG_GMOD_SOURCES][PG_GMOD_TARGETS];
  __shared__ PgModLfo s_lfo_state[2];
  __shared__ float s_mstatic[2];   // velocity, note_pitch
  __shared__ int s_lfo_cursor[2];  // the LFO lanes' places in the command list

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x >= L.n_live) return;
  const int rec = L.live[blockIdx.x];
  if (rec < 0 || (uint32_t)rec >= L.n_recs) return;
  PgGrainVoice* const V = L.recs + rec;
  {  // the voice has ended (its pool ran dry, its envelope went Idle, it was stopped before it began): tell the host, render nothing
    const PgVoice* const pv = L.voices + V->voice;
    if (!pv->active || pv->finished) {
      if (tid == 0) { *(volatile int32_t*)(L.ended + rec) = 1; __threadfence_system(); }
      return;
    }
  }
  const uint64_t stage_off = L.t0 - L.chunk_t0;
  if (L.t0 < L.chunk_t0 || stage_off + L.n > PG_MAX_FRAMES) return;   // (the host stages one chunk of the main mixer at most)
  const int voice = V->voice;
  const float* const pcm = V->pcm;
  const uint64_t len = V->n_frames;
  float* const staged = V->staged + stage_off * 2;
  float* const pos_trace = V->pos_trace ? V->pos_trace + stage_off : nullptr;   // playback status: the playhead behind every frame (PgGrainVoice::pos_trace)
  const int window = V->params.window & (PG_GRAIN_WINDOWS - 1);

  for (int i = tid; i < PG_GRAIN_LUT_N; i += 256) s_lut[i] = L.lut[window * PG_GRAIN_LUT_N + i];
  if (tid == 0) s_ncmd = 0;
  __syncthreads();
  // the voice's commands of this piece: the list is sorted by (unit, frame), so a voice's commands stand in frame order
  for (int i = tid; i < L.n_cmds; i += 256) {
    if (grain_cmd_matches(L.cmds[i], voice)) { const int k = atomicAdd(&s_ncmd, 1); if (k < GRAIN_CMD_CAP) s_cmd[k] = i; }
  }
  __syncthreads();
  const int n_cmd = s_ncmd;
  const bool cmd_overflow = n_cmd > GRAIN_CMD_CAP;   // (more than the LDS list holds: lane 0 walks the launch's list itself)
  if (tid == 0 && !cmd_overflow) {  // back into list order
    for (int i = 1; i < n_cmd; ++i) { const int x = s_cmd[i]; int j = i - 1; while (j >= 0 && s_cmd[j] > x) { s_cmd[j + 1] = s_cmd[j]; --j; } s_cmd[j + 1] = x; }
  }

  PgGrain g;
  if (tid < PG_GRAIN_POOL) g = V->grains[tid];
  else { g.active = 0; g.samples_remaining = 0; }
  GrainSched S;
  uint64_t stop_time = UINT64_MAX, exhausted_at = UINT64_MAX;
  int cmd_cursor = 0;
  if (tid == 0) {
    S.p = V->params; S.pool = V->pool; S.n_frames = len; S.sample_rate = L.sample_rate;
    S.prim_phase = 0.0; S.prim_inc = 0.0;
    if (S.pool.primary >= 0 && S.pool.primary < PG_GRAIN_POOL) { S.prim_phase = V->grains[S.pool.primary].window_phase; S.prim_inc = V->grains[S.pool.primary].window_increment; }
    stop_time = V->stop_time; exhausted_at = V->exhausted_at;
  }
  const uint64_t start_time = V->start_time;
  const int has_env = V->has_env;
  const bool has_mod = V->mod.on != 0;   // (the same for every lane of the workgroup)
  int route_cursor = 0;
  if (has_mod) {
    if (tid < PG_GMOD_SOURCES * PG_GMOD_TARGETS) { (&s_ramt[0][0])[tid] = (&V->mod.amount[0][0])[tid]; (&s_rbip[0][0])[tid] = (&V->mod.bipolar[0][0])[tid]; }
    if (tid == 64 || tid == 128) { s_lfo_state[(tid >> 6) - 1] = V->mod.lfo[(tid >> 6) - 1]; s_lfo_cursor[(tid >> 6) - 1] = 0; }
    if (tid == 192) { s_mstatic[0] = V->mod.velocity; s_mstatic[1] = V->mod.note_pitch; }
  }
  // the voice's next command at or behind `cursor` in the launch's list (-1: none): a lane's own walk
  auto peek_cmd = [&](int& cursor) -> int {
    if (!cmd_overflow) return cursor < n_cmd ? s_cmd[cursor] : -1;
    while (cursor < L.n_cmds && !grain_cmd_matches(L.cmds[cursor], voice)) ++cursor;
    return cursor < L.n_cmds ? cursor : -1;
  };
  __syncthreads();

  for (uint32_t base = 0; base < L.n; base += GT) {
    const int tn = (int)(L.n - base < (uint32_t)GT ? L.n - base : (uint32_t)GT);
    const uint64_t tile_t = L.t0 + base;
    if (tid < PG_GRAIN_POOL) {
      s_end[tid] = g.active ? (int)(g.samples_remaining < 0x3fffffffull ? g.samples_remaining : 0x3fffffffull) : 0;
      s_vol[tid] = g.volume; s_pan[tid] = g.panning; s_touched[tid] = 0;
    }
    __syncthreads();
    // ---- phase 0: the modulation matrix ----
    if (has_mod) {
      int otid = tid;
      asm volatile("" : "+v"(otid));   // (opaque: the lane's LDS addresses below are formed here, not in front of the tile loop to be kept in registers through phases 1-3)
      if (otid == 64 || otid == 128) {  // one lane per LFO, in waves of their own
        const int l = (otid >> 6) - 1;
        PgModLfo m = s_lfo_state[l];
        int lfo_cursor = s_lfo_cursor[l];
        for (int f = 0; f < tn; ++f) {
          const uint32_t lf = base + (uint32_t)f;
          for (;;) {  // Lfo::set_rate / set_waveform in front of this frame (matrix.rs:417-429)
            const int ci = peek_cmd(lfo_cursor);
            if (ci < 0) break;
            const PgCmd c = L.cmds[ci];
            if (c.frame > lf) break;
            ++lfo_cursor;
            if (c.type == CMD_VOICE_LFO_RATE || c.type == CMD_VOICE_LFO_WAVEFORM) grain_lfo_apply(c, c.type == CMD_VOICE_LFO_RATE, l, m);
          }
          if (tile_t + (uint64_t)f >= start_time) s_lfo[l][f] = mod_lfo_run(m);
        }
        s_lfo_state[l] = m; s_lfo_cursor[l] = lfo_cursor;
      }
      // the sums, in segments cut at the tile's route commands: every frame takes exactly the routes set in front of it. The walk over the
      // command list is the same in every lane; lane 0 changes the table between two segments.
      const int mk = otid / GT, mf = otid % GT;   // lane (target, frame)
      for (int seg0 = 0;;) {
        for (;;) {  // ModulationMatrixSlot::update_target (matrix.rs:60-83) in front of frame seg0; the other commands are not this walk's
          const int ci = peek_cmd(route_cursor);
          if (ci < 0 || L.cmds[ci].frame > base + (uint32_t)seg0) break;
          ++route_cursor;
          if (tid == 0 && L.cmds[ci].type == CMD_VOICE_MOD_ROUTE) grain_route_apply(L.cmds[ci], s_ramt, s_rbip);
        }
        int seg1 = tn;
        for (int cur = route_cursor;;) {  // the next route command inside the tile ends the segment
          const int ci = peek_cmd(cur);
          if (ci < 0 || L.cmds[ci].frame >= base + (uint32_t)tn) break;
          if (L.cmds[ci].type == CMD_VOICE_MOD_ROUTE) { seg1 = (int)(L.cmds[ci].frame - base); break; }
          ++cur;
        }
        __syncthreads();   // (the LFO lanes' values and lane 0's table)
        if (mk < PG_GMOD_TARGETS && mf >= seg0 && mf < seg1 && tile_t + (uint64_t)mf >= start_time) {
          // ModulationMatrix::output (matrix.rs:194-303): LFO 1, LFO 2, velocity, keytracking — each only if it routes to the target
          float total = 0.0f;
          if (s_ramt[0][mk] != 0.0f) total += mod_bipolar_source(s_lfo[0][mf], s_rbip[0][mk]) * s_ramt[0][mk];
          if (s_ramt[1][mk] != 0.0f) total += mod_bipolar_source(s_lfo[1][mf], s_rbip[1][mk]) * s_ramt[1][mk];
          if (s_ramt[2][mk] != 0.0f) total += mod_unipolar_source(s_mstatic[0], s_rbip[2][mk]) * s_ramt[2][mk];
          if (s_ramt[3][mk] != 0.0f) total += mod_unipolar_source(s_mstatic[1], s_rbip[3][mk]) * s_ramt[3][mk];
          s_mod[mk][mf] = total;
          if (mf == tn - 1) V->mod.last[mk] = total;
        }
        __syncthreads();   // (phase 1, or lane 0's next change of the table, begins behind it)
        if (seg1 >= tn) break;
        seg0 = seg1;
      }
    }
    // ---- phase 1: the scheduler ----
    if (tid == 0) {
      int max_end = -1;
      for (int f = 0; f < tn; ++f) {
        const uint64_t t = tile_t + (uint64_t)f;
        const uint32_t lf = base + (uint32_t)f;
        for (;;) {  // commands due at this frame (GrainPool::set_volume / set_panning / set_speed / stop, :491-514): they act on what is activated from here on
          int ci = -1;
          if (!cmd_overflow) { if (cmd_cursor < n_cmd) ci = s_cmd[cmd_cursor]; }
          else { while (cmd_cursor < L.n_cmds && !grain_cmd_matches(L.cmds[cmd_cursor], voice)) ++cmd_cursor; if (cmd_cursor < L.n_cmds) ci = cmd_cursor; }
          if (ci < 0) break;
          const PgCmd c = L.cmds[ci];
          if (c.frame > lf) break;
          ++cmd_cursor;
          if (c.type == CMD_VOICE_VOLUME) S.pool.volume = c.value;
          else if (c.type == CMD_VOICE_PAN) S.pool.panning = c.value;
          else if (c.type == CMD_VOICE_SPEED) S.pool.speed = __longlong_as_double((long long)c.value64);   // (the glide is ignored: SamplerVoice::set_speed hands the pool the speed alone)
          else if (c.type == CMD_VOICE_STOP) stop_time = c.value64;
          else if (c.type == CMD_VOICE_RELEASE && !has_env) S.pool.trigger_new_grains = 0;   // without an envelope: SamplerVoice::stop -> GrainPool::stop
          else if (exhausted_at != UINT64_MAX) {}   // (the pool ran dry in front of this frame: the voice ends with that call, it takes no parameters any more)
          else if (c.type == CMD_VOICE_GRAIN_PARAM) {
            grain_set_parameter(S.p, (uint32_t)c.value64, c.value);
            // in front of the note: GrainPool::start reads the position at note-on (:487)
            if ((uint32_t)c.value64 == PG_GP_POSITION && L.t0 + (uint64_t)c.frame < start_time) S.pool.playhead = c.value;
          } else if (c.type == CMD_VOICE_GRAIN_LOOP) grain_loop_apply(c, S.p);
          // (the modulation matrix's commands were taken in phase 0)
        }
        if (t < start_time) { s_act[f].slot = -1; continue; }
        if (t >= stop_time) S.pool.trigger_new_grains = 0;
        GrainActivation a;
        const GrainModFrame m = {&s_mod[0][f]};
        if (has_mod) grain_sched_frame<true>(S, s_end, f, a, m);
        else grain_sched_frame<false>(S, s_end, f, a, m);
        if (a.slot >= 0) { s_act[f] = a; s_touched[a.slot] = 1; }
        else s_act[f].slot = -1;
        // GrainPool::playback_position(parameters, pos_mod) as a process call that ends behind this frame finds it (voice.rs:434-453)
        if (pos_trace) pos_trace[lf] = has_mod ? grain_playback_position<true>(S, m.position()) : grain_playback_position<false>(S, 0.0f);
        if (!S.pool.trigger_new_grains && exhausted_at == UINT64_MAX) {
          if (max_end < 0) { max_end = 0; for (int s = 0; s < PG_GRAIN_POOL; ++s) max_end = s_end[s] > max_end ? s_end[s] : max_end; }
          if (max_end <= f + 1) exhausted_at = t;   // nothing is active behind this frame and nothing will be triggered: is_exhausted (:442-444)
        }
      }
    }
    __syncthreads();
    // ---- phase 2: one lane per slot ----
    const bool live = tid < PG_GRAIN_POOL && (g.active || s_touched[tid]);
    if (live) {
      uint32_t src = 0;
      for (int f = 0; f < tn; ++f) {
        if (s_act[f].slot == tid) { grain_take_activation(g, s_act[f]); src = (uint32_t)(f + 1); }
        const int o = tid * GT + f;
        if (g.active) {
          float position, fraction;
          uint32_t index;
          grain_step(g, position, index, fraction);
          s_pos[o] = position; s_frac[o] = fraction; s_ti[o] = index | (src << 16) | ((uint32_t)(g.window_mode & (PG_GRAIN_WINDOWS - 1)) << 24);
        } else s_ti[o] = PG_GRAIN_INACTIVE;
      }
    }
    {  // the live slots in ascending order (slots 0..63 sit in wave 0, 64..99 in wave 1)
      const unsigned long long m = __ballot(live);
      if (lane == 0 && wave < 2) s_wcnt[wave] = __popcll(m);
      __syncthreads();
      if (live) s_live[__popcll(m & ((1ull << lane) - 1ull)) + (wave == 1 ? s_wcnt[0] : 0)] = tid;
    }
    __syncthreads();
    const int n_live = s_wcnt[0] + s_wcnt[1];
    // ---- phase 3: (slot, frame) pairs over all lanes ----
    for (int i = tid; i < n_live * GT; i += 256) {
      const int f = i % GT;
      if (f >= tn) continue;
      const int slot = s_live[i / GT];
      const int o = slot * GT + f;
      const uint32_t w = s_ti[o];
      float l = 0.0f, r = 0.0f;
      if (w != PG_GRAIN_INACTIVE) {
        const uint32_t a = (w >> 16) & 0xff;
        const float vol = a ? s_act[a - 1].volume : s_vol[slot], pan = a ? s_act[a - 1].panning : s_pan[slot];
        const uint32_t index = w & (PG_GRAIN_LUT_N - 1);
        const int mode = (int)((w >> 24) & (PG_GRAIN_WINDOWS - 1));
        const float env = mode == window ? grain_window_value(s_lut, index, s_frac[o]) : grain_window_value(L.lut + mode * PG_GRAIN_LUT_N, index, s_frac[o]);
        grain_term(env, pcm, len, s_pos[o], vol, pan, l, r);
      }
      s_pos[o] = l; s_frac[o] = r;
    }
    __syncthreads();
    if (tid < 2 * tn) {
      const int f = tid >> 1;
      const float* const terms = (tid & 1) ? s_frac : s_pos;
      float acc = 0.0f;
      for (int k = 0; k < n_live; ++k) acc += terms[s_live[k] * GT + f];
      staged[(size_t)(base + (uint32_t)f) * 2 + (tid & 1)] = acc;
    }
    __syncthreads();
  }
  if (tid < PG_GRAIN_POOL) V->grains[tid] = g;
  if (tid == 0) { V->params = S.p; V->pool = S.pool; V->stop_time = stop_time; V->exhausted_at = exhausted_at; V->stage_pos = L.chunk_t0; }
  if (has_mod) {  // (the last tile's barriers are behind every lane)
    if (tid < PG_GMOD_SOURCES * PG_GMOD_TARGETS) { (&V->mod.amount[0][0])[tid] = (&s_ramt[0][0])[tid]; (&V->mod.bipolar[0][0])[tid] = (&s_rbip[0][0])[tid]; }
    if (tid == 64 || tid == 128) V->mod.lfo[(tid >> 6) - 1] = s_lfo_state[(tid >> 6) - 1];
  }
}

hipError_t pg_launch_grain(const PgGrainLaunch& L, hipStream_t stream) {
  if (L.n_live == 0 || L.n == 0) return hipSuccess;
  hipLaunchKernelGGL(pg_grain_kernel, dim3(L.n_live), dim3(256), 0, stream, L);
  return hipGetLastError();
}

// GRAIN_WINDOW_LUT (granular.rs:221): [PG_GRAIN_WINDOWS][PG_GRAIN_LUT_N]
void pg_grain_build_lut(float* out) {
  for (int i = 0; i < PG_GRAIN_LUT_N; ++i) {
    float e[PG_GRAIN_WINDOWS];
    grain_window_entry(i, e);
    for (int w = 0; w < PG_GRAIN_WINDOWS; ++w) out[w * PG_GRAIN_LUT_N + i] = e[w];
  }
}
