// pg_grain_kernel: the grain engine of the sampler's granular voices (GrainPool<100>, src/generator/sampler/granular.rs) — one workgroup per
// living granular voice, launched on the write's stream in front of the unit kernels of a chunk's piece. It renders the voice's frames of the
// piece as interleaved stereo f32 into the voice's staging buffer; the exact unit kernel takes them as the voice's source output (a plain copy
// in its source stage, pg_source_dev.h) and puts the volume envelope on top. Commands of the piece (volume, panning, speed, stop, release) are
// read from the launch's command list and applied at their frames.
//
// Per tile of PG_GRAIN_TILE frames (pg_grain_dev.h has the arithmetic):
//   1  lane 0 walks the scheduler frame by frame and leaves the activations, one slot per frame at most, in LDS;
//   2  lane s walks slot s: takes its activations at their frames, steps Grain::process's f64 recurrences and leaves, per frame, the f32 read
//      position and the window table's index and fraction in LDS (12 bytes per slot and frame: 38 KB for 100 slots x 32 frames); the slot's
//      record stays in the lane's registers for the whole launch. Slots without an active grain in the tile are left out of what follows;
//   3  all lanes, spread over (active slot, frame): window lookup from the voice's table row in LDS, the four reads of the buffer, Catmull-Rom,
//      the threshold test, the two stereo terms — written over the slot's LDS words; then one lane per (frame, channel) adds the terms in
//      ascending slot order and stores the frame.
// State does not depend on how a render is cut into launches or tiles: every recurrence is walked frame by frame in the reference's order.
#include "pg_host_internal.h"
#include "pg_grain_dev.h"

using namespace pgd;

#define GT PG_GRAIN_TILE
#define GRAIN_CMD_CAP 64

__device__ __forceinline__ bool grain_cmd_matches(const PgCmd& c, int voice) {
  return c.target == voice && (c.type == CMD_VOICE_VOLUME || c.type == CMD_VOICE_PAN || c.type == CMD_VOICE_SPEED || c.type == CMD_VOICE_STOP || c.type == CMD_VOICE_RELEASE);
}

__global__ void __launch_bounds__(256) pg_grain_kernel(PgGrainLaunch L) {
  __shared__ float s_lut[PG_GRAIN_LUT_N];
  __shared__ float s_pos[PG_GRAIN_POOL * GT];     // phase 2: read position; phase 3: the left term
  __shared__ float s_frac[PG_GRAIN_POOL * GT];    // phase 2: window fraction; phase 3: the right term
  __shared__ uint32_t s_ti[PG_GRAIN_POOL * GT];   // window index | (1 + frame of the activation the grain's volume / panning come from, 0: the slot's as the tile began) << 16
  __shared__ GrainActivation s_act[GT];
  __shared__ int s_end[PG_GRAIN_POOL];
  __shared__ float s_vol[PG_GRAIN_POOL], s_pan[PG_GRAIN_POOL];
  __shared__ int s_touched[PG_GRAIN_POOL];
  __shared__ int s_live[PG_GRAIN_POOL];
  __shared__ int s_wcnt[2];
  __shared__ int s_cmd[GRAIN_CMD_CAP];
  __shared__ int s_ncmd;

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
  __syncthreads();

  for (uint32_t base = 0; base < L.n; base += GT) {
    const int tn = (int)(L.n - base < (uint32_t)GT ? L.n - base : (uint32_t)GT);
    const uint64_t tile_t = L.t0 + base;
    if (tid < PG_GRAIN_POOL) {
      s_end[tid] = g.active ? (int)(g.samples_remaining < 0x3fffffffull ? g.samples_remaining : 0x3fffffffull) : 0;
      s_vol[tid] = g.volume; s_pan[tid] = g.panning; s_touched[tid] = 0;
    }
    __syncthreads();
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
          else if (!has_env) S.pool.trigger_new_grains = 0;   // CMD_VOICE_RELEASE without an envelope: SamplerVoice::stop -> GrainPool::stop
        }
        if (t < start_time) { s_act[f].slot = -1; continue; }
        if (t >= stop_time) S.pool.trigger_new_grains = 0;
        GrainActivation a;
        grain_sched_frame(S, s_end, f, a);
        if (a.slot >= 0) { s_act[f] = a; s_touched[a.slot] = 1; }
        else s_act[f].slot = -1;
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
        if (s_act[f].slot == tid) { grain_take_activation(g, s_act[f], window); src = (uint32_t)(f + 1); }
        const int o = tid * GT + f;
        if (g.active) {
          float position, fraction;
          uint32_t index;
          grain_step(g, position, index, fraction);
          s_pos[o] = position; s_frac[o] = fraction; s_ti[o] = index | (src << 16);
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
        const uint32_t a = w >> 16;
        const float vol = a ? s_act[a - 1].volume : s_vol[slot], pan = a ? s_act[a - 1].panning : s_pan[slot];
        grain_term(s_lut, pcm, len, s_pos[o], w & (PG_GRAIN_LUT_N - 1), s_frac[o], vol, pan, l, r);
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
  if (tid == 0) { V->pool = S.pool; V->stop_time = stop_time; V->exhausted_at = exhausted_at; V->stage_pos = L.chunk_t0; }
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
