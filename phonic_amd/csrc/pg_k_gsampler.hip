// pg_gsampler_kernel: the note layer of the granular-mode samplers (pg_graph_add_granular_sampler; Sampler::with_granular_playback,
// src/generator/sampler.rs:598-637) — one workgroup per living sampler, launched on the write's stream BETWEEN the pg_grain_kernel launches of
// consecutive spans of the samplers' source-write grid:
//     close span k-1  ->  apply the messages due at span k's first frame  ->  pg_grain_kernel over span k  ...  -> close the chunk's last span
// Which slot a note gets depends on which slots are active and which release at exactly the note's frame. A granular slot stops being active in
// the SamplerVoice::process call in which its pool became exhausted or its envelope went Idle (voice.rs:488-502), that is at the END of the
// Sampler::write that rendered that frame — and the ends of those writes are the cuts of the owning mixer chain (mixed.rs:679-712). A slot that
// has run dry keeps its scheduler, and so its generator, running until that end, and the pool's reset does not reseed: the ends have to be taken
// on the reference's grid, not where a message happens to arrive.
// The host issues one launch per boundary of ANY sampler's grid (pg_sampler.hip: launch_gsampler_spans); the workgroup of a sampler whose mixer
// has no cut there returns at once: the boundary is the sampler's own iff the chunk begins there, its start time lies there, or a command of its
// unit — an event of the mixer, a call boundary of an ancestor (CMD_CALL_SPLIT) — stands at that frame of the piece's command list. A sampler on
// the MAIN mixer (pg_graph_add_granular_sampler_to_main) has its own source unit in note.unit: its messages are events of the main mixer, each
// begins a chunk, so its boundaries are the chunk's first frame and its start time.
// The arithmetic is pg_gsampler_dev.h's.
#include "pg_host_internal.h"
#include "pg_gsampler_dev.h"

using namespace pgd;

__global__ void __launch_bounds__(256) pg_gsampler_kernel(PgGSamplerLaunch L) {
  __shared__ GsShared S;
  const int tid = (int)threadIdx.x;
  if (blockIdx.x >= L.n_live) return;
  const int rec = L.live[blockIdx.x];
  if (rec < 0 || (uint32_t)rec >= L.n_recs) return;
  PgGSampler& r = L.recs[rec];
  if (!gs_pool_ok(L, r)) return;
  int boundary = (L.closing || L.chunk_first || L.t == r.start_time) ? 1 : 0;
  if (!boundary) {
    int hit = 0;
    for (int i = tid; i < L.n_cmds; i += 256) {
      const PgCmd c = L.cmds[i];
      hit |= (c.unit == r.note.unit && c.frame == L.frame && c.type != CMD_CHUNK_END && c.type != CMD_CALL_END) ? 1 : 0;
    }
    boundary = __syncthreads_or(hit);
  }
  if (!boundary) return;
  const uint64_t span_t0 = r.span_t0;
  __syncthreads();
  if (span_t0 != PG_USIZE_MAX && span_t0 < L.t) gs_close(L, r, span_t0, L.t, S);
  const bool opens = !L.closing && L.t >= r.start_time;   // (the mixer does not call the sampler before its start time, mixed.rs:565-576)
  if (opens && !r.note.stopped) gs_open(L, r, S);          // (a stopped sampler returns empty-handed: sampler.rs:978-981)
  if (!L.closing) {   // what the write that begins here returns (PgGSampler::delivers), the messages of its first frame applied
    __syncthreads();
    const int any_active = __syncthreads_or((tid < r.note.n_voices && r.active[tid] != 0) ? 1 : 0);
    if (tid == 0) r.delivers = (opens && !r.note.stopped && (any_active || r.note.stopping)) ? 1 : 0;
  }
  if (tid == 0) r.span_t0 = opens ? L.t : PG_USIZE_MAX;
}

hipError_t pg_launch_gsampler(const PgGSamplerLaunch& L, hipStream_t stream) {
  if (L.n_live == 0) return hipSuccess;
  hipLaunchKernelGGL(pg_gsampler_kernel, dim3(L.n_live), dim3(256), 0, stream, L);
  return hipGetLastError();
}
