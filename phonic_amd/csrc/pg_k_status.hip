// Playback status events on the device: PlaybackStatusEvent::Position and ::Stopped (src/source/status.rs) as every file source and every
// sampler voice of the reference sends them — FileSourceImpl::send_playback_position_status / send_playback_stopped_status
// (src/source/file/common.rs:171-221) from PreloadedFileSource::write / stop / kill (src/source/file/preloaded.rs:196-239, :396-475) and from
// SamplerVoice::process (src/generator/sampler/voice.rs:434-467, :488-502). The reference decides them once per Source::write call, from state
// the device holds at exactly that grid, so the records are decided here: pg_playback_status_kernel, one lane per voice that reports, behind
// every launch that can end a source write of such a voice — each piece of each chunk, level by level (a graph with a voice that reports
// leaves the super-block launches). It keeps a small record per voice (PgStatVoice, pg_dev.h): the emit clock, the voice as the launch before
// left it, the source write in progress.
//
// Two ways to learn what a launch's source writes left:
//   a launch of the time-parallel kernels holds ONE segment per unit: one source write of the voice, or a part of one — PgVoice holds what
//     it left — or, where the voice's stop time lies inside the launch, the write that returns there and the one that begins there with the
//     Stop message: every kernel's voice_process leaves playback_pos behind the first in PgVoice::stop_pos_lo / _hi (that write is neither at
//     the end of its file nor finished: a source that ends stops the walk and the stop stays pending), PgVoice holds what the second left. The
//     kernel restates voice_process's walk for that one segment (pg_source_dev.h) to know WHEN the writes began and whether the last one ends
//     with this launch;
//   the exact kernel renders chunks cut by events and stop times inside a piece — several source writes per launch: it logs every write that
//     returns (PgStatVoice::log) and stamps the record with the launch's round; the kernel here takes the log instead.
// Records go to fixed slots in mapped host memory, a job's count behind them: no atomics, a deterministic order; the host compacts the slots
// after the call (pg_status_host.h). Plain vector stores only.
#include "pg_host_internal.h"

struct PgStatLaunch {
  PgStatJob* jobs;             // mapped host memory: this launch's jobs
  pg_status_event* slots;      // mapped host memory: slot 0 of the table the jobs' slot0 count from
  PgStatVoice* recs;
  const PgVoice* voices;
  uint32_t n_recs;
  int32_t n_jobs;
};

__global__ void __launch_bounds__(64) pg_playback_status_kernel(PgStatLaunch L) {
  const int j = (int)(blockIdx.x * 64u + threadIdx.x);
  if (j >= L.n_jobs) return;
  PgStatJob* const job = L.jobs + j;
  const int rec = job->rec;
  int count = 0, lost = 0;
  if (rec >= 0 && (uint32_t)rec < L.n_recs) {
    PgStatVoice& sv = L.recs[rec];
    const PgVoice& v = L.voices[sv.voice];
    pg_status_event* const out = L.slots + job->slot0;
    const int n_slots = job->n_slots;
    const bool granular = (sv.flags & PG_SV_GRANULAR) != 0;
    auto put = [&](int kind, uint64_t time, uint64_t frame_pos, double seconds, int exhausted) {
      if (count < n_slots) {
        pg_status_event e;
        e.kind = kind; e.voice_id = sv.voice_id; e.sample_time = time; e.frame_pos = frame_pos; e.position_seconds = seconds; e.exhausted = exhausted; e.reserved = 0;
        out[count] = e;
        count += 1;
      } else lost += 1;
    };
    // FileSourceImpl::send_playback_position_status (common.rs:183-208): should_report_pos, the clock's reset, frame and second position
    auto position = [&](uint64_t time, uint64_t sample_pos, bool is_start_event) {
      if (!(sv.flags & PG_SV_POSITION)) return;
      const uint64_t elapsed = time > sv.clock_start ? time - sv.clock_start : 0;   // SampleTimeClock::elapsed: saturating_sub (time.rs:46-50)
      if (!(is_start_event || elapsed >= sv.emit_rate)) return;
      sv.clock_start = time;
      const uint64_t frame_pos = sample_pos / (uint64_t)(sv.channels ? sv.channels : 1u);
      put(PG_STATUS_POSITION, time, frame_pos, (double)frame_pos / (double)sv.rate, 0);
    };
    auto stopped = [&](uint64_t time, int exhausted) {
      if (sv.flags & PG_SV_STOPPED) put(PG_STATUS_STOPPED, time, 0, 0.0, exhausted);
    };
    // one Source::write call of the voice that has returned
    auto source_write = [&](uint64_t w_time, uint64_t w_pos, int w_flags) {
      if (w_flags & PG_SW_SKIPPED) return;                                                             // preloaded.rs:400-403
      if (w_flags & PG_SW_KILLED) { stopped(w_time, (w_flags & PG_SW_EOF_BEFORE) ? 1 : 0); return; }   // :196-208, then :400-403
      bool is_start_event = false;
      if (granular) { is_start_event = (sv.flags & PG_SV_STARTED) != 0; sv.flags &= ~PG_SV_STARTED; }  // voice.rs:456-457
      position(w_time, w_pos, is_start_event);                                                         // preloaded.rs:454-462 / voice.rs:448-467
      if (w_flags & PG_SW_FINISHED) {
        if (granular) {
          // voice.rs:488-502: reset() -> PreloadedFileSource::kill — the file source of a granular voice never played: exhausted = pos_eof = false —
          // then { exhausted: pool.is_exhausted() } behind GrainPool::reset, which has set trigger_new_grains (granular.rs:442-444, :495-502): false
          stopped(w_time, 0);
          stopped(w_time, 0);
        } else stopped(w_time, (w_flags & PG_SW_EOF) ? 1 : 0);                                         // preloaded.rs:464-472; voice.rs:488-495 -> :212-239
      }
    };
    if (sv.log_round == job->round) {
      // the exact kernel rendered the voice's unit in this launch: its log holds every source write that returned there, in order
      const int n = sv.n_log < PG_STAT_LOG ? sv.n_log : PG_STAT_LOG;
      for (int i = 0; i < n; ++i) source_write(sv.log[i].time, sv.log[i].pos, sv.log[i].flags);
      lost += sv.lost;
    } else {
      // a time-parallel kernel rendered it: voice_process for one segment [p0, p1) of a chunk that ends at c1
      const uint64_t p0 = job->t0, p1 = p0 + (uint64_t)job->n, c1 = job->chunk_end;
      const bool first = job->first != 0;
      if (sv.prev_active && !(sv.prev_chunk_skip && !first)) {
        uint64_t t = p0;
        bool runs = true;
        if (v.start_time > p0) { if (v.start_time >= p1) runs = false; else t = v.start_time; }
        if (runs) {
          const bool pending = sv.prev_has_stop && sv.prev_stop_time <= t;
          if (!sv.open) {
            const bool killed = pending && !sv.prev_finished && !granular && !(v.fade_out_seconds > 0.0f);
            sv.open = 1; sv.open_time = t;
            sv.open_flags = (sv.prev_finished ? PG_SW_SKIPPED : 0) | (killed ? PG_SW_KILLED : 0) | (sv.prev_pos_eof ? PG_SW_EOF_BEFORE : 0);
          }
          // The write reached the voice's stop time inside this launch (has_stop is consumed there, mixed.rs:584-603): it returned at the stop
          // time, and the next one began there with the Stop message — a fade-out, or Stopped at once (preloaded.rs:196-208)
          const bool cut = sv.prev_has_stop && !pending && sv.prev_stop_time < p1 && !v.has_stop;
          if (cut) {
            source_write(sv.open_time, (uint64_t)v.stop_pos_lo | ((uint64_t)v.stop_pos_hi << 32), sv.open_flags);
            sv.open_time = sv.prev_stop_time;
            sv.open_flags = (!granular && !(v.fade_out_seconds > 0.0f)) ? PG_SW_KILLED : 0;
          }
          // the call returns with this launch: the chunk ends, the stop time is its end, or the source has ended
          const bool ask_ends = p1 >= c1 || (sv.prev_has_stop && !pending && !cut && sv.prev_stop_time <= p1);
          if (ask_ends || v.finished) {
            source_write(sv.open_time, v.playback_pos, sv.open_flags | (v.pos_eof ? PG_SW_EOF : 0) | (v.finished ? PG_SW_FINISHED : 0));
            sv.open = 0;
          }
        }
      }
    }
    sv.n_log = 0; sv.lost = 0;
    // the voice as the next launch's source write finds it
    sv.prev_active = v.active; sv.prev_finished = v.finished; sv.prev_has_stop = v.has_stop; sv.prev_pos_eof = v.pos_eof; sv.prev_chunk_skip = v.chunk_skip;
    sv.prev_stop_time = v.stop_time;
  }
  job->lost = lost;
  __threadfence_system();   // the records and `lost` are out before the count says so
  job->count = count;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static int pstat_tables_reserve(pg_graph* g, size_t n_voices) {
  PstatState& s = g->pstat;
  const size_t pieces = (PG_MAX_FRAMES + g->max_frames - 1) / g->max_frames;
  const size_t hj = std::max<size_t>(1024, next_pow2(2 * std::max<size_t>(n_voices, 1) * pieces)), hs = 4 * hj;
  if (s.h_jobs && hj <= s.half_jobs) return PG_OK;
  if (s.h_jobs) (void)pg_host_free(s.h_jobs);
  if (s.h_slots) (void)pg_host_free(s.h_slots);
  s.h_jobs = nullptr; s.h_slots = nullptr; s.half_jobs = s.half_slots = 0;
  HIP_TRY(pg_host_malloc((void**)&s.h_jobs, 2 * hj * sizeof(PgStatJob), hipHostMallocMapped));
  HIP_TRY(pg_host_malloc((void**)&s.h_slots, 2 * hs * sizeof(pg_status_event), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void**)&s.d_jobs, s.h_jobs, 0));
  HIP_TRY(hipHostGetDevicePointer((void**)&s.d_slots, s.h_slots, 0));
  for (int i = 0; i < 2; ++i) { if (!s.ev[i]) HIP_TRY(hipEventCreateWithFlags(&s.ev[i], hipEventDisableTiming)); s.in_flight[i] = false; }   // (the caller drained the streams and collected)
  s.half_jobs = hj; s.half_slots = hs; s.turn = 0; s.nj = s.ns = 0;
  s.pending.clear(); s.pending_head = 0;
  s.pending.reserve(2 * hj + 16);
  s.gather.reserve(2 * hs);
  s.walk.reserve(std::max<size_t>(n_voices, 64));
  return PG_OK;
}

void graph_pstat_release(pg_graph* g) {
  PstatState& s = g->pstat;
  if (s.h_jobs) (void)pg_host_free(s.h_jobs);
  if (s.h_slots) (void)pg_host_free(s.h_slots);
  for (int i = 0; i < 2; ++i) if (s.ev[i]) (void)hipEventDestroy(s.ev[i]);
  if (s.d_recs) (void)pg_free(s.d_recs);
  if (s.d_of_voice) (void)pg_free(s.d_of_voice);
  s.h_jobs = nullptr; s.h_slots = nullptr; s.d_recs = nullptr; s.d_of_voice = nullptr;
}

// Completed chunks -> the ring, oldest first. A chunk's launches are taken together (their records are ordered over the whole chunk) once the
// last of them has been issued and every job's count is there. Reads mapped host memory: no wait unless `wait` asks for one.
void graph_pstat_collect(pg_graph* g, bool wait) {
  PstatState& s = g->pstat;
  if (!s.on) return;
  if (wait && s.pending_head < s.pending.size()) {
    (void)hipSetDevice(g->device);
    (void)pg_stream_sync(g->stream);
    if (g->last_stream && g->last_stream != g->stream) (void)pg_stream_sync(g->last_stream);
  }
  while (s.pending_head < s.pending.size()) {
    size_t end = s.pending_head;
    while (end < s.pending.size() && !s.pending[end].closes) ++end;
    if (end == s.pending.size()) break;   // the chunk is still being issued
    bool done = true;
    for (size_t i = s.pending_head; i <= end && done; ++i) done = pgs::status_jobs_done(s.h_jobs + s.pending[i].job0, s.pending[i].n_jobs);
    if (!done) break;
    std::atomic_thread_fence(std::memory_order_acquire);
    s.gather.clear();
    uint64_t lost = 0;
    for (size_t i = s.pending_head; i <= end; ++i) {
      const PstatLaunch& pl = s.pending[i];
      const size_t half = pl.job0 / s.half_jobs;
      pgs::status_gather(s.h_jobs + pl.job0, pl.n_jobs, s.h_slots + half * s.half_slots, s.gather, lost);
    }
    pgs::status_sort(s.gather);
    pgs::status_flush(s.gather, s.ring);
    s.ring.dropped += lost;
    s.pending_head = end + 1;
  }
  if (s.pending_head == s.pending.size()) { s.pending.clear(); s.pending_head = 0; }
}

// The voices that report, in the order the reference's write reaches them: a mixer's sub-mixers first, in the order they were added, then its
// sources in playing order (process_sub_mixers, process_sources: mixed.rs:505-620).
static void pstat_walk(pg_graph* g, int m, int top, int max_depth, uint32_t& rank) {
  PstatState& s = g->pstat;
  const HostMixer& mx = g->mixers[m];
  if (m == 0) { for (size_t c = 1; c < g->mixers.size(); ++c) if (g->mixers[c].parent == 0 && !g->mixers[c].removed) pstat_walk(g, (int)c, (int)c, max_depth, rank); }
  else for (int c : mx.children) if (!g->mixers[c].removed) pstat_walk(g, c, top, max_depth, rank);
  for (int v : mx.voices) {
    const HostVoice& hv = g->voices[v];
    if (hv.pstat >= 0 && hv.pstat_on && hv.mixer == m) {
      PstatState::Walk w;
      w.voice = v; w.rank = rank; w.top = top;
      w.level = m == 0 ? max_depth - 1 : max_depth - mx.depth;   // the levels run deepest first; the main mixer's sources ride with its sub-mixers (rebuild_topology)
      w.unit = m == 0 ? g->source_unit_of_voice[v] : mx.unit_slot;
      s.walk.push_back(w);
    }
    rank += 1;
  }
}
static int pstat_cmds_of(const std::vector<std::pair<int, int>>& unit_cmds, int unit) {
  auto it = std::lower_bound(unit_cmds.begin(), unit_cmds.end(), std::make_pair(unit, 0));
  return it != unit_cmds.end() && it->first == unit ? it->second : 0;
}
// Records a job may have to place: a source write sends a Position and a Stopped at most (a granular voice: two Stopped, voice.rs:488-502); a
// launch without commands for the voice's unit holds one source write that returns, one with c commands c + 2 at most (a segment per command, a
// stop time), and the exact kernel logs PG_STAT_LOG of them.
static int pstat_job_slots(int unit_cmds, bool min_slots) { return 3 * ((unit_cmds > 0 && !min_slots) ? std::min(PG_STAT_LOG, unit_cmds + 2) : 1); }

int graph_pstat_begin_chunk(pg_graph* g, const std::vector<std::vector<std::pair<int, int>>>& piece_cmds, hipStream_t stream) {
  PstatState& s = g->pstat;
  s.walk.clear();
  s.chunk_jobs_left = s.chunk_slots_left = 0;
  if (!s.on || !s.h_jobs) return PG_OK;
  uint32_t rank = 0;
  pstat_walk(g, 0, 0, (int)g->levels.size(), rank);
  if (s.walk.empty()) return PG_OK;
  size_t need_jobs = 0, need_slots = 0;
  s.chunk_min_slots = false;
  for (const auto& pc : piece_cmds) for (const PstatState::Walk& w : s.walk) { need_jobs += 1; need_slots += (size_t)pstat_job_slots(pstat_cmds_of(pc, w.unit), false); }
  if (need_slots > s.half_slots) { s.chunk_min_slots = true; need_slots = 3 * need_jobs; }   // (many voices on a unit that takes many commands in one piece)
  if (need_jobs > s.half_jobs || need_slots > s.half_slots) return set_error(PG_ERR_STATE, "playback status tables were not reserved by the mutating call");
  if (s.nj + need_jobs > s.half_jobs || s.ns + need_slots > s.half_slots) {
    // the other half: once the event behind its last launch has passed, every chunk in it is complete — into the ring with them
    (void)hipSetDevice(g->device);
    HIP_TRY(hipEventRecord(s.ev[s.turn], stream));
    s.in_flight[s.turn] = true;
    s.turn ^= 1;
    if (s.in_flight[s.turn] && hipEventQuery(s.ev[s.turn]) != hipSuccess) HIP_TRY(hipEventSynchronize(s.ev[s.turn]));
    s.in_flight[s.turn] = false;
    graph_pstat_collect(g, false);
    for (size_t i = s.pending_head; i < s.pending.size(); ++i)
      if (s.pending[i].job0 / s.half_jobs == (size_t)s.turn) return set_error(PG_ERR_STATE, "playback status launch tables: a launch of the half to be reused has not been collected");
    s.nj = s.ns = 0;
  }
  s.chunk_jobs_left = need_jobs; s.chunk_slots_left = need_slots;
  return PG_OK;
}

int graph_pstat_launch(pg_graph* g, size_t li, uint64_t t0, uint32_t n, bool first, uint64_t chunk_end, uint32_t round, const std::vector<std::pair<int, int>>& unit_cmds, hipStream_t stream) {
  PstatState& s = g->pstat;
  if (s.walk.empty() || s.chunk_jobs_left == 0) return PG_OK;
  const size_t j0 = (size_t)s.turn * s.half_jobs + s.nj;
  size_t nj = 0, ns = 0;
  for (const PstatState::Walk& w : s.walk) {
    if ((size_t)w.level != li) continue;
    const int slots = pstat_job_slots(pstat_cmds_of(unit_cmds, w.unit), s.chunk_min_slots);
    if (nj + 1 > s.chunk_jobs_left || ns + (size_t)slots > s.chunk_slots_left) return set_error(PG_ERR_STATE, "playback status launch tables: the chunk's reservation is used up");
    PgStatJob job;
    memset(&job, 0, sizeof job);
    job.rec = g->voices[w.voice].pstat;
    job.slot0 = (int32_t)(s.ns + ns); job.n_slots = slots;
    job.count = -1; job.lost = 0;
    job.round = round; job.t0 = t0; job.n = n; job.first = first ? 1 : 0; job.chunk_end = chunk_end;
    job.rank = w.rank; job.top = w.top;
    s.h_jobs[j0 + nj] = job;
    nj += 1; ns += (size_t)slots;
  }
  if (nj == 0) return PG_OK;
  s.nj += nj; s.ns += ns; s.chunk_jobs_left -= nj; s.chunk_slots_left -= ns;
  PgStatLaunch L;
  L.jobs = s.d_jobs + j0; L.slots = s.d_slots + (size_t)s.turn * s.half_slots;
  L.recs = s.d_recs; L.voices = g->d_voices.d; L.n_recs = (uint32_t)s.n_recs; L.n_jobs = (int32_t)nj;
  hipLaunchKernelGGL(pg_playback_status_kernel, dim3((unsigned)((nj + 63) / 64)), dim3(64), 0, stream, L);
  HIP_TRY(hipGetLastError());
  PstatLaunch pl;
  pl.job0 = j0; pl.n_jobs = nj; pl.closes = false;
  s.pending.push_back(pl);
  return PG_OK;
}

void graph_pstat_end_chunk(pg_graph* g) {
  PstatState& s = g->pstat;
  if (!s.pending.empty() && s.pending_head < s.pending.size()) s.pending.back().closes = true;
  s.chunk_jobs_left = s.chunk_slots_left = 0;
}

extern "C" {

int pg_graph_enable_status(pg_graph* g, size_t capacity_events) {
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (capacity_events == 0) return set_error(PG_ERR_PARAMETER, "the status ring needs room for one record at least");
  if (g->pstat.on) return set_error(PG_ERR_STATE, "playback status is enabled already");
  if (g->write_count > 0) return set_error(PG_ERR_STATE, "playback status is enabled before the first write");
  if (graph_quiesce(g)) return graph_fail(g, PG_ERR_DEVICE);
  (void)hipSetDevice(g->device);
  g->pstat.ring.reset(capacity_events);
  // the side table the exact kernel reaches the voices' records through, and the launch tables
  if (graph_env_reserve(g, std::max<size_t>(g->voices.size(), 1))) return graph_fail(g, PG_ERR_DEVICE);
  { const int rc = pstat_tables_reserve(g, 64); if (rc) return graph_fail(g, rc); }
  g->pstat.on = true;
  return PG_OK;
}

int pg_graph_set_voice_status(pg_graph* g, int voice_id, double position_emit_seconds, int report_stopped) {
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (std::isnan(position_emit_seconds)) return set_error(PG_ERR_PARAMETER, "Invalid position emit rate: %g", position_emit_seconds);
  const VoiceKind kind = voice_kind(g, voice_id);
  if (kind == VOICE_DEAD) return set_error(PG_ERR_NOT_FOUND, "Source with id %d not found", voice_id);
  if (!g->pstat.on) return set_error(PG_ERR_STATE, "playback status is not enabled on this graph (pg_graph_enable_status)");
  drain_control_messages(g);
  if (g->voices[voice_id].mixer < 0) return set_error(PG_ERR_NOT_FOUND, "Source with id %d not found", voice_id);
  HostVoice& hv = g->voices[voice_id];
  if (kind == VOICE_HOST_FED || hv.stream) return set_error(PG_ERR_PARAMETER, "Source with id %d is fed by the host: its playback status is the host's", voice_id);
  if (hv.outer) return set_error(PG_ERR_PARAMETER, "Source with id %d runs at a rate of its own behind a resampler: playback status is not supported there", voice_id);
  if (voice_has_rendered(g, hv)) return set_error(PG_ERR_STATE, "Source with id %d has rendered frames already: playback status is set before the voice starts", voice_id);
  if (graph_quiesce(g)) return graph_fail(g, PG_ERR_DEVICE);
  graph_pstat_collect(g, false);   // (quiescent: everything issued is complete — the launch tables may move)
  (void)hipSetDevice(g->device);
  PstatState& s = g->pstat;
  if (graph_env_reserve(g, std::max<size_t>(g->voices.size(), (size_t)hv.dev_index + 1))) return graph_fail(g, PG_ERR_DEVICE);
  const bool fresh = hv.pstat < 0;
  if (fresh && s.n_recs + 1 > s.cap_recs) {  // grow by doubling; the records live on
    const size_t cap = std::max<size_t>(64, s.cap_recs * 2);
    PgStatVoice* nd = nullptr;
    HIP_TRY(pg_malloc((void**)&nd, cap * sizeof(PgStatVoice)));
    if (pg_memset(nd, 0, cap * sizeof(PgStatVoice)) != hipSuccess ||
        (s.n_recs && pg_memcpy(nd, s.d_recs, s.n_recs * sizeof(PgStatVoice), hipMemcpyDeviceToDevice) != hipSuccess)) { (void)pg_free(nd); return graph_fail(g, set_error(PG_ERR_DEVICE, "status record allocation failed")); }
    if (s.d_recs) (void)pg_free(s.d_recs);
    s.d_recs = nd; s.cap_recs = cap;
  }
  const int rec = fresh ? (int)s.n_recs : hv.pstat;
  const bool granular = voice_kind_is_granular(kind);
  std::unique_ptr<PgStatVoice> r(new PgStatVoice);
  memset(r.get(), 0, sizeof(PgStatVoice));
  r->voice = hv.dev_index; r->voice_id = voice_id;
  r->flags = (position_emit_seconds > 0.0 ? PG_SV_POSITION : 0) | (report_stopped ? PG_SV_STOPPED : 0) | (granular ? (PG_SV_GRANULAR | PG_SV_STARTED) : 0);
  r->log_round = 0xffffffffu;   // (no launch carries this round before 2^32 - 1 others have)
  r->emit_rate = position_emit_seconds > 0.0 ? pgs::status_emit_rate_frames(position_emit_seconds, g->sample_rate) : 0;
  r->clock_start = 0;           // SampleTimeClock::new (time.rs:19-26)
  r->channels = hv.file_channels ? hv.file_channels : 1; r->rate = hv.file_rate ? hv.file_rate : g->sample_rate; r->buffer_len = hv.file_samples;
  // what the voice's first source write will find: a source the mixer holds, not finished; a stop that was sent for it already
  r->prev_active = 1; r->prev_has_stop = hv.stop_time != UINT64_MAX ? 1 : 0; r->prev_stop_time = hv.stop_time != UINT64_MAX ? hv.stop_time : 0;
  HIP_TRY(pg_memcpy(s.d_recs + rec, r.get(), sizeof(PgStatVoice), hipMemcpyHostToDevice));
  const int32_t rec32 = (r->flags & (PG_SV_POSITION | PG_SV_STOPPED)) ? (int32_t)rec : -1;   // (both off: the voice reports nothing — the exact kernel leaves it alone)
  HIP_TRY(pg_memcpy(s.d_of_voice + hv.dev_index, &rec32, sizeof rec32, hipMemcpyHostToDevice));
  if (fresh) { s.n_recs += 1; s.voices.push_back(voice_id); }
  hv.pstat = rec; hv.pstat_on = rec32 >= 0;
  if (granular && hv.gran >= 0) {  // the grain engine leaves the playhead behind every frame for a voice that reports its position
    if ((r->flags & PG_SV_POSITION) && !hv.d_trace) {
      HIP_TRY(pg_malloc((void**)&hv.d_trace, (size_t)PG_MAX_FRAMES * sizeof(float)));
      HIP_TRY(pg_memset(hv.d_trace, 0, (size_t)PG_MAX_FRAMES * sizeof(float)));
    }
    float* const trace = (r->flags & PG_SV_POSITION) ? hv.d_trace : nullptr;
    HIP_TRY(pg_memcpy((char*)(g->d_gran + hv.gran) + offsetof(PgGrainVoice, pos_trace), &trace, sizeof trace, hipMemcpyHostToDevice));
  }
  { const int rc = graph_env_head_refresh(g); if (rc) return graph_fail(g, rc); }
  { const int rc = pstat_tables_reserve(g, s.voices.size()); if (rc) return graph_fail(g, rc); }
  return PG_OK;
}

int pg_graph_poll_status(pg_graph* g, pg_status_event* out, size_t max_events) {
  if (!g || !g->pstat.on || (!out && max_events)) return 0;
  graph_pstat_collect(g, false);
  return (int)g->pstat.ring.poll(out, std::min<size_t>(max_events, 0x7fffffffu));
}

uint64_t pg_graph_status_dropped(pg_graph* g) {
  if (!g || !g->pstat.on) return 0;
  graph_pstat_collect(g, false);
  return g->pstat.ring.dropped;
}

}  // extern "C"
