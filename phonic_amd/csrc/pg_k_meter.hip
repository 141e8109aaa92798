// Per-mixer peak / RMS level metering on the device: the reference wraps the main mixer and every sub-mixer in a MeteredSource
// (PlayerConfig::metering_interval, src/player.rs:162-217, :346-348, :784-786; src/source/mixed/submixer.rs:24) and hands the levels out
// through Player::audio_level / MixerHandle::audio_level (src/source/metered.rs). The samples a meter needs — the sub-mixers' rows of the
// per-unit output table — never leave the device, so the meter runs there: pg_meter_kernel, one workgroup per metered mixer, behind the
// work it reads, on the same stream, only while metering is on.
//
// One RECORD is one AudioLevelState::record call (metered.rs:104-143) = one write call of the wrapped mixer that returned samples:
//   main mixer   one per pg_graph_write* call, over the samples the call delivers (behind the bus effects), time = the call's position;
//   sub-mixer    one per chunk of its parent — the call of SubMixerProcessor::process (submixer.rs:47-77) in which its silence gate is
//                decided, over the same buffer (the unit's output row; a call the gate silences, 2 s below -60 dB, reads as zeros here) —
//                time = the chunk's start.
// The host describes a record as SPANS of device memory (a chunk rendered as pieces, a host write copied out part by part: several spans,
// the last one carries the publish check); the kernel keeps the accumulators per mixer in device memory and writes a published level to
// pinned host memory. The reference skips a record when its try_lock fails (metered.rs:196-204): here one kernel owns a mixer's state and a
// reader never blocks it, so no record is ever skipped.
#include "pg_host_internal.h"

struct PgMeterLaunch {
  const PgMeterJob* jobs;
  const PgMeterSpan* spans;
  PgMeterState* state;
  int32_t* seen_inactive;      // per voice (device index): the meter saw the source inactive behind an earlier record: the mixer has dropped it since
  const PgUnit* units;
  const PgVoice* voices;
  const int32_t* voice_index;
  uint64_t interval;           // update_interval in frames
};

// Each lane keeps an f32 maximum and an f64 sum of squares per channel; a record is reduced by a butterfly inside every wave and then over
// the four waves' words in LDS, in wave order, by lane 0: a fixed order, the same bits on every run. Squares of f32 values are exact in
// f64, so any order of n <= 2^22 such terms is within n * 2^-53 of the exact sum: the published RMS is within one f32 rounding of the
// reference's sequential sum; the maximum does not depend on the order at all.
__global__ void __launch_bounds__(256) pg_meter_kernel(PgMeterLaunch L) {
  __shared__ double red_sq[4][2];
  __shared__ float red_pk[4][2];
  const int tid = (int)threadIdx.x;
  const PgMeterJob job = L.jobs[blockIdx.x];
  // Was there a source in the mixer's list when the record's call began? A transient source that ran dry is marked inactive and dropped
  // when that call ends (mixed.rs:612-616, :715): it counts for the record in which the meter first sees it inactive, not after. (A
  // launch that holds several records of such a mixer — a parent that splits its chunk — decides the later ones on the state behind the
  // launch.)
  int first_written = 1, later_written = 1;
  if (!(job.flags & PG_METER_JOB_WRITTEN)) {
    const PgUnit& u = L.units[job.unit];
    int pre = 0, post = 0;
    for (int i = tid; i < u.n_voices; i += 256) {
      const int v = L.voice_index[u.voice_off + i];
      const int active = L.voices[v].active != 0;
      pre |= active | (L.seen_inactive[v] == 0);
      post |= active;
      L.seen_inactive[v] = active ? 0 : 1;
    }
    first_written = __syncthreads_or(pre);
    later_written = __syncthreads_or(post);
    if (!first_written && !later_written) return;
  }
  PgMeterState st = L.state[job.slot];   // (lane 0's copy is the one that counts)
  float pk0 = 0.0f, pk1 = 0.0f;
  double sq0 = 0.0, sq1 = 0.0;
  uint64_t rec_frames = 0;
  int rec = 0;
  for (int si = 0; si < job.span_count; ++si) {
    const PgMeterSpan sp = L.spans[job.span_first + si];
    const bool written = rec == 0 ? first_written != 0 : later_written != 0;
    if (written) {
      rec_frames += sp.n_frames;
      if (!(sp.flags & PG_METER_ZEROS)) {
        const float* p = job.base + sp.off;
        const int n = (int)sp.n_frames * 2;
        // scalar head up to the first 16-byte boundary, float4 body, scalar tail (rows start on frame boundaries: 8-byte aligned)
        int head = (int)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);
        if (head > n) head = n;
        const int n4 = (n - head) >> 2;
        const int tail0 = head + n4 * 4;
        if (tid < head) {
          const float a = fabsf(p[tid]);
          if (tid & 1) { if (a > pk1) pk1 = a; sq1 += (double)p[tid] * (double)p[tid]; }
          else { if (a > pk0) pk0 = a; sq0 += (double)p[tid] * (double)p[tid]; }
        }
        const float4* p4 = (const float4*)(p + head);
        const bool swap = (head & 1) != 0;   // which channel the vector's even elements belong to
        for (int j = tid; j < n4; j += 256) {
          const float4 v = p4[j];
          float e0 = v.x, o0 = v.y, e1 = v.z, o1 = v.w;
          if (swap) { e0 = v.y; o0 = v.x; e1 = v.w; o1 = v.z; }
          float a;
          a = fabsf(e0); if (a > pk0) pk0 = a;
          a = fabsf(e1); if (a > pk0) pk0 = a;
          a = fabsf(o0); if (a > pk1) pk1 = a;
          a = fabsf(o1); if (a > pk1) pk1 = a;
          sq0 += (double)e0 * (double)e0; sq0 += (double)e1 * (double)e1;
          sq1 += (double)o0 * (double)o0; sq1 += (double)o1 * (double)o1;
        }
        if (tail0 + tid < n) {
          const int i = tail0 + tid;
          const float a = fabsf(p[i]);
          if (i & 1) { if (a > pk1) pk1 = a; sq1 += (double)p[i] * (double)p[i]; }
          else { if (a > pk0) pk0 = a; sq0 += (double)p[i] * (double)p[i]; }
        }
      }
    }
    // the launch's last span may leave its record open (a host write copied out part by part: the next launch goes on with it): what the
    // lanes hold is folded into the mixer's state all the same — the accumulators are sums and maxima — only the publish check waits
    const bool ends = (sp.flags & PG_METER_END_OF_RECORD) != 0;
    if (!ends && si + 1 < job.span_count) continue;
    if (written) {
      for (int off = 32; off > 0; off >>= 1) {
        const float q0 = __shfl_xor(pk0, off, 64), q1 = __shfl_xor(pk1, off, 64);
        if (q0 > pk0) pk0 = q0;
        if (q1 > pk1) pk1 = q1;
        sq0 += __shfl_xor(sq0, off, 64);
        sq1 += __shfl_xor(sq1, off, 64);
      }
      __syncthreads();   // (the words of the record before have been read)
      if ((tid & 63) == 0) { red_pk[tid >> 6][0] = pk0; red_pk[tid >> 6][1] = pk1; red_sq[tid >> 6][0] = sq0; red_sq[tid >> 6][1] = sq1; }
      __syncthreads();
      if (tid == 0) {
        for (int c = 0; c < 2; ++c) {
          double s = red_sq[0][c];
          for (int w = 1; w < 4; ++w) s += red_sq[w][c];
          st.sum_square[c] += s;
          for (int w = 0; w < 4; ++w) if (red_pk[w][c] > st.peak_hold[c]) st.peak_hold[c] = red_pk[w][c];
        }
        st.collected_frames += rec_frames;
        const uint64_t elapsed = sp.time > st.clock_start ? sp.time - st.clock_start : 0;   // saturating_sub
        if (ends && elapsed >= L.interval) {
          float rms[2];
          for (int c = 0; c < 2; ++c) rms[c] = st.collected_frames > 0 ? (float)sqrt(st.sum_square[c] / (double)st.collected_frames) : 0.0f;
          volatile PgMeterPub* pub = job.pub;
          pub->seq = st.seq + 1;
          __threadfence_system();
          pub->peak[0] = st.peak_hold[0]; pub->peak[1] = st.peak_hold[1];
          pub->rms[0] = rms[0]; pub->rms[1] = rms[1];
          __threadfence_system();
          st.seq += 2;
          pub->seq = st.seq;
          st.clock_start = sp.time;
          st.collected_frames = 0;
          st.peak_hold[0] = st.peak_hold[1] = 0.0f;
          st.sum_square[0] = st.sum_square[1] = 0.0;
        }
      }
    }
    pk0 = pk1 = 0.0f; sq0 = sq1 = 0.0; rec_frames = 0;
    rec += 1;
  }
  if (tid == 0) { L.state[job.slot] = st; __threadfence_system(); }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static constexpr size_t METER_PUB_CHUNK = 1024;

// The launch tables: pinned host memory the kernel reads in place, two halves each. A half is refilled only once the event recorded behind
// the last launch that read it has passed (waited for in the rare case it has not): writes allocate nothing and do not block.
static int meter_ring_reserve(pg_graph* g, size_t jobs, size_t spans) {
  MeterRing& r = g->meter_ring;
  const size_t hj = std::max<size_t>(4096, next_pow2(4 * jobs)), hs = std::max<size_t>(4096, next_pow2(4 * spans));
  if (r.h_jobs && hj <= r.half_jobs && hs <= r.half_spans) return PG_OK;
  if (r.h_jobs) (void)pg_host_free(r.h_jobs);
  if (r.h_spans) (void)pg_host_free(r.h_spans);
  r.h_jobs = nullptr; r.h_spans = nullptr; r.half_jobs = r.half_spans = 0;
  HIP_TRY(pg_host_malloc((void**)&r.h_jobs, 2 * hj * sizeof(PgMeterJob), hipHostMallocMapped));
  HIP_TRY(pg_host_malloc((void**)&r.h_spans, 2 * hs * sizeof(PgMeterSpan), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void**)&r.d_jobs, r.h_jobs, 0));
  HIP_TRY(hipHostGetDevicePointer((void**)&r.d_spans, r.h_spans, 0));
  for (int i = 0; i < 2; ++i) { if (!r.ev[i]) HIP_TRY(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming)); r.in_flight[i] = false; }   // (the caller drained the streams)
  r.half_jobs = hj; r.half_spans = hs; r.turn = 0; r.nj = r.ns = 0;
  return PG_OK;
}

static int meter_pub_reserve(pg_graph* g, size_t n_mixers) {
  for (size_t c = 0; c * METER_PUB_CHUNK < n_mixers; ++c) {
    if (c >= PG_METER_PUB_CHUNKS) return set_error(PG_ERR_STATE, "too many mixers to meter");
    if (g->meter_pub[c].load(std::memory_order_relaxed)) continue;
    PgMeterPub* p = nullptr;
    HIP_TRY(pg_host_malloc((void**)&p, METER_PUB_CHUNK * sizeof(PgMeterPub), hipHostMallocMapped));
    memset(p, 0, METER_PUB_CHUNK * sizeof(PgMeterPub));
    PgMeterPub* d = nullptr;
    if (hipHostGetDevicePointer((void**)&d, p, 0) != hipSuccess) { (void)pg_host_free(p); return set_error(PG_ERR_DEVICE, "hipHostGetDevicePointer failed"); }
    g->meter_pub_dev[c] = d;
    g->meter_pub[c].store(p, std::memory_order_release);
  }
  return PG_OK;
}

// Everything metering needs for the graph as the host mirror describes it now (the graph is quiescent): state per mixer, the `seen
// inactive` word per voice, the published levels, the launch tables. New entries are AudioLevelState::new: zero.
int graph_meter_reserve(pg_graph* g) {
  if (!g->metering) return PG_OK;
  (void)hipSetDevice(g->device);
  const size_t n_mixers = g->mixers.size(), n_voices = std::max<size_t>(g->voices.size(), 1);
  if (n_mixers > g->meter_cap) {
    const size_t cap = std::max<size_t>(next_pow2(n_mixers), 64);
    PgMeterState* nd = nullptr;
    HIP_TRY(pg_malloc((void**)&nd, cap * sizeof(PgMeterState)));
    HIP_TRY(pg_memset(nd, 0, cap * sizeof(PgMeterState)));
    if (g->d_meter_state) { HIP_TRY(pg_memcpy(nd, g->d_meter_state, g->meter_cap * sizeof(PgMeterState), hipMemcpyDeviceToDevice)); (void)pg_free(g->d_meter_state); }
    g->d_meter_state = nd; g->meter_cap = cap;
  }
  if (n_voices > g->meter_seen_cap) {
    const size_t cap = std::max<size_t>(next_pow2(n_voices), 256);
    int32_t* nd = nullptr;
    HIP_TRY(pg_malloc((void**)&nd, cap * sizeof(int32_t)));
    HIP_TRY(pg_memset(nd, 0, cap * sizeof(int32_t)));
    if (g->d_meter_seen) { HIP_TRY(pg_memcpy(nd, g->d_meter_seen, g->meter_seen_cap * sizeof(int32_t), hipMemcpyDeviceToDevice)); (void)pg_free(g->d_meter_seen); }
    g->d_meter_seen = nd; g->meter_seen_cap = cap;
  }
  { const int rc = meter_pub_reserve(g, n_mixers); if (rc) return rc; }
  // one launch: a job per mixer; the sub-mixers of the main mixer share one run of spans (a span per block of a launch sequence / piece of
  // a chunk), a nested one has its own, cut where an ancestor splits its chunk (at most PG_MAX_CALLS calls per chunk)
  size_t nested = 0;
  for (const HostMixer& mx : g->mixers) nested += mx.depth >= 2 ? 1 : 0;
  return meter_ring_reserve(g, n_mixers, (nested + 2) * (graph_table_blocks(g) + PG_MAX_CALLS + 2));
}

void graph_meter_release(pg_graph* g) {
  MeterRing& r = g->meter_ring;
  if (r.h_jobs) (void)pg_host_free(r.h_jobs);
  if (r.h_spans) (void)pg_host_free(r.h_spans);
  for (int i = 0; i < 2; ++i) if (r.ev[i]) (void)hipEventDestroy(r.ev[i]);
  if (g->d_meter_state) (void)pg_free(g->d_meter_state);
  if (g->d_meter_seen) (void)pg_free(g->d_meter_seen);
  for (size_t c = 0; c < PG_METER_PUB_CHUNKS; ++c) if (PgMeterPub* p = g->meter_pub[c].load()) (void)pg_host_free(p);
}

// One launch: g->meter_jobs / g->meter_spans (span_first relative to the list) -> a free region of the pinned tables -> pg_meter_kernel on `stream`.
int graph_meter_launch(pg_graph* g, hipStream_t stream) {
  const size_t nj = g->meter_jobs.size(), ns = g->meter_spans.size();
  if (nj == 0) return PG_OK;
  MeterRing& r = g->meter_ring;
  if (nj > r.half_jobs || ns > r.half_spans) return set_error(PG_ERR_STATE, "metering tables were not reserved by the mutating call");
  if (r.nj + nj > r.half_jobs || r.ns + ns > r.half_spans) {
    HIP_TRY(hipEventRecord(r.ev[r.turn], stream));
    r.in_flight[r.turn] = true;
    r.turn ^= 1;
    if (r.in_flight[r.turn] && hipEventQuery(r.ev[r.turn]) != hipSuccess) HIP_TRY(hipEventSynchronize(r.ev[r.turn]));
    r.in_flight[r.turn] = false;
    r.nj = r.ns = 0;
  }
  const size_t j0 = (size_t)r.turn * r.half_jobs + r.nj, s0 = (size_t)r.turn * r.half_spans + r.ns;
  memcpy(r.h_spans + s0, g->meter_spans.data(), ns * sizeof(PgMeterSpan));
  for (size_t i = 0; i < nj; ++i) {
    PgMeterJob j = g->meter_jobs[i];
    j.span_first += (int32_t)s0;
    j.pub = g->meter_pub_dev[(size_t)j.slot / METER_PUB_CHUNK] + (size_t)j.slot % METER_PUB_CHUNK;
    r.h_jobs[j0 + i] = j;
  }
  r.nj += nj; r.ns += ns;
  PgMeterLaunch L;
  L.jobs = r.d_jobs + j0; L.spans = r.d_spans;
  L.state = g->d_meter_state; L.seen_inactive = g->d_meter_seen;
  L.units = g->d_units.d; L.voices = g->d_voices.d; L.voice_index = g->d_voice_index.d;
  L.interval = g->meter_interval;
  hipLaunchKernelGGL(pg_meter_kernel, dim3((unsigned)nj), dim3(256), 0, stream, L);
  HIP_TRY(hipGetLastError());
  g->meter_jobs.clear(); g->meter_spans.clear();
  return PG_OK;
}

// The main mixer's record, or a part of it: `frames` frames at d_ptr (nullptr: silence) of the write call that began at `time`.
int graph_meter_main(pg_graph* g, const float* d_ptr, uint64_t frames, uint64_t time, bool end_of_record, hipStream_t stream) {
  if (!g->metering || g->failed) return PG_OK;
  (void)hipSetDevice(g->device);
  if (g->last_stream && g->last_stream != stream) { HIP_TRY(pg_stream_sync(g->last_stream)); g->cmds_since_sync = 0; }
  g->last_stream = stream;
  g->meter_jobs.clear(); g->meter_spans.clear();
  uint64_t off = 0;
  do {
    const uint64_t n = std::min<uint64_t>(frames - off, 1u << 29);
    PgMeterSpan sp;
    sp.off = off * 2; sp.time = time; sp.n_frames = (uint32_t)n;
    sp.flags = (d_ptr ? 0 : PG_METER_ZEROS) | ((end_of_record && off + n == frames) ? PG_METER_END_OF_RECORD : 0);
    g->meter_spans.push_back(sp);
    off += n;
  } while (off < frames);
  PgMeterJob j;
  memset(&j, 0, sizeof j);
  j.base = d_ptr; j.slot = 0; j.unit = -1; j.span_first = 0; j.span_count = (int32_t)g->meter_spans.size(); j.flags = PG_METER_JOB_WRITTEN;
  g->meter_jobs.push_back(j);
  return graph_meter_launch(g, stream);
}

static uint64_t meter_interval_frames(double seconds, uint32_t sample_rate) {   // (interval.as_secs_f64() * sample_rate as f64) as u64, src/utils/time.rs:28-35
  const double f = seconds * (double)sample_rate;
  return f >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)f;   // (`as u64` saturates)
}

extern "C" {

int pg_graph_set_metering(pg_graph* g, double interval_seconds) {
  if (std::isnan(interval_seconds) || (std::isinf(interval_seconds) && interval_seconds > 0)) return set_error(PG_ERR_PARAMETER, "Invalid metering interval: %g", interval_seconds);
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (graph_quiesce(g)) { g->failed = true; return PG_ERR_DEVICE; }
  if (interval_seconds < 0) {   // PlayerConfig::metering_interval = None
    g->metering = false;
    g->meter_on.store(0, std::memory_order_release);
    return PG_OK;
  }
  g->metering = true;
  g->meter_interval = meter_interval_frames(interval_seconds, g->sample_rate);
  { const int rc = graph_meter_reserve(g); if (rc) { g->failed = true; return rc; } }
  // AudioLevelState::new for every mixer (metered.rs:87-101): accumulators, clock and published levels at zero
  HIP_TRY(pg_memset(g->d_meter_state, 0, g->meter_cap * sizeof(PgMeterState)));
  HIP_TRY(pg_memset(g->d_meter_seen, 0, g->meter_seen_cap * sizeof(int32_t)));
  for (size_t c = 0; c < PG_METER_PUB_CHUNKS; ++c) {
    PgMeterPub* p = g->meter_pub[c].load(std::memory_order_relaxed);
    if (!p) continue;
    for (size_t i = 0; i < METER_PUB_CHUNK; ++i) {   // (a reader on another thread: the same sequence protocol as the kernel's; the device words restart at 0 with it)
      volatile PgMeterPub* q = p + i;
      q->seq = 1;
      std::atomic_thread_fence(std::memory_order_seq_cst);
      q->peak[0] = q->peak[1] = q->rms[0] = q->rms[1] = 0.0f;
      std::atomic_thread_fence(std::memory_order_seq_cst);
      q->seq = 0;
    }
  }
  g->meter_ring.nj = g->meter_ring.ns = 0;
  g->meter_on.store(1, std::memory_order_release);
  return PG_OK;
}

int pg_graph_mixer_audio_level(pg_graph* g, int mixer_id, pg_audio_level* out) {
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (!out) return set_error(PG_ERR_PARAMETER, "`out` must not be null");
  if (!g->meter_on.load(std::memory_order_acquire)) return set_error(PG_ERR_STATE, "metering is off (pg_graph_set_metering)");
  if (mixer_id < 0 || (size_t)mixer_id >= g->mixer_alive_tab.size() || g->mixer_alive_tab.get((size_t)mixer_id) == 0) return set_error(PG_ERR_NOT_FOUND, "Mixer with id %d not found", mixer_id);
  const PgMeterPub* chunk = g->meter_pub[(size_t)mixer_id / METER_PUB_CHUNK].load(std::memory_order_acquire);
  if (!chunk) return set_error(PG_ERR_NOT_FOUND, "Mixer with id %d not found", mixer_id);
  const volatile PgMeterPub* p = chunk + (size_t)mixer_id % METER_PUB_CHUNK;
  for (;;) {
    const uint32_t s0 = p->seq;
    std::atomic_thread_fence(std::memory_order_acquire);
    pg_audio_level v;
    v.peak[0] = p->peak[0]; v.peak[1] = p->peak[1]; v.rms[0] = p->rms[0]; v.rms[1] = p->rms[1];
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!(s0 & 1u) && p->seq == s0) { *out = v; return PG_OK; }
  }
}

}  // extern "C"
