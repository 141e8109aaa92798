// Host side of the sampler voices: per-voice AHDSR envelopes (src/utils/ahdsr.rs, src/generator/sampler/voice.rs:181-212), granular voices
// (src/generator/sampler/granular.rs; rendered by pg_grain_kernel, pg_k_grain.hip), their modulation matrix (src/modulation/matrix.rs,
// src/generator/sampler/modulation.rs), the granular parameters that change while a voice plays (src/generator/sampler.rs:299-360), sample
// buffers, and the samplers: pools of file voices whose note, allocation and stealing layer runs on the device (pg_sampler_dev.h), and the
// granular-mode samplers: pools of grain records under a note layer of their own kernel (pg_gsampler_dev.h).
// The graph, the control ring's drain and the write path are pg_host.hip's; what crosses between the two files stands in pg_host_internal.h.
//
// Every record has ONE builder and every kind of call one path; where a lone voice and a pool slot start differently, the difference is an argument
// at the call site. Records: grain_rec_init (PgGrainVoice), mod_matrix_init (PgGrainMod), note_rec_init (PgSamplerRec, PgGSampler::note),
// voice_init_grain_staged (a granular voice's or slot's PgVoice). A pool: sampler_pool_check -> sampler_pool_push -> sampler_pool_register, with the
// kind's own tables and uploads between them. A message: sampler_tab_word (does the id take messages, what kind is it) -> sampler_message. A
// read-back: sampler_for_readback. A grain launch: launch_grain_list. The four grow-by-doubling tables (graph_*_reserve) stay four functions: they
// differ in what rides along — three side arrays, a launch list, a header in front, no words at all — more than they agree.
#include "pg_host_internal.h"
#include "pg_grain_dev.h"   // mod_lfo_reset: the note_on of a voice's modulation matrix runs on the host

// ---- `ended` words: one per envelope / granular record, set by the kernel that finds the record's voice ended ----
int MappedWords::reserve(size_t n, const MappedWords& from) {
  if (pg_host_malloc((void**)&h, n * sizeof(int32_t), hipHostMallocMapped) != hipSuccess) { h = nullptr; return PG_ERR_DEVICE; }
  memset(h, 0, n * sizeof(int32_t));
  if (hipHostGetDevicePointer((void**)&d, h, 0) != hipSuccess) { release(); return PG_ERR_DEVICE; }
  if (from.cap) memcpy(h, from.h, from.cap * sizeof(int32_t));
  cap = n;
  return PG_OK;
}
void MappedWords::release() {
  if (h) (void)pg_host_free(h);
  h = nullptr; d = nullptr; cap = 0;
}
// Voices of `ids` whose word is set (or that left the graph): `live` goes off, the id leaves the list and the voice's unit goes back to the
// time-parallel kernels with the next topology upload. Reads mapped host words: no wait. Returns whether any left.
static bool poll_ended(pg_graph* g, std::vector<int>& ids, const MappedWords& words, int HostVoice::*word, bool HostVoice::*live) {
  bool any = false;
  for (size_t i = 0; i < ids.size();) {
    HostVoice& hv = g->voices[ids[i]];
    if (hv.mixer < 0 || words[(size_t)(hv.*word)] != 0) {
      hv.*live = false;
      ids.erase(ids.begin() + i);
      g->topo_dirty = true;
      any = true;
    } else ++i;
  }
  return any;
}
static void samplers_poll_stopped(pg_graph* g);
// Enveloped voices the exact kernel has reported as ended, granular voices pg_grain_kernel has (they leave its launch list too); a pool voice of
// a sampler is not among them: one that ended is started again by a later note
void graph_sampler_poll(pg_graph* g) {
  if (!g->env_voices.empty()) poll_ended(g, g->env_voices, g->env_done, &HostVoice::dev_index, &HostVoice::env_live);
  if (!g->gran_voices.empty() && poll_ended(g, g->gran_voices, g->gran_ended, &HostVoice::gran, &HostVoice::gran_live)) g->gran_live_dirty = true;
  samplers_poll_stopped(g);
}

// The header of envelope table `tab` — its words, its grain_of_voice list, the granular records as the graph holds them now (the graph is quiescent)
static hipError_t env_head_upload(const pg_graph* g, PgEnvTable* tab, const MappedWords& done, const int32_t* grain_of_voice, const int32_t* stat_of_voice) {
  PgEnvTable head;
  memset(&head, 0, sizeof head);
  head.done = done.d; head.cap = done.cap;
  head.grain_of_voice = grain_of_voice; head.grains = g->d_gran; head.n_grains = (uint32_t)g->gran_n;
  head.stat_of_voice = stat_of_voice; head.stats = g->pstat.d_recs; head.n_stats = (uint32_t)g->pstat.n_recs;   // (playback status: pg_k_status.hip)
  head.samplers = g->d_samp;   // (samplers: below)
  return pg_memcpy(tab, &head, sizeof head, hipMemcpyHostToDevice);
}
// The header again, for the tables as the graph holds them now (a table behind it grew: pg_k_status.hip). The graph is quiescent.
int graph_env_head_refresh(pg_graph* g) {
  if (!g->d_env_tab) return PG_OK;
  HIP_TRY(env_head_upload(g, g->d_env_tab, g->env_done, g->d_grain_of_voice, g->pstat.d_of_voice));
  return PG_OK;
}
// The envelope side table and its `ended` words for `n` voices (grow-by-doubling; the graph is quiescent: nothing in flight reads the old ones).
int graph_env_reserve(pg_graph* g, size_t n) {
  if (n <= g->env_done.cap) return PG_OK;
  const size_t cap = std::max<size_t>(next_pow2(n), 64), bytes = sizeof(PgEnvTable) + cap * sizeof(PgEnv);
  PgEnvTable* nt = nullptr;
  int32_t* ngv = nullptr;   // PgEnvTable::grain_of_voice: -1 for every voice that is not granular
  int32_t* nsv = nullptr;   // PgEnvTable::stat_of_voice: -1 for every voice that reports no playback status
  MappedWords done;
  HIP_TRY(pg_malloc((void**)&nt, bytes));
  PgEnv* const nd = (PgEnv*)(nt + 1);
  auto fail = [&](const char* what) { (void)pg_free(nt); if (ngv) (void)pg_free(ngv); if (nsv) (void)pg_free(nsv); done.release(); return set_error(PG_ERR_DEVICE, "envelope table %s failed", what); };
  if (pg_memset(nt, 0, bytes) != hipSuccess || done.reserve(cap, g->env_done) || pg_malloc((void**)&ngv, cap * sizeof(int32_t)) != hipSuccess ||
      pg_memset(ngv, 0xff, cap * sizeof(int32_t)) != hipSuccess || pg_malloc((void**)&nsv, cap * sizeof(int32_t)) != hipSuccess ||
      pg_memset(nsv, 0xff, cap * sizeof(int32_t)) != hipSuccess) return fail("allocation");
  if (env_head_upload(g, nt, done, ngv, nsv) != hipSuccess) return fail("upload");
  if (g->d_env && (pg_memcpy(nd, g->d_env, g->env_done.cap * sizeof(PgEnv), hipMemcpyDeviceToDevice) != hipSuccess ||
                   pg_memcpy(ngv, g->d_grain_of_voice, g->env_done.cap * sizeof(int32_t), hipMemcpyDeviceToDevice) != hipSuccess ||
                   pg_memcpy(nsv, g->pstat.d_of_voice, g->env_done.cap * sizeof(int32_t), hipMemcpyDeviceToDevice) != hipSuccess)) return fail("copy");
  // (the new table is complete: let go of the old one and swap — a failure above leaves the graph on its old table)
  if (g->d_env_tab) (void)pg_free(g->d_env_tab);
  if (g->d_grain_of_voice) (void)pg_free(g->d_grain_of_voice);
  if (g->pstat.d_of_voice) (void)pg_free(g->pstat.d_of_voice);
  g->env_done.release();
  g->d_env_tab = nt; g->d_env = nd; g->env_done = done; g->d_grain_of_voice = ngv; g->pstat.d_of_voice = nsv;
  return PG_OK;
}
// Room for `n` granular records, their `ended` words and their launch list; the window tables with the first one. The graph is quiescent.
// A failure leaves the graph on its old records.
static int graph_gran_reserve(pg_graph* g, size_t n) {
  if (!g->d_grain_lut) {
    std::vector<float> lut((size_t)PG_GRAIN_WINDOWS * PG_GRAIN_LUT_N);
    pg_grain_build_lut(lut.data());
    HIP_TRY(pg_malloc((void**)&g->d_grain_lut, lut.size() * sizeof(float)));
    HIP_TRY(pg_memcpy(g->d_grain_lut, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const size_t cap = std::max<size_t>(next_pow2(n), 16);
  int rc;
  if ((rc = g->d_gran_live.reserve(cap))) return rc;
  g->gran_live.reserve(g->d_gran_live.cap);   // (graph_gran_upload_live runs inside write: it must not allocate)
  if (n <= g->gran_ended.cap) return PG_OK;
  PgGrainVoice* nd = nullptr;
  MappedWords ended;
  HIP_TRY(pg_malloc((void**)&nd, cap * sizeof(PgGrainVoice)));
  if (ended.reserve(cap, g->gran_ended) || (g->gran_n && pg_memcpy(nd, g->d_gran, g->gran_n * sizeof(PgGrainVoice), hipMemcpyDeviceToDevice) != hipSuccess))
    { (void)pg_free(nd); ended.release(); return set_error(PG_ERR_DEVICE, "granular table allocation failed"); }
  if (g->d_gran) (void)pg_free(g->d_gran);
  g->gran_ended.release();
  g->d_gran = nd; g->gran_ended = ended;
  return PG_OK;
}
// The records pg_grain_kernel renders from here on -> its launch list (inside write: capacity was reserved with the voices, nothing allocates)
int graph_gran_upload_live(pg_graph* g, hipStream_t stream) {
  g->gran_live.clear();
  for (int id : g->gran_voices) g->gran_live.push_back(g->voices[id].gran);
  g->gran_live_dirty = false;   // (a failure is the graph's: it renders nothing from then on)
  return g->d_gran_live.upload_async(g->gran_live, stream);
}
// One pg_grain_kernel launch over the `n_live` records of launch list `live`, frames [t0, t0 + n) of the chunk that began at chunk_t0 (inside
// write: nothing allocates)
static int launch_grain_list(pg_graph* g, const int32_t* live, size_t n_live, uint64_t t0, uint32_t n, uint64_t chunk_t0, const PgCmd* d_cmds, int n_cmds, hipStream_t stream) {
  PgGrainLaunch L;
  memset(&L, 0, sizeof L);
  L.recs = g->d_gran; L.n_recs = (uint32_t)g->gran_n; L.n_live = (uint32_t)n_live; L.live = live;
  L.voices = g->d_voices.d; L.cmds = d_cmds; L.n_cmds = n_cmds; L.sample_rate = g->sample_rate; L.lut = g->d_grain_lut; L.ended = g->gran_ended.d;
  L.t0 = t0; L.n = n; L.chunk_t0 = chunk_t0;
  HIP_TRY(pg_launch_grain(L, stream));
  return PG_OK;
}
// ... for the lone granular voices, in front of the unit kernels that take its frames: each picks its voice's commands from the piece's list
int launch_grains(pg_graph* g, uint64_t t0, uint32_t n, uint64_t chunk_t0, const PgCmd* d_cmds, int n_cmds, hipStream_t stream) {
  if (g->gran_voices.empty()) return PG_OK;
  return launch_grain_list(g, g->d_gran_live.d, g->gran_voices.size(), t0, n, chunk_t0, d_cmds, n_cmds, stream);
}
void graph_sampler_release(pg_graph* g) {
  if (g->d_env_tab) (void)pg_free(g->d_env_tab);
  if (g->d_grain_of_voice) (void)pg_free(g->d_grain_of_voice);
  if (g->d_gran) (void)pg_free(g->d_gran);
  if (g->d_grain_lut) (void)pg_free(g->d_grain_lut);
  g->env_done.release(); g->gran_ended.release(); g->d_gran_live.release();
  if (g->d_samp) (void)pg_free(g->d_samp);
  if (g->d_speed_tab) (void)pg_free(g->d_speed_tab);
  g->samp_stopped.release();
  if (g->d_gsamp) (void)pg_free(g->d_gsamp);
  g->d_gsamp_live.release(); g->d_gsamp_grains.release();
}

// note_on belongs to a voice's start (voice.rs:181-184): neither an envelope nor a matrix for a voice that has rendered frames already.
// A voice renders in every write that ends behind its start time — a start time at or before a write's position starts it at once,
// voice_process — so it has rendered iff a write issued since it was added ended behind its start time, wherever the earlier ones stood.
bool voice_has_rendered(const pg_graph* g, const HostVoice& hv) {
  for (const auto& w : g->write_end_max) if (w.first > hv.added_at_write) return w.second > hv.start_time;
  return false;
}
// The Xoshiro256++ state an `rng_state` input stands for (pg_granular_params, pg_mod_lfo): all-zero = SplitMix64 of the fixed seed, four times
static uint64_t splitmix64_next(uint64_t& z) { z += 0x9E3779B97F4A7C15ull; uint64_t x = z; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); }
static void rng_state_from(const uint64_t in[4], uint64_t out[4]) {
  if ((in[0] | in[1] | in[2] | in[3]) != 0) { memmove(out, in, 4 * sizeof(uint64_t)); return; }
  uint64_t z = 0x5EED0000ull;
  for (int i = 0; i < 4; ++i) out[i] = splitmix64_next(z);
}
// pg_granular_params <-> the device's PgGrainParams (rng_state is the pool's, not a parameter: it reads 0 on the way back)
static void grain_params_to_device(const pg_granular_params& p, PgGrainParams& q) {
  q.overlap_mode = p.overlap_mode; q.window = p.window; q.size = p.size; q.density = p.density; q.variation = p.variation; q.spray = p.spray;
  q.pan_spread = p.pan_spread; q.direction = p.playback_direction; q.position = p.position; q.step = p.step;
  q.has_loop = p.has_loop_range ? 1 : 0; q.loop_start = p.has_loop_range ? p.loop_start : 0.0f; q.loop_end = p.has_loop_range ? p.loop_end : 0.0f;
}
static void grain_params_from_device(const PgGrainParams& q, pg_granular_params& p) {
  memset(&p, 0, sizeof p);
  p.overlap_mode = q.overlap_mode; p.window = q.window; p.size = q.size; p.density = q.density; p.variation = q.variation; p.spray = q.spray;
  p.pan_spread = q.pan_spread; p.playback_direction = q.direction; p.position = q.position; p.step = q.step;
  p.has_loop_range = q.has_loop; p.loop_start = q.loop_start; p.loop_end = q.loop_end;
}
// The reference's parameter errors (ahdsr.rs:143-152, :179-188, :224-233, :259-268) + what no Duration can hold; touches no graph and no device.
int pg_ahdsr_params_check(const pg_ahdsr_params* p) {
  if (!p) return set_error(PG_ERR_PARAMETER, "envelope parameters must not be null");
  const float times[4] = {p->attack_s, p->hold_s, p->decay_s, p->release_s};
  static const char* const names[4] = {"attack", "hold", "decay", "release"};
  for (int i = 0; i < 4; ++i) if (!std::isfinite(times[i]) || times[i] < 0.0f) return set_error(PG_ERR_PARAMETER, "Invalid %s time: %g. Must be finite and >= 0", names[i], (double)times[i]);
  if (!(p->attack_scaling >= -1.0f && p->attack_scaling <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Invalid attack scaling: %g. Must be in range [-1.0, 1.0]", (double)p->attack_scaling);
  if (!(p->decay_scaling >= -1.0f && p->decay_scaling <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Invalid decay scaling: %g. Must be in range [-1.0, 1.0]", (double)p->decay_scaling);
  if (!(p->sustain_level >= 0.0f && p->sustain_level <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Invalid sustain level: %g. Must be in range [0.0, 1.0]", (double)p->sustain_level);
  if (!(p->release_scaling >= -1.0f && p->release_scaling <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Invalid release scaling: %g. Must be in range [-1.0, 1.0]", (double)p->release_scaling);
  return PG_OK;
}

// The debug read-backs of a granular record `rec`: a voice's, or a slot's of a granular-mode sampler
static int grain_state_read(pg_graph* g, int rec, pg_grain_state* out) {
  std::unique_ptr<PgGrainVoice> r(new PgGrainVoice);
  { const int rc = graph_read_back(g, r.get(), g->d_gran + rec, sizeof(PgGrainVoice)); if (rc) return rc; }
  memset(out, 0, sizeof *out);
  const PgGrainPool& pool = r->pool;
  out->trigger_phase = pool.trigger_phase; out->playhead = pool.playhead; out->playing_loop_range = pool.playing_loop_range;
  out->trigger_new_grains = pool.trigger_new_grains; out->primary_slot = pool.primary; out->overlap_mode = pool.overlap_mode; out->speed = pool.speed; out->volume = pool.volume; out->panning = pool.panning;
  memcpy(out->rng_state, pool.rng, sizeof out->rng_state);
  for (int i = 0; i < PG_GRAIN_POOL; ++i) {
    const PgGrain& s = r->grains[i];
    pg_grain_slot& o = out->slots[i];
    o.position = s.position; o.increment = s.increment; o.window_phase = s.window_phase; o.window_increment = s.window_increment;
    o.samples_remaining = s.samples_remaining; o.volume = s.volume; o.panning = s.panning; o.active = s.active; o.window_mode = s.window_mode; o.has_loop_range = s.has_loop;
  }
  return PG_OK;
}
static int granular_params_read(pg_graph* g, int rec, pg_granular_params* out) {
  PgGrainParams q;
  { const int rc = graph_read_back(g, &q, (const char*)(g->d_gran + rec) + offsetof(PgGrainVoice, params), sizeof q); if (rc) return rc; }
  grain_params_from_device(q, *out);
  return PG_OK;
}
static int modulation_state_read(pg_graph* g, int rec, pg_modulation_state* out) {
  PgGrainMod m;
  { const int rc = graph_read_back(g, &m, (const char*)(g->d_gran + rec) + offsetof(PgGrainVoice, mod), sizeof m); if (rc) return rc; }
  memset(out, 0, sizeof *out);
  for (int l = 0; l < 2; ++l) {
    const PgModLfo& s = m.lfo[l];
    pg_mod_lfo_state& o = out->lfo[l];
    o.phase = s.phase; o.phase_inc = s.phase_inc; o.sample_hold = s.sample_hold; o.jitter_current = s.jitter_current; o.jitter_target = s.jitter_target; o.waveform = s.waveform;
    memcpy(o.rng_state, s.rng, sizeof o.rng_state);
  }
  out->velocity = m.velocity; out->note_pitch = m.note_pitch;
  for (int s = 0; s < PG_MOD_SOURCES; ++s) for (int t = 0; t < PG_MOD_TARGETS; ++t) { out->routes[s][t].amount = m.amount[s][t]; out->routes[s][t].bipolar = m.bipolar[s][t]; }
  for (int t = 0; t < PG_MOD_TARGETS; ++t) out->last[t] = m.last[t];
  return PG_OK;
}

extern "C" {

void pg_ahdsr_params_default(pg_ahdsr_params* p) {  // AhdsrParameters::default (utils/ahdsr.rs:348-359)
  if (!p) return;
  p->attack_s = 0.010f; p->attack_scaling = 0.0f; p->hold_s = 1.0f; p->decay_s = 0.5f; p->decay_scaling = 0.0f; p->sustain_level = 0.75f; p->release_s = 1.0f; p->release_scaling = 0.0f;
}
// AhdsrParameters::new_with_scaling + set_sample_rate(sample_rate) (ahdsr.rs:75-98, :123-136), setter by setter in the reference's order: the
// first setup runs at the placeholder rate with the sustain level still 0 when set_decay_time divides (:205-214, :307-309); the second one —
// set_sample_rate's, skipped when the rate IS the placeholder — is what gives decay_rate its final value.
static PgEnvParams ahdsr_build_params(const pg_ahdsr_params& a, uint32_t sample_rate) {
  PgEnvParams p;
  memset(&p, 0, sizeof p);
  uint32_t sr = 66666;  // UNINITIALIZED_SAMPLE_RATE
  auto set_attack = [&]() { p.attack_rate = a.attack_s == 0.0f ? FLT_MAX : 1.0f / (a.attack_s * (float)sr); };
  auto set_decay = [&]() { p.decay_rate = a.decay_s == 0.0f ? FLT_MAX : (1.0f - p.sustain_level) / (a.decay_s * (float)sr); };
  auto set_release = [&]() { p.release_rate = a.release_s == 0.0f ? FLT_MAX : 1.0f / (a.release_s * (float)sr); };
  set_attack(); p.attack_scaling = a.attack_scaling; set_decay(); p.decay_scaling = a.decay_scaling; p.sustain_level = a.sustain_level; set_release(); p.release_scaling = a.release_scaling;
  if (sr != sample_rate) { sr = sample_rate; set_attack(); set_decay(); p.sustain_level = a.sustain_level; set_release(); }
  p.hold_samples = a.hold_s * (float)sr;
  p.zero_times = (a.hold_s == 0.0f ? PG_AHDSR_HOLD_ZERO : 0) | (a.decay_s == 0.0f ? PG_AHDSR_DECAY_ZERO : 0) | (a.release_s == 0.0f ? PG_AHDSR_RELEASE_ZERO : 0);
  return p;
}
int pg_graph_set_voice_envelope(pg_graph* g, int voice_id, const pg_ahdsr_params* p) {
  { const int rc = pg_ahdsr_params_check(p); if (rc) return rc; }
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (voice_kind(g, voice_id) == VOICE_DEAD) return set_error(PG_ERR_NOT_FOUND, "Source with id %d not found", voice_id);
  drain_control_messages(g);
  if (g->voices[voice_id].mixer < 0) return set_error(PG_ERR_NOT_FOUND, "Source with id %d not found", voice_id);
  HostVoice& hv = g->voices[voice_id];
  if (voice_has_rendered(g, hv)) return set_error(PG_ERR_STATE, "Source with id %d has rendered frames already: an envelope is attached before the voice starts", voice_id);
  if (graph_quiesce(g)) return graph_fail(g, PG_ERR_DEVICE);
  if (graph_env_reserve(g, std::max<size_t>(g->voices.size(), (size_t)hv.dev_index + 1))) return graph_fail(g, PG_ERR_DEVICE);
  PgEnv e;
  memset(&e, 0, sizeof e);
  e.on = 1;
  e.params = ahdsr_build_params(*p, g->sample_rate);
  // AhdsrEnvelope::note_on(parameters, 1.0) (ahdsr.rs:402-419)
  e.state.target_volume = 1.0f;
  if (e.params.attack_rate == FLT_MAX) {
    e.state.output = 1.0f;
    if (!(e.params.zero_times & PG_AHDSR_HOLD_ZERO)) { e.state.stage = PG_AHDSR_HOLD; e.state.hold_samples_remaining = e.params.hold_samples; }
    else e.state.stage = PG_AHDSR_DECAY;
  } else { e.state.output = 0.0f; e.state.stage = PG_AHDSR_ATTACK; }
  (void)hipSetDevice(g->device);
  HIP_TRY(pg_memcpy(g->d_env + hv.dev_index, &e, sizeof e, hipMemcpyHostToDevice));
  g->env_done[(size_t)hv.dev_index] = 0;
  if (hv.gran >= 0) {  // pg_grain_kernel: a release is the envelope's note_off from here on, not GrainPool::stop
    const int32_t one = 1;
    HIP_TRY(pg_memcpy((char*)(g->d_gran + hv.gran) + offsetof(PgGrainVoice, has_env), &one, sizeof one, hipMemcpyHostToDevice));
  }
  if (!hv.env_live) g->env_voices.push_back(voice_id);
  hv.env = true; hv.env_live = true;
  g->topo_dirty = true;
  return PG_OK;
}
int pg_graph_voice_envelope_stage(pg_graph* g, int voice_id) {
  if (!g || voice_id < 0 || voice_id >= (int)g->voices.size() || g->voices[voice_id].mixer < 0 || !g->voices[voice_id].env || !g->d_env) return -1;
  PgEnv e;
  if (graph_read_back(g, &e, g->d_env + g->voices[voice_id].dev_index, sizeof e)) return -1;
  return e.on ? (int)e.state.stage : -1;
}

// ---- granular voices (src/generator/sampler/granular.rs; pg_k_grain.hip) ----
void pg_granular_params_default(pg_granular_params* p) {  // GranularParameters::default (granular.rs:268-283)
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->overlap_mode = 0; p->window = 2; p->size = 100.0f; p->density = 10.0f; p->playback_direction = 0; p->position = 0.5f;
}
int pg_granular_params_check(const pg_granular_params* p) {  // GranularParameters::validate (granular.rs:291-335); a NaN fails every range
  if (!p) return set_error(PG_ERR_PARAMETER, "granular parameters must not be null");
  if (p->overlap_mode < 0 || p->overlap_mode > 1) return set_error(PG_ERR_PARAMETER, "Invalid grain overlap mode: %d", p->overlap_mode);
  if (p->window < 0 || p->window >= PG_GRAIN_WINDOWS) return set_error(PG_ERR_PARAMETER, "Invalid grain window mode: %d", p->window);
  if (p->playback_direction < 0 || p->playback_direction > 2) return set_error(PG_ERR_PARAMETER, "Invalid grain playback direction: %d", p->playback_direction);
  if (!(p->size >= 1.0f && p->size <= 1000.0f)) return set_error(PG_ERR_PARAMETER, "Grain size must be between 1 and 1000 ms");
  if (!(p->density >= 1.0f && p->density <= 100.0f)) return set_error(PG_ERR_PARAMETER, "Grain density must be between 1.0 and 100.0 Hz");
  if (!(p->spray >= 0.0f && p->spray <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Grain spray must be between 0.0 and 1.0");
  if (!(p->variation >= 0.0f && p->variation <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Grain variation must be between 0.0 and 1.0");
  if (!(p->pan_spread >= 0.0f && p->pan_spread <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Grain pan spread must be between 0.0 and 1.0");
  if (!(p->position >= 0.0f && p->position <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Position must be between 0.0 and 1.0");
  if (!(p->step >= -4.0f && p->step <= 4.0f)) return set_error(PG_ERR_PARAMETER, "Step must be between -4.0 and 4.0");
  if (p->has_loop_range && !(p->loop_start >= 0.0f && p->loop_start <= 1.0f && p->loop_end >= 0.0f && p->loop_end <= 1.0f))
    return set_error(PG_ERR_PARAMETER, "Invalid loop points (should be relative positions), but are: (%g, %g)", (double)p->loop_start, (double)p->loop_end);
  return PG_OK;
}
}  // extern "C"
// A granular voice as its mixer sees it — a lone one or a slot of a granular-mode sampler: a stereo source at the graph's rate whose frames
// pg_grain_kernel stages; AmplifiedSource / PannedSource / fader are neutral — the granular branch of SamplerVoice::process does not pass them
// (voice.rs:412-427)
static void voice_init_grain_staged(const pg_graph* g, PgVoice& v, const pg_voice_options* opt) {
  voice_init_neutral(g, v, opt, 1.0f, 0.0f);
  v.channels = 2; v.src_rate = g->sample_rate; v.out_rate = g->sample_rate; v.ratio = 1.0f;
  v.current_speed = 1.0; v.target_speed = 1.0;
  v.sched_class = -1;
}
// The staging buffer of a granular record (PgGrainVoice::staged), zeroed; on a failure *p is null or what the caller has to free
static hipError_t grain_stage_alloc(void** p) {
  const size_t bytes = (size_t)PG_MAX_FRAMES * 2 * sizeof(float);
  const hipError_t err = pg_malloc(p, bytes);
  return err != hipSuccess ? err : pg_memset(*p, 0, bytes);
}
// The ONE builder of a granular record: GrainPool::new (granular.rs:384-429) over `n_frames` mono frames at `pcm`, rendering into `staged` for the
// voice with device index `voice`. `rng`: an rng_state input (all-zero = the fixed seed). What a lone voice and a sampler's slot start with
// differently are the arguments in the middle; each call site says where its values come from. No envelope and no matrix yet.
static void grain_rec_init(PgGrainVoice& r, const pg_granular_params& p, const uint64_t rng[4], double speed, float volume, float panning, float trigger_phase, float playhead,
                           const float* pcm, uint64_t n_frames, void* staged, uint64_t start_time, int voice) {
  memset(&r, 0, sizeof r);
  grain_params_to_device(p, r.params);
  PgGrainPool& pool = r.pool;
  rng_state_from(rng, pool.rng);
  pool.trigger_new_grains = 1; pool.trigger_phase = trigger_phase;
  pool.speed = speed; pool.volume = volume; pool.panning = panning;
  pool.playhead = playhead; pool.playing_loop_range = 0; pool.primary = -1; pool.overlap_mode = 0;   // (Cloud: GrainPool::new, granular.rs:399)
  for (int i = 0; i < PG_GRAIN_POOL; ++i) { r.grains[i].volume = 1.0f; r.grains[i].window_mode = 2; }   // Grain::new (:995-1008)
  r.pcm = pcm; r.n_frames = n_frames; r.staged = (float*)staged; r.stage_pos = 0;
  r.start_time = start_time; r.stop_time = UINT64_MAX; r.exhausted_at = UINT64_MAX; r.voice = voice; r.has_env = 0;
}
// pg_graph_add_granular_voice / _from_buffer: `mono_pcm` (copied to the device, owned by the voice) or, with mono_pcm null, the granular mono
// buffer of sample buffer `sbuf` (made already; n_frames is its length)
static int graph_add_granular_voice(pg_graph* g, int mixer_id, const float* mono_pcm, int sbuf, size_t n_frames, const pg_granular_params* p, const pg_voice_options* opt) {
  { const int rc = pg_granular_params_check(p); if (rc) return -rc; }
  if (!g) return -set_error(PG_ERR_PARAMETER, "graph handle is null");
  if ((!mono_pcm && sbuf < 0) || n_frames < 1) return -set_error(PG_ERR_PARAMETER, "Need a valid, non empty sample buffer");
  if (mixer_id < 0 || mixer_id >= (int)g->mixers.size() || g->mixers[mixer_id].removed) return -set_error(PG_ERR_NOT_FOUND, "Mixer with id %d not found", mixer_id);
  drain_control_messages(g);
  pg_voice_options def;
  if (!opt) { pg_voice_options_default(&def); opt = &def; }
  if (!(opt->speed > 0.0)) return -set_error(PG_ERR_PARAMETER, "speed must be > 0");
  if (opt->volume < 0.0f || opt->panning < -1.0f || opt->panning > 1.0f) return -set_error(PG_ERR_PARAMETER, "invalid volume or panning");
  if (graph_quiesce(g)) return -graph_fail(g, PG_ERR_DEVICE);
  PgVoice v;
  voice_init_grain_staged(g, v, opt);
  HostVoice hv;
  auto release = [&]() { if (hv.d_pcm) (void)pg_free(hv.d_pcm); if (hv.d_stage) (void)pg_free(hv.d_stage); };
  if ((sbuf < 0 && (pg_malloc(&hv.d_pcm, n_frames * sizeof(float)) != hipSuccess || pg_memcpy(hv.d_pcm, mono_pcm, n_frames * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) ||
      grain_stage_alloc(&hv.d_stage) != hipSuccess) {
    release();
    return -graph_fail(g, set_error(PG_ERR_DEVICE, "granular voice allocation failed"));
  }
  if (graph_gran_reserve(g, g->gran_n + 1)) { release(); return -graph_fail(g, PG_ERR_DEVICE); }
  int dev_index = -1;
  int rc = g->d_voices.push(v, &dev_index);
  if (rc) { release(); return -graph_fail(g, rc); }
  if (graph_env_reserve(g, std::max<size_t>(g->voices.size() + 1, (size_t)dev_index + 1))) { release(); return -graph_fail(g, PG_ERR_DEVICE); }
  // GrainPool::new, then start(parameters, speed, volume, panning) (granular.rs:474-489) with the options' three: the trigger phase is 1.0 — the
  // first frame triggers a grain — and the playhead stands at the parameters' position; the voice starts at the options' start time
  std::unique_ptr<PgGrainVoice> r(new PgGrainVoice);
  grain_rec_init(*r, *p, p->rng_state, opt->speed, opt->volume, opt->panning, /*trigger_phase*/ 1.0f, /*playhead*/ p->position,
                 sbuf >= 0 ? g->sample_buffers[sbuf].d_mono : (const float*)hv.d_pcm, n_frames, hv.d_stage, opt->start_time, dev_index);
  const int32_t rec = (int32_t)g->gran_n;
  (void)hipSetDevice(g->device);
  if (pg_memcpy(g->d_gran + rec, r.get(), sizeof(PgGrainVoice), hipMemcpyHostToDevice) != hipSuccess ||
      pg_memcpy(g->d_grain_of_voice + dev_index, &rec, sizeof rec, hipMemcpyHostToDevice) != hipSuccess) { release(); return -graph_fail(g, set_error(PG_ERR_DEVICE, "granular voice upload failed")); }
  g->gran_ended[(size_t)rec] = 0;
  g->gran_n += 1;
  if (env_head_upload(g, g->d_env_tab, g->env_done, g->d_grain_of_voice, g->pstat.d_of_voice) != hipSuccess) { release(); return -graph_fail(g, set_error(PG_ERR_DEVICE, "granular voice upload failed")); }
  hv.gran = rec; hv.gran_live = true;
  if (sbuf >= 0) { const SampleBuffer& b = g->sample_buffers[sbuf]; hv.file_channels = b.channels; hv.file_rate = b.rate; hv.file_samples = (uint64_t)b.n_frames * b.channels; }
  else { hv.file_channels = 1; hv.file_rate = g->sample_rate; hv.file_samples = n_frames; }
  if (sbuf >= 0) { hv.sbuf = sbuf; g->sample_buffers[sbuf].use_count += 1; }   // (nothing fails behind this that would release the voice)
  return graph_register_voice(g, mixer_id, dev_index, opt, hv, VOICE_GRANULAR);
}

// ---- sample buffers (src/source/file/buffer.rs behind an Arc; the granular mono buffer: pg_k_sample.hip) ----
int sample_buffer_desc_check(const float* pcm, size_t n_frames, const pg_sample_buffer_desc* d) {   // AudioFileBuffer::new (file/buffer.rs:22-60)
  if (!pcm || !d) return set_error(PG_ERR_PARAMETER, "sample buffer PCM and description must not be empty");
  if (n_frames < 1) return set_error(PG_ERR_PARAMETER, "file buffer must not be empty");
  if (d->channels != 1 && d->channels != 2) return set_error(PG_ERR_PARAMETER, "only mono and stereo file buffers are supported");
  if (d->rate == 0) return set_error(PG_ERR_PARAMETER, "file buffer sample rate must be > 0");
  if (d->has_loop_range && (d->loop_start >= n_frames || d->loop_end > n_frames || d->loop_start >= d->loop_end))
    return set_error(PG_ERR_PARAMETER, "file buffer loop range is out of bounds");
  return PG_OK;
}
SampleBuffer* sample_buffer_find(pg_graph* g, int buffer_id) {
  if (buffer_id < 0 || buffer_id >= (int)g->sample_buffers.size() || !g->sample_buffers[buffer_id].held) { set_error(PG_ERR_NOT_FOUND, "Sample buffer with id %d not found", buffer_id); return nullptr; }
  return &g->sample_buffers[buffer_id];
}
bool sample_buffer_timing() {   // the measurement hook is armed like the fault injector: only with PHONIC_DEBUG_HOOKS=1 in the environment
  static const bool armed = [] { const char* e = getenv("PHONIC_DEBUG_HOOKS"); return e && e[0] == '1'; }();
  return armed;
}
static void sample_buffer_free(SampleBuffer& b) {   // nobody holds it: nothing in flight reads it (the graph is quiescent)
  if (b.d_mono && b.d_mono != (float*)b.d_pcm) (void)pg_free(b.d_mono);
  if (b.d_pcm) (void)pg_free(b.d_pcm);
  b.d_pcm = nullptr; b.d_mono = nullptr;
}
void sample_buffer_unref(pg_graph* g, int sbuf) {
  SampleBuffer& b = g->sample_buffers[sbuf];
  if (--b.use_count == 0 && !b.held) sample_buffer_free(b);
}
void graph_sample_buffers_release(pg_graph* g) {
  for (SampleBuffer& b : g->sample_buffers) sample_buffer_free(b);
  g->sample_buffers.clear();
}

extern "C" {

int pg_graph_add_granular_voice(pg_graph* g, int mixer_id, const float* mono_pcm, size_t n_frames, const pg_granular_params* p, const pg_voice_options* opt) {
  return graph_add_granular_voice(g, mixer_id, mono_pcm, -1, n_frames, p, opt);
}
int pg_graph_add_sample_buffer(pg_graph* g, const float* pcm, size_t n_frames, const pg_sample_buffer_desc* desc) {
  { const int rc = sample_buffer_desc_check(pcm, n_frames, desc); if (rc) return -rc; }
  if (!g) return -set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (graph_quiesce(g)) return -graph_fail(g, PG_ERR_DEVICE);
  SampleBuffer b;
  b.n_frames = n_frames; b.channels = desc->channels; b.rate = desc->rate;
  b.has_loop = desc->has_loop_range != 0; b.loop_start = b.has_loop ? desc->loop_start : 0; b.loop_end = b.has_loop ? desc->loop_end : 0;
  const size_t bytes = n_frames * desc->channels * sizeof(float);
  hipEvent_t e0 = nullptr, e1 = nullptr;   // (measurement hook, pg_debug_sample_buffer_times: no event without PHONIC_DEBUG_HOOKS=1)
  hipError_t err = pg_malloc(&b.d_pcm, bytes);
  const bool timed = sample_buffer_timing() && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess && hipEventRecord(e0, g->stream) == hipSuccess;
  if (err == hipSuccess) err = pg_memcpy(b.d_pcm, pcm, bytes, hipMemcpyHostToDevice);
  if (err == hipSuccess && timed && hipEventRecord(e1, g->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess) (void)hipEventElapsedTime(&b.upload_ms, e0, e1);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (err != hipSuccess) { if (b.d_pcm) (void)pg_free(b.d_pcm); return -graph_fail(g, set_error(PG_ERR_DEVICE, "sample buffer upload failed: %s", hipGetErrorString(err))); }
  g->sample_buffers.push_back(b);
  return (int)g->sample_buffers.size() - 1;
}
int pg_graph_release_sample_buffer(pg_graph* g, int buffer_id) {
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  SampleBuffer* b = sample_buffer_find(g, buffer_id);
  if (!b) return PG_ERR_NOT_FOUND;
  if (graph_quiesce(g)) return graph_fail(g, PG_ERR_DEVICE);   // (voices retired by earlier writes let go of their references here)
  b->held = false;
  if (b->use_count == 0) sample_buffer_free(*b);
  return PG_OK;
}
int pg_graph_add_voice_from_buffer(pg_graph* g, int mixer_id, int buffer_id, const pg_voice_options* opt) {
  if (!g) return -set_error(PG_ERR_PARAMETER, "graph handle is null");
  const SampleBuffer* b = sample_buffer_find(g, buffer_id);
  if (!b) return -PG_ERR_NOT_FOUND;
  return graph_add_file_voice(g, mixer_id, nullptr, buffer_id, b->n_frames, b->channels, b->rate, opt);
}
int pg_graph_prepare_granular_buffer(pg_graph* g, int buffer_id) {
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  SampleBuffer* b = sample_buffer_find(g, buffer_id);
  if (!b) return PG_ERR_NOT_FOUND;
  if (b->mono_frames >= 0) return PG_OK;
  if (graph_quiesce(g)) return graph_fail(g, PG_ERR_DEVICE);
  const int rc = sample_buffer_convert(g, *b);
  return rc == PG_ERR_DEVICE ? graph_fail(g, rc) : rc;
}
int pg_graph_add_granular_voice_from_buffer(pg_graph* g, int mixer_id, int buffer_id, const pg_granular_params* p, const pg_voice_options* opt) {
  { const int rc = pg_granular_params_check(p); if (rc) return -rc; }
  if (!g) return -set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (mixer_id < 0 || mixer_id >= (int)g->mixers.size() || g->mixers[mixer_id].removed) return -set_error(PG_ERR_NOT_FOUND, "Mixer with id %d not found", mixer_id);
  { const int rc = pg_graph_prepare_granular_buffer(g, buffer_id); if (rc) return -rc; }
  const SampleBuffer& b = g->sample_buffers[buffer_id];
  pg_granular_params q = *p;
  if (!q.has_loop_range && b.has_loop) {   // SamplerVoice::enable_granular_playback (voice.rs:355-360)
    const float total = (float)b.n_frames;
    q.has_loop_range = 1; q.loop_start = (float)b.loop_start / total; q.loop_end = (float)b.loop_end / total;
  }
  return graph_add_granular_voice(g, mixer_id, nullptr, buffer_id, (size_t)b.mono_frames, &q, opt);
}
int pg_graph_sample_buffer_info(pg_graph* g, int buffer_id, pg_sample_buffer_info* out) {
  if (!g || !out) return set_error(PG_ERR_PARAMETER, "graph handle or output is null");
  const SampleBuffer* b = sample_buffer_find(g, buffer_id);
  if (!b) return PG_ERR_NOT_FOUND;
  memset(out, 0, sizeof *out);
  out->n_frames = b->n_frames; out->channels = b->channels; out->rate = b->rate; out->has_loop_range = b->has_loop ? 1 : 0; out->use_count = b->use_count;
  out->loop_start = b->loop_start; out->loop_end = b->loop_end; out->granular_frames = b->mono_frames;
  return PG_OK;
}
int pg_debug_sample_buffer_times(pg_graph* g, int buffer_id, float out_ms[3]) {
  if (!g || !out_ms) return set_error(PG_ERR_PARAMETER, "graph handle or output is null");
  const SampleBuffer* b = sample_buffer_find(g, buffer_id);
  if (!b) return PG_ERR_NOT_FOUND;
  out_ms[0] = b->upload_ms; out_ms[1] = b->sched_ms; out_ms[2] = b->interp_ms;
  return PG_OK;
}
int64_t pg_graph_read_granular_buffer(pg_graph* g, int buffer_id, float* out, size_t cap_frames) {
  if (!g || (!out && cap_frames)) return -set_error(PG_ERR_PARAMETER, "graph handle or output is null");
  { const int rc = pg_graph_prepare_granular_buffer(g, buffer_id); if (rc) return -rc; }
  const SampleBuffer& b = g->sample_buffers[buffer_id];
  const size_t n = std::min<size_t>(cap_frames, (size_t)b.mono_frames);
  if (n) { const int rc = graph_read_back(g, out, b.d_mono, n * sizeof(float)); if (rc) return -rc; }
  return b.mono_frames;
}
int pg_graph_voice_grain_state(pg_graph* g, int voice_id, pg_grain_state* out) {
  if (!g || !out) return set_error(PG_ERR_PARAMETER, "graph handle or output is null");
  if (voice_id < 0 || voice_id >= (int)g->voices.size() || g->voices[voice_id].gran < 0) return set_error(PG_ERR_NOT_FOUND, "Source with id %d is not a granular voice", voice_id);
  return grain_state_read(g, g->voices[voice_id].gran, out);
}
// ---- the granular parameters and the loop range while the voice plays (Sampler::set_granular_parameter, sampler.rs:299-360, :1132-1147;
// SamplerMessage::SetLoopRange -> GrainPool::set_loop_range, sampler.rs:1246-1270, granular.rs:516-518) ----
// The timed calls: records in the control ring like the other voice commands; the writing thread turns them into events of the voice's mixer.
int pg_graph_set_voice_granular_parameter(pg_graph* g, int voice_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time) {
  const int pi = find_granular_param(fourcc);
  if (pi < 0) return set_error(PG_ERR_PARAMETER, "Invalid/unknown granular playback parameter 0x%08x", fourcc);
  if (value != value) return set_error(PG_ERR_PARAMETER, "Granular playback parameter '%s' is not a number", GRANULAR_PARAMS[pi].name);
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  float raw;
  if (!resolve_update(GRANULAR_PARAMS[pi], value, is_normalized != 0, raw)) {  // a raw enum index out of range: logged + ignored in the reference (enum.rs:256-290)
    if (!voice_kind_is_granular(voice_kind(g, voice_id))) return set_error(PG_ERR_NOT_FOUND, "Source with id %d is not a granular voice", voice_id);
    return PG_OK;
  }
  return voice_message(g, voice_id, VOICE_GRANULAR, pgc::CT_VOICE_GRAIN_PARAM, sample_time, raw, pi);
}
int pg_graph_set_voice_grain_loop_range(pg_graph* g, int voice_id, int has_loop_range, float loop_start, float loop_end, uint64_t sample_time) {
  if (has_loop_range && !(loop_start >= 0.0f && loop_start <= 1.0f && loop_end >= 0.0f && loop_end <= 1.0f))
    return set_error(PG_ERR_PARAMETER, "Invalid loop points (should be relative positions), but are: (%g, %g)", (double)loop_start, (double)loop_end);
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  return voice_message(g, voice_id, VOICE_GRANULAR, pgc::CT_VOICE_GRAIN_LOOP, sample_time, has_loop_range ? loop_start : 0.0f, has_loop_range ? 1 : 0, 0.0, has_loop_range ? loop_end : 0.0f);
}
int pg_graph_voice_granular_params(pg_graph* g, int voice_id, pg_granular_params* out) {
  if (!g || !out) return set_error(PG_ERR_PARAMETER, "graph handle or output is null");
  if (voice_id < 0 || voice_id >= (int)g->voices.size() || g->voices[voice_id].gran < 0) return set_error(PG_ERR_NOT_FOUND, "Source with id %d is not a granular voice", voice_id);
  return granular_params_read(g, g->voices[voice_id].gran, out);
}

// ---- the modulation matrix of a granular voice (src/modulation/matrix.rs, src/generator/sampler/modulation.rs; phase 0 of pg_grain_kernel) ----
static_assert(PG_MOD_SOURCES == PG_GMOD_SOURCES && PG_MOD_TARGETS == PG_GMOD_TARGETS, "the header's and the device's matrix agree");
static float mod_clamp_rate(float rate_hz) { return rate_hz < 0.01f ? 0.01f : (rate_hz > 20.0f ? 20.0f : rate_hz); }   // FloatParameter::clamp_value of ML1R / ML2R (sampler.rs:369-384)
static float mod_phase_inc(float rate_hz, uint32_t sample_rate) { return (float)((double)mod_clamp_rate(rate_hz) / (double)sample_rate); }   // Lfo::set_rate (lfo.rs:102-104)
void pg_modulation_params_default(pg_modulation_params* p) {  // Sampler::modulation_config (sampler.rs:369-427), a note at full velocity
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->lfo[0].rate_hz = 1.0f; p->lfo[0].waveform = 0;
  p->lfo[1].rate_hz = 2.0f; p->lfo[1].waveform = 1;
  p->velocity = 1.0f; p->note = 60;
}
static int mod_check_route(int source, int target, float amount) {  // ModulationState::set_modulation (state.rs:174-201)
  if (source < 0 || source >= PG_MOD_SOURCES) return set_error(PG_ERR_PARAMETER, "Unknown modulation source '%d'", source);
  if (target < 0 || target >= PG_MOD_TARGETS) return set_error(PG_ERR_PARAMETER, "Unknown modulation target '%d'", target);
  if (!(amount >= -1.0f && amount <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Modulation amount must be in range -1..-1.0 but is %g", (double)amount);
  return PG_OK;
}
int pg_modulation_params_check(const pg_modulation_params* p) {
  if (!p) return set_error(PG_ERR_PARAMETER, "modulation parameters must not be null");
  for (int l = 0; l < 2; ++l) {
    if (p->lfo[l].rate_hz != p->lfo[l].rate_hz) return set_error(PG_ERR_PARAMETER, "LFO %d rate is not a number", l + 1);
    if (p->lfo[l].waveform < 0 || p->lfo[l].waveform > 6) return set_error(PG_ERR_PARAMETER, "Invalid LFO %d waveform: %d", l + 1, p->lfo[l].waveform);
  }
  if (!(p->velocity >= 0.0f && p->velocity <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Velocity must be in range [0.0, 1.0]");
  if (p->note < 0 || p->note > 127) return set_error(PG_ERR_PARAMETER, "MIDI note must be in range [0, 127]");
  for (int s = 0; s < PG_MOD_SOURCES; ++s) for (int t = 0; t < PG_MOD_TARGETS; ++t) { const int rc = mod_check_route(s, t, p->routes[s][t].amount); if (rc) return rc; }
  return PG_OK;
}
// The ONE builder of a matrix, as create_matrix leaves it before any note (voice.rs:341-373): each Lfo::new(sample_rate, default rate, default
// waveform) draws its three random values from its generator (state.rs:96-113, lfo.rs:70-86) — `rng0` / `rng1`: an rng_state input per LFO,
// all-zero = the fixed seed —, then the parameter updates in front of the first note, set_rate / set_waveform (lfo.rs:102-119), then the routes.
// The two static sources stand where they stand before a note (processor.rs:236-244, :292-298); note_on — mod_lfo_reset, velocity, note pitch — is
// the caller's, where it has a note.
static void mod_matrix_init(PgGrainMod& m, const pg_modulation_params& p, uint32_t sample_rate, const uint64_t rng0[4], const uint64_t rng1[4]) {
  memset(&m, 0, sizeof m);
  m.on = 1;
  for (int l = 0; l < 2; ++l) {
    PgModLfo& o = m.lfo[l];
    rng_state_from(l ? rng1 : rng0, o.rng);
    o.phase = 0.0f;
    o.sample_hold = lfo_random_bipolar(o.rng); o.jitter_current = lfo_random_bipolar(o.rng); o.jitter_target = lfo_random_bipolar(o.rng);
    o.phase_inc = mod_phase_inc(p.lfo[l].rate_hz, sample_rate);
    o.waveform = p.lfo[l].waveform;
  }
  for (int s = 0; s < PG_MOD_SOURCES; ++s) for (int t = 0; t < PG_MOD_TARGETS; ++t) {  // update_target on an empty slot (matrix.rs:75-82)
    const pg_mod_route& r = p.routes[s][t];
    if (fabsf(r.amount) >= 0.001f) { m.amount[s][t] = r.amount; m.bipolar[s][t] = r.bipolar ? 1 : 0; }
  }
  m.velocity = 0.0f; m.note_pitch = 60.0f / 127.0f;
}
int pg_graph_set_voice_modulation_matrix(pg_graph* g, int voice_id, const pg_modulation_params* p) {
  { const int rc = pg_modulation_params_check(p); if (rc) return rc; }
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (voice_kind(g, voice_id) == VOICE_DEAD) return set_error(PG_ERR_NOT_FOUND, "Source with id %d not found", voice_id);
  drain_control_messages(g);
  if (g->voices[voice_id].mixer < 0) return set_error(PG_ERR_NOT_FOUND, "Source with id %d not found", voice_id);
  HostVoice& hv = g->voices[voice_id];
  if (hv.gran < 0) return set_error(PG_ERR_NOT_FOUND, "Source with id %d is not a granular voice", voice_id);
  // the matrix is created with the voice and note_on belongs to its start (voice.rs:341-373, :181-184)
  if (voice_has_rendered(g, hv)) return set_error(PG_ERR_STATE, "Source with id %d has rendered frames already: the modulation matrix is attached before the voice starts", voice_id);
  if (graph_quiesce(g)) return graph_fail(g, PG_ERR_DEVICE);
  PgGrainMod m;
  mod_matrix_init(m, *p, g->sample_rate, p->lfo[0].rng_state, p->lfo[1].rng_state);
  // the voice's note is known here: SamplerVoiceModulationState::start(note, velocity) = ModulationMatrix::note_on (matrix.rs:394-408)
  for (int l = 0; l < 2; ++l) mod_lfo_reset(m.lfo[l]);
  m.velocity = p->velocity;
  m.note_pitch = (float)p->note / 127.0f;
  (void)hipSetDevice(g->device);
  HIP_TRY(pg_memcpy((char*)(g->d_gran + hv.gran) + offsetof(PgGrainVoice, mod), &m, sizeof m, hipMemcpyHostToDevice));
  hv.mod = true;
  g->voice_alive_tab.set((size_t)voice_id, VOICE_GRANULAR_MOD);
  return PG_OK;
}
// The timed calls: records in the control ring like the other voice commands; the writing thread turns them into events of the voice's mixer.
int pg_graph_set_voice_modulation(pg_graph* g, int voice_id, int source, int target, float amount, int bipolar, uint64_t sample_time) {
  { const int rc = mod_check_route(source, target, amount); if (rc) return rc; }
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  const bool keep = fabsf(amount) >= 0.001f;   // update_target's threshold (matrix.rs:61): below it the route is removed, or not added
  return voice_message(g, voice_id, VOICE_GRANULAR_MOD, pgc::CT_VOICE_MOD_ROUTE, sample_time, keep ? amount : 0.0f, source | (target << 8) | ((keep && bipolar) ? 1 << 16 : 0));
}
int pg_graph_clear_voice_modulation(pg_graph* g, int voice_id, int source, int target, uint64_t sample_time) {  // set_modulation(.., 0.0, false) (state.rs:223-231)
  return pg_graph_set_voice_modulation(g, voice_id, source, target, 0.0f, 0, sample_time);
}
int pg_graph_set_voice_lfo_rate(pg_graph* g, int voice_id, int lfo, float rate_hz, uint64_t sample_time) {
  if (lfo < 0 || lfo > 1) return set_error(PG_ERR_PARAMETER, "Invalid LFO index: %d", lfo);
  if (rate_hz != rate_hz) return set_error(PG_ERR_PARAMETER, "LFO %d rate is not a number", lfo + 1);
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  return voice_message(g, voice_id, VOICE_GRANULAR_MOD, pgc::CT_VOICE_LFO_RATE, sample_time, mod_clamp_rate(rate_hz), lfo);
}
int pg_graph_set_voice_lfo_waveform(pg_graph* g, int voice_id, int lfo, int waveform, uint64_t sample_time) {
  if (lfo < 0 || lfo > 1) return set_error(PG_ERR_PARAMETER, "Invalid LFO index: %d", lfo);
  if (waveform < 0 || waveform > 6) return set_error(PG_ERR_PARAMETER, "Invalid LFO %d waveform: %d", lfo + 1, waveform);
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  return voice_message(g, voice_id, VOICE_GRANULAR_MOD, pgc::CT_VOICE_LFO_WAVEFORM, sample_time, 0.0f, lfo | (waveform << 8));
}
int pg_graph_voice_modulation_state(pg_graph* g, int voice_id, pg_modulation_state* out) {
  if (!g || !out) return set_error(PG_ERR_PARAMETER, "graph handle or output is null");
  if (voice_id < 0 || voice_id >= (int)g->voices.size() || g->voices[voice_id].gran < 0) return set_error(PG_ERR_NOT_FOUND, "Source with id %d is not a granular voice", voice_id);
  const HostVoice* hv = &g->voices[voice_id];
  if (!hv->mod) return set_error(PG_ERR_STATE, "Source with id %d has no modulation matrix", voice_id);
  return modulation_state_read(g, hv->gran, out);
}

}  // extern "C"

// ---- samplers: the note, voice-allocation and stealing layer of Sampler (src/generator/sampler.rs) for file playback. The layer itself runs on the
// device (pg_sampler_dev.h, in pg_unit_kernel's command loop); here: construction, the message -> event -> command path, removal, the read-back ----
static_assert(PG_SAMPLER_MAX_VOICES == 64, "the header's and the device's pool size agree (the header defines the same macro)");
static HostSampler* sampler_find(pg_graph* g, int sampler_id) {   // owner thread: the sampler while it lives, else null (PG_ERR_NOT_FOUND is set)
  if (sampler_id < 0 || sampler_id >= (int)g->samplers.size() || !g->samplers[sampler_id].alive) { set_error(PG_ERR_NOT_FOUND, "Sampler with id %d not found", sampler_id); return nullptr; }
  return &g->samplers[sampler_id];
}
// The pool leaves its mixer (RemoveSource, a mixer that drops an exhausted generator: mixed.rs:612-616): its voices are retired like removed
// sources — their buffer references return when their memory is released — and what is still queued for it finds no source when it comes due
static void sampler_retire(pg_graph* g, int sampler_id) {
  HostSampler& hs = g->samplers[sampler_id];
  HostMixer& mx = g->mixers[hs.mixer];
  for (int k = 0; k < hs.n_voices; ++k) {
    const int v = hs.voice_id_slot0 - k;
    if (g->voices[v].mixer < 0) continue;
    mx.voices.erase(std::remove(mx.voices.begin(), mx.voices.end(), v), mx.voices.end());
    g->voices[v].mixer = -1;
    g->retired_voices.push_back(v);
  }
  for (Event& e : mx.events) if ((pg_cmd_is_sampler_message(e.cmd.type) || pg_cmd_is_sampler_output(e.cmd.type)) && e.cmd.target == hs.rec) { e.cmd.type = CMD_NOP; e.cmd.target = 0; }
  if (hs.unit >= 0) {   // a source of the main mixer is gone: a granular pool's voices all counted as live ones, a file pool's as their notes had it — the next count says
    g->n_main_samplers -= 1;
    if (hs.granular) g->main_active_voices = std::max(0, g->main_active_voices - hs.n_voices);
  }
  hs.alive = false;
  if (hs.granular) g->gsamp_dirty = true;
  g->sampler_alive_tab.set((size_t)sampler_id, 0);
  g->topo_dirty = true;
}
void samplers_of_removed_mixers(pg_graph* g) {
  for (size_t i = 0; i < g->samplers.size(); ++i)
    if (g->samplers[i].alive && g->mixers[g->samplers[i].mixer].removed) { g->samplers[i].alive = false; g->sampler_alive_tab.set(i, 0); if (g->samplers[i].granular) g->gsamp_dirty = true; }
}
// Transient samplers whose `stopped` word the exact kernel has set: the mixer drops them (reads mapped host words: no wait)
static void samplers_poll_stopped(pg_graph* g) {
  for (size_t i = 0; i < g->samplers.size(); ++i) {
    const HostSampler& hs = g->samplers[i];
    if (hs.alive && hs.transient && g->samp_stopped[(size_t)hs.rec] != 0) sampler_retire(g, (int)i);
  }
}
// Room for `n` records, their `stopped` words and the header; speed_from_note's table with the first sampler. The graph is quiescent. A failure
// leaves the graph on its old records.
static int graph_samp_reserve(pg_graph* g, size_t n) {
  if (!g->d_speed_tab) {
    double tab[256];   // speed_from_note (utils.rs:67-78): pitch_from_note(n) / pitch_from_note(60), pitch = 440 * 2^((n - 69) / 12)
    for (int i = 0; i < 256; ++i) tab[i] = (440.0 * std::pow(2.0, ((double)i - 69.0) / 12.0)) / (440.0 * std::pow(2.0, (60.0 - 69.0) / 12.0));
    HIP_TRY(pg_malloc((void**)&g->d_speed_tab, sizeof tab));
    HIP_TRY(pg_memcpy(g->d_speed_tab, tab, sizeof tab, hipMemcpyHostToDevice));
  }
  if (n <= g->samp_cap) return PG_OK;
  const size_t cap = std::max<size_t>(next_pow2(n), 4);
  PgSamplerTab* nt = nullptr;
  MappedWords stopped;
  HIP_TRY(pg_malloc((void**)&nt, sizeof(PgSamplerTab) + cap * sizeof(PgSamplerRec)));
  if (pg_memset(nt, 0, sizeof(PgSamplerTab) + cap * sizeof(PgSamplerRec)) != hipSuccess || stopped.reserve(cap, g->samp_stopped) ||
      (g->d_samp && pg_memcpy(nt + 1, g->d_samp + 1, g->samplers.size() * sizeof(PgSamplerRec), hipMemcpyDeviceToDevice) != hipSuccess)) {
    (void)pg_free(nt); stopped.release();
    return set_error(PG_ERR_DEVICE, "sampler table allocation failed");
  }
  if (g->d_samp) (void)pg_free(g->d_samp);
  g->samp_stopped.release();
  g->d_samp = nt; g->samp_stopped = stopped; g->samp_cap = cap;
  return PG_OK;
}
static hipError_t samp_head_upload(const pg_graph* g, size_t n) {
  PgSamplerTab head;
  memset(&head, 0, sizeof head);
  head.n = (uint32_t)n; head.speed_tab = g->d_speed_tab; head.stopped = g->samp_stopped.d; head.gsamp = g->d_gsamp;
  return pg_memcpy(g->d_samp, &head, sizeof head, hipMemcpyHostToDevice);
}

// The timed sampler messages — each becomes an event of the sampler's mixer — with the command a message turns into and what the command carries
// (pg_dev.h: PgCmdType). The ONE list of them: sampler_drain_message builds the events from it.
struct SamplerEvent { int32_t msg, cmd; void (*fill)(const pgc::CtrlMsg& m, PgCmd& c); };
static const SamplerEvent SAMPLER_EVENTS[] = {
  {pgc::CT_SAMPLER_NOTE_ON, CMD_SAMPLER_NOTE_ON, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; c.value = m.value; c.value64 = pg_note_on_pack((int)m.dvalue, m.value2); }},
  {pgc::CT_SAMPLER_NOTE_OFF, CMD_SAMPLER_NOTE_OFF, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; }},
  {pgc::CT_SAMPLER_ALL_NOTES_OFF, CMD_SAMPLER_ALL_NOTES_OFF, [](const pgc::CtrlMsg&, PgCmd&) {}},
  {pgc::CT_SAMPLER_NOTE_SPEED, CMD_SAMPLER_NOTE_SPEED, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; c.value = m.value; memcpy(&c.value64, &m.dvalue, 8); }},
  {pgc::CT_SAMPLER_NOTE_VOLUME, CMD_SAMPLER_NOTE_VOLUME, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; c.value = m.value; }},
  {pgc::CT_SAMPLER_NOTE_PAN, CMD_SAMPLER_NOTE_PAN, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; c.value = m.value; }},
  {pgc::CT_SAMPLER_PARAM, CMD_SAMPLER_PARAM, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; c.value = m.value; }},   // (the pitch factor: sampler_stage_command)
  {pgc::CT_SAMPLER_STOP, CMD_SAMPLER_STOP, [](const pgc::CtrlMsg&, PgCmd&) {}},
  {pgc::CT_SAMPLER_GRAIN_PARAM, CMD_SAMPLER_GRAIN_PARAM, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; c.value = m.value; }},
  {pgc::CT_SAMPLER_ENV_PARAM, CMD_SAMPLER_ENV_PARAM, [](const pgc::CtrlMsg& m, PgCmd& c) { c.param = m.param; c.value = m.value; }},   // (the field it changes: sampler_stage_command)
  // the words of the lone voices' commands of the same name (pg_host.hip: VOICE_EVENTS); the call has turned an LFO's rate into its phase increment
  {pgc::CT_SAMPLER_MOD_ROUTE, CMD_SAMPLER_MOD_ROUTE, [](const pgc::CtrlMsg& m, PgCmd& c) { c.value = m.value; c.value64 = (uint64_t)(uint32_t)m.param; }},
  {pgc::CT_SAMPLER_LFO_RATE, CMD_SAMPLER_LFO_RATE, [](const pgc::CtrlMsg& m, PgCmd& c) { c.value = m.value; c.value64 = (uint64_t)(uint32_t)m.param; }},
  {pgc::CT_SAMPLER_LFO_WAVEFORM, CMD_SAMPLER_LFO_WAVEFORM, [](const pgc::CtrlMsg& m, PgCmd& c) { c.value64 = (uint64_t)(uint32_t)m.param; }},
  {pgc::CT_SAMPLER_GRAIN_LOOP, CMD_SAMPLER_GRAIN_LOOP, [](const pgc::CtrlMsg& m, PgCmd& c) { uint32_t end; memcpy(&end, &m.value2, 4); c.value = m.value; c.value64 = (uint64_t)(m.param & 1) | ((uint64_t)end << 32); }},
  // the generator's output stage of a main-mixer sampler: events of the main mixer like a voice's SetSourceVolume / SetSourcePanning
  {pgc::CT_SAMPLER_OUT_VOLUME, CMD_SAMPLER_OUT_VOLUME, [](const pgc::CtrlMsg& m, PgCmd& c) { c.value = m.value; }},
  {pgc::CT_SAMPLER_OUT_PAN, CMD_SAMPLER_OUT_PAN, [](const pgc::CtrlMsg& m, PgCmd& c) { c.value = m.value; }},
};
bool sampler_drain_message(pg_graph* g, const pgc::CtrlMsg& m) {
  if (m.type < pgc::CT_SAMPLER_NOTE_ON || m.type > pgc::CT_SAMPLER_OUT_PAN) return false;
  if (m.id < 0 || m.id >= (int)g->samplers.size() || !g->samplers[m.id].alive) return true;   // gone in the meantime: dropped
  if (m.type == pgc::CT_SAMPLER_REMOVE) { sampler_retire(g, m.id); return true; }
  const HostSampler& hs = g->samplers[m.id];
  for (const SamplerEvent& se : SAMPLER_EVENTS) if (se.msg == m.type) {
    PgCmd c;
    memset(&c, 0, sizeof c);
    c.type = se.cmd; c.target = hs.rec;
    se.fill(m, c);
    // The mixer does not call a source before its start time (mixed.rs:565-576); a trigger that comes due earlier only goes into the generator's
    // queue (mixed.rs:902-918), and the sampler drains that queue at the top of its first write, whose first frame is `now` for all of them
    // (sampler.rs:656-731). So such a message becomes an event AT the start time, ordered among those by the time it was stamped with and
    // then by sending order, as the mixer would have queued them. The mixer still cuts its chunk where the message came due: a no-op event.
    if (m.sample_time < hs.start_time) {
      PgCmd nop;
      memset(&nop, 0, sizeof nop);
      nop.type = CMD_NOP;
      push_event(g, hs.mixer, m.sample_time, nop);
      push_event(g, hs.mixer, hs.start_time, c, m.sample_time);
    } else push_event(g, hs.mixer, m.sample_time, c);
    break;
  }
  return true;
}
// The pitch factor of a base-pitch command is 2^(transpose / 12 + finetune / 1200) of the pair that holds once the command is applied
// (voice.rs:144-148), with this host's libm. Messages may be sent out of time order, so the pair is tracked here, where a mixer's events leave its
// sorted list one by one.
//
// An envelope command is resolved here for the same reason: AhdsrParameters' setters are not independent (ahdsr.rs:143-249). set_sustain_level
// stores the level and leaves decay_rate alone; set_decay_time divides (1 - sustain_level) as it holds THEN; a zero time is a rate of f32::MAX.
// The command gets the one field its setter writes and the zero times that hold behind it.
// Duration::from_secs_f32(seconds).as_secs_f32() (sampler.rs:191-208): nanoseconds rounded to nearest, ties to even, then
// `secs as f32 + nanos as f32 / 1e9f32`. The rounding rule is how the standard library's documentation describes try_from_secs_f32; it is
// UNVERIFIED against the library's source, which this project does not hold. f32 x 1e9 is exact in f64 (24 + 21 bits).
static float duration_round_trip(float seconds, bool& is_zero) {
  const uint64_t total = (uint64_t)std::nearbyint((double)(seconds > 0.0f ? seconds : 0.0f) * 1e9);
  is_zero = total == 0;
  return (float)(total / 1000000000ull) + (float)(uint32_t)(total % 1000000000ull) / 1e9f;
}
static void sampler_stage_envelope(pg_graph* g, PgCmd& c) {
  if (c.target < 0 || c.target >= (int)g->samplers.size()) return;
  PgEnvParams& p = g->samplers[c.target].env;
  const float sr = (float)g->sample_rate;
  if (c.param == PG_SE_SUSTAIN) p.sustain_level = c.value;
  else {
    bool zero = false;
    const float secs = duration_round_trip(c.value, zero);
    int bit = 0;
    if (c.param == PG_SE_ATTACK) c.value = p.attack_rate = secs == 0.0f ? FLT_MAX : 1.0f / (secs * sr);
    else if (c.param == PG_SE_HOLD) { c.value = p.hold_samples = secs * sr; bit = PG_AHDSR_HOLD_ZERO; }
    else if (c.param == PG_SE_DECAY) { c.value = p.decay_rate = zero ? FLT_MAX : (1.0f - p.sustain_level) / (secs * sr); bit = PG_AHDSR_DECAY_ZERO; }
    else if (c.param == PG_SE_RELEASE) { c.value = p.release_rate = secs == 0.0f ? FLT_MAX : 1.0f / (secs * sr); bit = PG_AHDSR_RELEASE_ZERO; }
    p.zero_times = (p.zero_times & ~bit) | (zero ? bit : 0);
  }
  c.value64 = (uint64_t)(uint32_t)p.zero_times;
}
void sampler_stage_command(pg_graph* g, PgCmd& c) {
  if (c.type == CMD_SAMPLER_ENV_PARAM) { sampler_stage_envelope(g, c); return; }
  if (c.type != CMD_SAMPLER_PARAM || (c.param != PG_SP_TRANSPOSE && c.param != PG_SP_FINETUNE)) return;
  for (HostSampler& hs : g->samplers) if (hs.rec == c.target) {
    if (c.param == PG_SP_TRANSPOSE) hs.transpose = (int)c.value; else hs.finetune = (int)c.value;
    const double pitch_factor = std::pow(2.0, (double)hs.transpose / 12.0 + (double)hs.finetune / 1200.0);
    memcpy(&c.value64, &pitch_factor, 8);
    return;
  }
}
// ---- the message calls' one path (any thread): what a call must know of the sampler stands in sampler_alive_tab / sampler_frames_tab ----
// The sampler's SAMPLER_TAB_* word while it takes messages; 0: PG_ERR_PARAMETER (null handle) or PG_ERR_NOT_FOUND is set ...
static int sampler_tab_word(pg_graph* g, int sampler_id) {
  if (!g) { set_error(PG_ERR_PARAMETER, "graph handle is null"); return 0; }
  if (sampler_id < 0 || (size_t)sampler_id >= g->sampler_alive_tab.size() || !g->sampler_alive_tab.get((size_t)sampler_id)) { set_error(PG_ERR_NOT_FOUND, "Sampler with id %d not found", sampler_id); return 0; }
  return g->sampler_alive_tab.get((size_t)sampler_id);
}
static int sampler_tab_error(const pg_graph* g) { return g ? PG_ERR_NOT_FOUND : PG_ERR_PARAMETER; }   // ... and the code it set
// One message for a sampler that takes messages into the control ring. `param`: a note id as note_param narrows it, or the call's own word.
static int sampler_message(pg_graph* g, int sampler_id, int type, uint64_t sample_time, int param = 0, float value = 0.0f, float value2 = 0.0f, double dvalue = 0.0) {
  if (!sampler_tab_word(g, sampler_id)) return sampler_tab_error(g);
  pgc::CtrlMsg m;
  memset(&m, 0, sizeof m);
  m.type = type; m.id = sampler_id; m.param = param; m.value = value; m.value2 = value2; m.dvalue = dvalue; m.sample_time = sample_time;
  if (!g->ctrl.push(m)) return set_error(PG_ERR_QUEUE_FULL, "mixer's message queue is full");
  return PG_OK;
}
// A note id as a message carries it: one this graph never handed out plays nowhere, and 0 is no note's id
static int note_param(int64_t note_id) { return (note_id > 0 && note_id <= INT32_MAX) ? (int32_t)note_id : 0; }
// The sampler behind `sampler_id` for a read-back (owner thread): while it lives, and a transient one that has stopped — it keeps its records, so
// the state that says so stays readable until the id is removed or its mixer goes. Else null (PG_ERR_NOT_FOUND is set).
static const HostSampler* sampler_for_readback(pg_graph* g, int sampler_id) {
  if (sampler_id < 0 || sampler_id >= (int)g->samplers.size() || (!g->samplers[sampler_id].alive && !(g->samplers[sampler_id].transient && g->samp_stopped[(size_t)sampler_id] != 0))) {
    set_error(PG_ERR_NOT_FOUND, "Sampler with id %d not found", sampler_id);
    return nullptr;
  }
  return &g->samplers[sampler_id];
}

// ---- a pool's construction: what pg_graph_add_sampler and pg_graph_add_granular_sampler share, in three steps with each kind's own work between them ----
// 1. The checks, in the order the calls make them: the options, a granular sampler's own options, the generator's options (`to_main`: the entry
// points that place the sampler on the main mixer; gen null = the defaults), the handle, the mixer, the buffer, the loop range.
static int sampler_pool_check(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt, bool granular, const pg_granular_sampler_options* gopt, bool to_main, const pg_generator_options* gen) {
  { const int rc = pg_sampler_options_check(opt); if (rc) return rc; }
  if (granular) { const int rc = pg_granular_sampler_options_check(gopt); if (rc) return rc; }
  if (to_main && gen) { const int rc = pg_generator_options_check(gen); if (rc) return rc; }
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  if (!to_main && mixer_id == PG_MAIN_MIXER) return set_error(PG_ERR_PARAMETER, "A sampler needs a sub-mixer: every source of the main mixer is a unit and a workgroup of its own, %s",
                                                  granular ? "the pool is one source of one mixer" : "the pool needs one workgroup that sees all of its voices");
  if (mixer_id < 0 || mixer_id >= (int)g->mixers.size() || g->mixers[mixer_id].removed) return set_error(PG_ERR_NOT_FOUND, "Mixer with id %d not found", mixer_id);
  const SampleBuffer* sb = sample_buffer_find(g, buffer_id);
  if (!sb) return PG_ERR_NOT_FOUND;
  if (opt->has_loop_range && (opt->loop_start >= sb->n_frames || opt->loop_end > sb->n_frames)) return set_error(PG_ERR_PARAMETER, "Invalid loop range: %llu..%llu not in range 0..%zu", (unsigned long long)opt->loop_start, (unsigned long long)opt->loop_end, sb->n_frames);
  return PG_OK;
}
// What every pool voice is added with: a source its mixer keeps, from the sampler's start time on
static pg_voice_options sampler_pool_voice_options(const pg_sampler_options* opt) {
  pg_voice_options vo;
  pg_voice_options_default(&vo);
  vo.non_transient = 1; vo.start_time = opt->start_time;
  return vo;
}
// 2. `n` copies of the caller's voice record `v` at consecutive device indices from *voice0 on, room for them in the envelope table; the device is
// set for the uploads that follow. A failure is the graph's.
static int sampler_pool_push(pg_graph* g, const PgVoice& v, int n, int* voice0) {
  for (int k = 0; k < n; ++k) {
    int di = -1;
    const int rc = g->d_voices.push(v, &di);
    if (rc || (k > 0 && di != *voice0 + k)) return graph_fail(g, rc ? rc : set_error(PG_ERR_STATE, "pool voices are not contiguous"));
    if (k == 0) *voice0 = di;
  }
  if (graph_env_reserve(g, std::max<size_t>(g->voices.size() + (size_t)n, (size_t)(*voice0 + n)))) return graph_fail(g, PG_ERR_DEVICE);
  (void)hipSetDevice(g->device);
  return PG_OK;
}
// The note layer's record before any note: the file sampler's PgSamplerRec, the granular one's PgGSampler::note
static void note_rec_init(PgSamplerRec& r, int unit, int voice0, int n, const pg_sampler_options* opt) {
  memset(&r, 0, sizeof r);
  r.unit = unit; r.voice0 = voice0; r.n_voices = n; r.has_envelope = opt->has_envelope ? 1 : 0; r.transient = opt->transient ? 1 : 0;
  r.base_volume = 1.0f; r.base_panning = 0.0f; r.pitch_factor = std::pow(2.0, 0.0 / 12.0 + 0.0 / 1200.0);
  for (int k = 0; k < PG_SAMPLER_MAX_VOICES; ++k) { r.slots[k].release_start_frame = UINT64_MAX; r.slots[k].note = 60; r.slots[k].note_volume = 1.0f; }   // SamplerVoice::new (voice.rs:51-55)
}
// 3. The records are on the device: the sampler's place in the graph. `hs` arrives with what is its kind's (a granular sampler's grain records),
// `tab_kind` with its kind's SAMPLER_TAB_* bits, `stages` with a granular sampler's staging buffers, one per slot: each passes to its slot's voice,
// and a failure frees those no voice owns yet. Returns the sampler's id (< 0: -PG_ERR_*).
// `unit`: the source unit of a sampler on the main mixer, which every voice of the pool maps to (graph_new_sampler_unit); -1 in a sub-mixer.
static int sampler_pool_register(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt, const pg_voice_options& vo, int voice0, HostSampler hs, int tab_kind, std::vector<void*>* stages, int unit) {
  const int n = (int)opt->voice_count, sampler_id = (int)g->samplers.size();
  const SampleBuffer& sb = g->sample_buffers[buffer_id];
  g->samp_stopped[(size_t)sampler_id] = 0;
  hs.mixer = mixer_id; hs.rec = sampler_id; hs.n_voices = n; hs.unit = unit; hs.has_envelope = opt->has_envelope != 0; hs.transient = opt->transient != 0; hs.start_time = opt->start_time;
  // the mixer's list inserts a new source in FRONT of those with the same start time (mixed.rs:324-329): the last slot goes in first, so that the
  // mixer — and the kernel that sums the pool — meets it in slot order (sampler.rs:989-1006)
  for (int k = n - 1; k >= 0; --k) {
    HostVoice hv;
    hv.sbuf = buffer_id; hv.sampler = sampler_id;
    if (stages) { hv.d_stage = (*stages)[(size_t)k]; (*stages)[(size_t)k] = nullptr; }   // (the voice owns it from here on)
    hv.file_channels = sb.channels; hv.file_rate = sb.rate; hv.file_samples = (uint64_t)sb.n_frames * sb.channels;
    g->sample_buffers[buffer_id].use_count += 1;
    const int id = graph_register_voice(g, mixer_id, voice0 + k, &vo, hv, VOICE_DEAD, unit);   // (VOICE_DEAD: the id takes none of the public voice calls)
    if (id < 0) { if (stages) for (void* p : *stages) if (p) (void)pg_free(p); return id; }
    if (k == 0) hs.voice_id_slot0 = id;
  }
  if (opt->has_envelope) hs.env = ahdsr_build_params(opt->envelope, g->sample_rate);
  g->samplers.push_back(hs);
  if (hs.granular) { g->n_gsamplers += 1; g->gsamp_dirty = true; }
  if (unit >= 0) g->n_main_samplers += 1;
  if (!g->sampler_frames_tab.append((uint64_t)sb.n_frames) || !g->sampler_alive_tab.append((int8_t)(tab_kind | (opt->has_envelope ? SAMPLER_TAB_ENVELOPE : 0) | (unit >= 0 ? SAMPLER_TAB_MAIN : 0)))) return -set_error(PG_ERR_STATE, "too many samplers");
  return sampler_id;
}

extern "C" {

void pg_sampler_options_default(pg_sampler_options* o) {   // GeneratorPlaybackOptions / Sampler::new (generator.rs:48-72): 8 voices, no envelope, not transient
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->voice_count = 8;
  pg_ahdsr_params_default(&o->envelope);
}
int pg_sampler_options_check(const pg_sampler_options* o) {
  if (!o) return set_error(PG_ERR_PARAMETER, "sampler options must not be null");
  if (o->voice_count < 1 || o->voice_count > PG_SAMPLER_MAX_VOICES) return set_error(PG_ERR_PARAMETER, "Invalid voice count: %u. Must be in range [1, %d]", o->voice_count, PG_SAMPLER_MAX_VOICES);
  if (o->has_envelope) { const int rc = pg_ahdsr_params_check(&o->envelope); if (rc) return rc; }
  if (o->has_loop_range && o->loop_start >= o->loop_end) return set_error(PG_ERR_PARAMETER, "Invalid loop range: %llu..%llu", (unsigned long long)o->loop_start, (unsigned long long)o->loop_end);
  return PG_OK;
}
int pg_sampler_param_count(void) { return PG_SP_COUNT; }
int pg_sampler_param(int index, pg_param_desc* out) {   // Sampler::base_parameters() (sampler.rs:120-127)
  if (!out) return set_error(PG_ERR_PARAMETER, "output is null");
  if (index < 0 || index >= PG_SP_COUNT) return set_error(PG_ERR_NOT_FOUND, "no such parameter");
  param_desc_from_spec(SAMPLER_PARAMS[index], out);
  return PG_OK;
}
// pg_graph_add_sampler (a sub-mixer's pool) and pg_graph_add_sampler_to_main (`to_main`: mixer_id is PG_MAIN_MIXER; the pool is ONE source unit
// of the main mixer, behind the generator's output stage with `gen`'s volume and panning — null: the defaults)
static int add_file_sampler(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt, bool to_main, const pg_generator_options* gen) {
  pg_sampler_options def;
  if (!opt) { pg_sampler_options_default(&def); opt = &def; }
  { const int rc = sampler_pool_check(g, mixer_id, buffer_id, opt, false, nullptr, to_main, gen); if (rc) return -rc; }
  drain_control_messages(g);
  if (graph_quiesce(g)) return -graph_fail(g, PG_ERR_DEVICE);
  const SampleBuffer sb = g->sample_buffers[buffer_id];
  const int n = (int)opt->voice_count, sampler_id = (int)g->samplers.size();
  // a pool voice: PreloadedFileSource::from_shared_buffer(buffer, FilePlaybackOptions::default().fade_out(50 ms), rate) behind AmplifiedSource(1.0) /
  // PannedSource(0.0) (sampler.rs:505-530, voice.rs:60-65) — a source its mixer keeps, with no note yet: inactive, delivering nothing
  const pg_voice_options vo = sampler_pool_voice_options(opt);
  PgVoice v;
  voice_init_neutral(g, v, &vo, 1.0f, 0.0f);
  v.active = 0;
  v.pcm = (const float*)sb.d_pcm; v.n_samples = (uint64_t)sb.n_frames * sb.channels; v.channels = sb.channels; v.src_rate = sb.rate; v.out_rate = g->sample_rate;
  v.ratio = (float)((double)sb.rate / (double)(uint32_t)d2u64((double)g->sample_rate / 1.0));
  if (!(v.ratio > 0.0f) || v.ratio > 64.0f) return -set_error(PG_ERR_PARAMETER, "Invalid resampling ratio");
  if (opt->has_loop_range) { v.has_loop = 1; v.loop_start = opt->loop_start; v.loop_end = opt->loop_end; v.repeat = PG_USIZE_MAX; }   // SamplerVoice::set_loop_range (voice.rs:313-328)
  else if (sb.has_loop) { v.has_loop = 1; v.loop_start = sb.loop_start; v.loop_end = sb.loop_end; v.repeat = PG_USIZE_MAX; }          // the file's embedded loop (preloaded.rs:89-104)
  v.repeat_count = v.repeat;
  v.fade_out_seconds = 0.05f;
  v.current_speed = 1.0; v.target_speed = 1.0;
  v.sched_class = -1;   // (always on the exact kernel, every note at a speed of its own: no shared resampler schedule)
  if (graph_samp_reserve(g, g->samplers.size() + 1)) return -graph_fail(g, PG_ERR_DEVICE);
  int voice0 = -1;
  { const int rc = sampler_pool_push(g, v, n, &voice0); if (rc) return -rc; }
  if (opt->has_envelope) {
    PgEnv e;
    memset(&e, 0, sizeof e);
    e.on = 1; e.params = ahdsr_build_params(opt->envelope, g->sample_rate);   // (state: Idle until the slot's first note_on)
    std::vector<PgEnv> es((size_t)n, e);
    if (pg_memcpy(g->d_env + voice0, es.data(), es.size() * sizeof(PgEnv), hipMemcpyHostToDevice) != hipSuccess) return -graph_fail(g, set_error(PG_ERR_DEVICE, "sampler upload failed"));
  }
  const int unit = to_main ? graph_new_sampler_unit(g, sampler_id) : -1;
  if (to_main && unit < 0) return -graph_fail(g, PG_ERR_DEVICE);
  std::unique_ptr<PgSamplerRec> r(new PgSamplerRec);
  note_rec_init(*r, to_main ? unit : g->mixers[mixer_id].unit_slot, voice0, n, opt);
  if (to_main) { pg_generator_options go; if (gen) go = *gen; else pg_generator_options_default(&go); genout_init(g, r->out, go.volume, go.panning); }
  if (pg_memcpy((PgSamplerRec*)(g->d_samp + 1) + sampler_id, r.get(), sizeof(PgSamplerRec), hipMemcpyHostToDevice) != hipSuccess || samp_head_upload(g, (size_t)sampler_id + 1) != hipSuccess ||
      graph_env_head_refresh(g)) return -graph_fail(g, set_error(PG_ERR_DEVICE, "sampler upload failed"));
  return sampler_pool_register(g, mixer_id, buffer_id, opt, vo, voice0, HostSampler(), SAMPLER_TAB_FILE, nullptr, unit);
}
int pg_graph_add_sampler(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt) { return add_file_sampler(g, mixer_id, buffer_id, opt, false, nullptr); }
int pg_graph_add_sampler_to_main(pg_graph* g, int buffer_id, const pg_sampler_options* opt, const pg_generator_options* gen) { return add_file_sampler(g, PG_MAIN_MIXER, buffer_id, opt, true, gen); }
void pg_generator_options_default(pg_generator_options* o) {   // GeneratorPlaybackOptions::default (generator.rs:62-78)
  if (!o) return;
  o->volume = 1.0f; o->panning = 0.0f;
}
int pg_generator_options_check(const pg_generator_options* o) {   // GeneratorPlaybackOptions::validate (generator.rs:120-140)
  if (!o) return set_error(PG_ERR_PARAMETER, "generator options must not be null");
  if (o->volume < 0.0f || o->volume != o->volume) return set_error(PG_ERR_PARAMETER, "playback options 'volume' value is '%g'", (double)o->volume);
  if (!(o->panning >= -1.0f && o->panning <= 1.0f)) return set_error(PG_ERR_PARAMETER, "playback options 'panning' value is '%g'", (double)o->panning);
  return PG_OK;
}
// ---- the generator's output stage of a sampler on the main mixer (GeneratorPlaybackHandle::set_volume / set_panning, player/handles/generator.rs:
// 119-196 -> MixerMessage::SetSourceVolume / SetSourcePanning): events of the main mixer, like a voice's. Any thread. ----
static int sampler_output_message(pg_graph* g, int sampler_id, int type, float value, uint64_t sample_time) {
  const int w = sampler_tab_word(g, sampler_id);
  if (!w) return sampler_tab_error(g);
  if (!(w & SAMPLER_TAB_MAIN)) return set_error(PG_ERR_STATE, "Sampler with id %d lives in a sub-mixer: its pool is summed there source by source, so no sum of the sampler exists to scale or pan (see pg_graph_add_sampler_to_main)", sampler_id);
  return sampler_message(g, sampler_id, type, sample_time, 0, value);
}
int pg_graph_sampler_set_volume(pg_graph* g, int sampler_id, float volume, uint64_t sample_time) {
  if (!(volume >= 0.0f) || !std::isfinite(volume)) return set_error(PG_ERR_PARAMETER, "Invalid volume: %g. Must be finite and >= 0", (double)volume);
  return sampler_output_message(g, sampler_id, pgc::CT_SAMPLER_OUT_VOLUME, volume, sample_time);
}
int pg_graph_sampler_set_panning(pg_graph* g, int sampler_id, float panning, uint64_t sample_time) {
  if (!std::isfinite(panning)) return set_error(PG_ERR_PARAMETER, "Invalid panning: %g. Must be finite", (double)panning);
  return sampler_output_message(g, sampler_id, pgc::CT_SAMPLER_OUT_PAN, panning, sample_time);
}
int pg_graph_sampler_output_state(pg_graph* g, int sampler_id, pg_sampler_output_state* out) {
  if (!out) return set_error(PG_ERR_PARAMETER, "output is null");
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  const HostSampler* hs = sampler_for_readback(g, sampler_id);
  if (!hs) return PG_ERR_NOT_FOUND;
  if (hs->unit < 0) return set_error(PG_ERR_STATE, "Sampler with id %d lives in a sub-mixer: its pool is summed there source by source, so it has no output stage (see pg_graph_add_sampler_to_main)", sampler_id);
  PgGenOut o;
  { const int rc = graph_read_back(g, &o, (const char*)((const PgSamplerRec*)(g->d_samp + 1) + hs->rec) + offsetof(PgSamplerRec, out), sizeof o); if (rc) return rc; }
  memset(out, 0, sizeof *out);
  out->volume_current = o.volume.current; out->volume_target = o.volume.target; out->panning_current = o.panning.current; out->panning_target = o.panning.target;
  out->volume_ramping = pgd::sm_need_ramp(o.volume) ? 1 : 0; out->panning_ramping = pgd::sm_need_ramp(o.panning) ? 1 : 0;
  return PG_OK;
}
int pg_graph_remove_sampler(pg_graph* g, int sampler_id) {
  const int rc = sampler_message(g, sampler_id, pgc::CT_SAMPLER_REMOVE, 0);
  if (rc == PG_OK) g->sampler_alive_tab.set((size_t)sampler_id, 0);   // dead for every later call; messages pushed before this one are still delivered
  return rc;
}
int64_t pg_graph_sampler_note_on(pg_graph* g, int sampler_id, uint8_t note, float volume, float panning, uint64_t sample_time) {
  if (!(volume >= 0.0f) || !std::isfinite(volume)) return -set_error(PG_ERR_PARAMETER, "Invalid note volume: %g. Must be finite and >= 0", (double)volume);
  if (!std::isfinite(panning)) return -set_error(PG_ERR_PARAMETER, "Invalid note panning: %g. Must be finite", (double)panning);
  if (!sampler_tab_word(g, sampler_id)) return -sampler_tab_error(g);   // (no id is used up for a sampler that is not there)
  const int64_t note_id = g->next_note_id.fetch_add(1, std::memory_order_relaxed);
  if (note_id > INT32_MAX) return -set_error(PG_ERR_STATE, "note ids are used up");
  const int rc = sampler_message(g, sampler_id, pgc::CT_SAMPLER_NOTE_ON, sample_time, note_param(note_id), volume, panning, (double)note);
  return rc ? -rc : note_id;
}
int pg_graph_sampler_note_off(pg_graph* g, int sampler_id, int64_t note_id, uint64_t sample_time) { return sampler_message(g, sampler_id, pgc::CT_SAMPLER_NOTE_OFF, sample_time, note_param(note_id)); }
int pg_graph_sampler_all_notes_off(pg_graph* g, int sampler_id, uint64_t sample_time) { return sampler_message(g, sampler_id, pgc::CT_SAMPLER_ALL_NOTES_OFF, sample_time); }
int pg_graph_sampler_set_note_speed(pg_graph* g, int sampler_id, int64_t note_id, double speed, float glide, uint64_t sample_time) {
  if (!(speed > 0.0) || !std::isfinite(speed)) return set_error(PG_ERR_PARAMETER, "speed must be > 0");
  return sampler_message(g, sampler_id, pgc::CT_SAMPLER_NOTE_SPEED, sample_time, note_param(note_id), glide > 0.0f ? glide : 0.0f, 0.0f, speed);
}
int pg_graph_sampler_set_note_volume(pg_graph* g, int sampler_id, int64_t note_id, float volume, uint64_t sample_time) {
  if (!(volume >= 0.0f) || !std::isfinite(volume)) return set_error(PG_ERR_PARAMETER, "Invalid note volume: %g. Must be finite and >= 0", (double)volume);
  return sampler_message(g, sampler_id, pgc::CT_SAMPLER_NOTE_VOLUME, sample_time, note_param(note_id), volume);
}
int pg_graph_sampler_set_note_panning(pg_graph* g, int sampler_id, int64_t note_id, float panning, uint64_t sample_time) {
  if (!std::isfinite(panning)) return set_error(PG_ERR_PARAMETER, "Invalid note panning: %g. Must be finite", (double)panning);
  return sampler_message(g, sampler_id, pgc::CT_SAMPLER_NOTE_PAN, sample_time, note_param(note_id), panning);
}
int pg_graph_sampler_set_parameter(pg_graph* g, int sampler_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time) {
  const int pi = find_sampler_param(fourcc);
  if (pi < 0) return set_error(PG_ERR_PARAMETER, "Invalid/unknown sampler parameter 0x%08x", fourcc);
  if (value != value) return set_error(PG_ERR_PARAMETER, "Sampler parameter '%s' is not a number", SAMPLER_PARAMS[pi].name);
  // (this call refuses a normalized value outside 0..1 where the envelope's and the granular parameters' calls clamp it: the difference is kept as it
  // was found — UNVERIFIED against the reference which of the two its handle does)
  if (is_normalized && !(value >= 0.0f && value <= 1.0f)) return set_error(PG_ERR_PARAMETER, "Invalid parameter update: value should be a normalized value, but is: '%g'", (double)value);
  float raw = 0.0f;
  (void)resolve_update(SAMPLER_PARAMS[pi], value, is_normalized != 0, raw);
  return sampler_message(g, sampler_id, pgc::CT_SAMPLER_PARAM, sample_time, pi, raw);
}
int pg_graph_sampler_stop(pg_graph* g, int sampler_id, uint64_t sample_time) { return sampler_message(g, sampler_id, pgc::CT_SAMPLER_STOP, sample_time); }
int pg_graph_sampler_state(pg_graph* g, int sampler_id, pg_sampler_state* out) {
  if (!out) return set_error(PG_ERR_PARAMETER, "output is null");
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  const HostSampler* hs = sampler_for_readback(g, sampler_id);
  if (!hs) return PG_ERR_NOT_FOUND;
  (void)hipSetDevice(g->device);
  if (g->d_voices.flush()) return PG_ERR_DEVICE;   // (pool voices no write has carried to the device yet)
  // The note layer's record (a file sampler's PgSamplerRec is read into q->note) and the two things a slot's state needs besides: whether it is
  // active and where its envelope stands. A granular sampler's record holds both, written by pg_gsampler_kernel; a file sampler's slot is active
  // as its voice says — SamplerVoice::is_active (pg_sampler_dev.h: sampler_slot_active) — and its envelope is its voice's PgEnv.
  std::unique_ptr<PgGSampler> q(new PgGSampler);
  std::vector<PgVoice> vs;
  std::vector<PgEnv> es;
  if (hs->granular) { const int rc = graph_read_back(g, q.get(), g->d_gsamp + hs->rec, sizeof(PgGSampler)); if (rc) return rc; }
  else {
    vs.resize((size_t)hs->n_voices); es.resize((size_t)hs->n_voices);
    { const int rc = graph_read_back(g, &q->note, (const PgSamplerRec*)(g->d_samp + 1) + hs->rec, sizeof(PgSamplerRec)); if (rc) return rc; }
    { const int rc = graph_read_back(g, vs.data(), g->d_voices.d + q->note.voice0, vs.size() * sizeof(PgVoice)); if (rc) return rc; }
    if (hs->has_envelope) { const int rc = graph_read_back(g, es.data(), g->d_env + q->note.voice0, es.size() * sizeof(PgEnv)); if (rc) return rc; }
  }
  const PgSamplerRec& r = q->note;
  memset(out, 0, sizeof *out);
  out->voice_count = hs->n_voices; out->stopping = r.stopping; out->stopped = r.stopped;
  out->transpose = r.transpose; out->finetune = r.finetune; out->volume = r.base_volume; out->panning = r.base_panning;
  for (int k = 0; k < hs->n_voices; ++k) {
    const bool active = hs->granular ? q->active[k] != 0 : (vs[(size_t)k].active != 0 && vs[(size_t)k].finished == 0);
    pg_sampler_slot_state& o = out->slots[k];
    o.note_id = active ? (int64_t)r.slots[k].note_id : 0;
    o.release_start_frame = active ? r.slots[k].release_start_frame : UINT64_MAX;   // SamplerVoice::reset clears it (voice.rs:234-235)
    o.note = r.slots[k].note; o.note_volume = r.slots[k].note_volume; o.note_panning = r.slots[k].note_panning;
    o.envelope_stage = !hs->has_envelope ? -1 : hs->granular ? (int)q->env[k].stage : (int)es[(size_t)k].state.stage;
    out->active_voices += active ? 1 : 0;
  }
  return PG_OK;
}

}  // extern "C"

// ---- granular-mode samplers: Sampler::with_granular_playback (src/generator/sampler.rs:598-637). The note layer runs on the device in a kernel
// of its own (pg_k_gsampler.hip, pg_gsampler_dev.h) between the grain launches of consecutive Sampler::write spans; here: construction, the
// span grid, the launches, the granular-parameter message, the read-backs ----
bool graph_has_gsamplers(const pg_graph* g) { return !g->gsamp_live.empty(); }
// The living granular samplers and their slots' grain records -> the launch lists (inside write: capacity was reserved with the samplers)
int graph_gsampler_upload_live(pg_graph* g, hipStream_t stream) {
  g->gsamp_live.clear(); g->gsamp_grains.clear();
  for (const HostSampler& hs : g->samplers) {
    if (!hs.alive || !hs.granular) continue;
    g->gsamp_live.push_back(hs.rec);
    for (int k = 0; k < hs.n_voices; ++k) g->gsamp_grains.push_back(hs.grain0 + k);
  }
  g->gsamp_dirty = false;   // (a failure is the graph's: it renders nothing from then on)
  const int rc = g->d_gsamp_live.upload_async(g->gsamp_live, stream);
  return rc ? rc : g->d_gsamp_grains.upload_async(g->gsamp_grains, stream);
}
void graph_gsampler_cuts(const pg_graph* g, uint64_t now, uint64_t chunk_n, std::vector<uint64_t>& cuts) {
  const uint64_t end = now + chunk_n;
  for (const HostSampler& hs : g->samplers) {
    if (!hs.alive || !hs.granular) continue;
    if (hs.start_time > now && hs.start_time < end) cuts.push_back(hs.start_time);
    // every event of the sampler's mixer ends a call of its sources, every event of an ancestor a call of the mixer itself (mixed.rs:679-712);
    // the main mixer's events bound the chunk
    for (int m = hs.mixer; m != 0; m = g->mixers[m].parent)
      for (const Event& e : g->mixers[m].events) { if (e.sample_time >= end) break; if (e.sample_time > now) cuts.push_back(e.sample_time); }
  }
  std::sort(cuts.begin(), cuts.end());
  cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
}
int launch_gsampler_boundary(pg_graph* g, uint64_t t, uint32_t frame, const PgCmd* d_cmds, int n_cmds, uint64_t chunk_t0, bool chunk_first, bool closing, hipStream_t stream) {
  if (g->gsamp_live.empty()) return PG_OK;
  PgGSamplerLaunch L;
  memset(&L, 0, sizeof L);
  L.recs = g->d_gsamp; L.live = g->d_gsamp_live.d; L.n_recs = (uint32_t)g->gsamp_cap; L.n_live = (uint32_t)g->gsamp_live.size();
  L.n_grains = (uint32_t)g->gran_n; L.grains = g->d_gran; L.cmds = d_cmds; L.n_cmds = d_cmds ? n_cmds : 0; L.frame = frame; L.t = t; L.chunk_t0 = chunk_t0;
  L.chunk_first = chunk_first ? 1 : 0; L.closing = closing ? 1 : 0; L.speed_tab = g->d_speed_tab; L.stopped = g->samp_stopped.d;
  HIP_TRY(pg_launch_gsampler(L, stream));
  return PG_OK;
}
int launch_gsampler_grains(pg_graph* g, uint64_t t0, uint32_t n, uint64_t chunk_t0, hipStream_t stream) {
  if (g->gsamp_grains.empty() || n == 0) return PG_OK;
  return launch_grain_list(g, g->d_gsamp_grains.d, g->gsamp_grains.size(), t0, n, chunk_t0, nullptr, 0, stream);   // (no commands: everything a slot takes is applied at a span's edge, by pg_gsampler_kernel)
}
// Room for `n` records, indexed like the samplers. The graph is quiescent. A failure leaves the graph on its old records.
static int graph_gsamp_reserve(pg_graph* g, size_t n) {
  if (n <= g->gsamp_cap) return PG_OK;
  const size_t cap = std::max<size_t>(next_pow2(n), 4);
  PgGSampler* nt = nullptr;
  HIP_TRY(pg_malloc((void**)&nt, cap * sizeof(PgGSampler)));
  if (pg_memset(nt, 0, cap * sizeof(PgGSampler)) != hipSuccess || (g->d_gsamp && pg_memcpy(nt, g->d_gsamp, g->gsamp_cap * sizeof(PgGSampler), hipMemcpyDeviceToDevice) != hipSuccess)) {
    (void)pg_free(nt);
    return set_error(PG_ERR_DEVICE, "granular sampler table allocation failed");
  }
  if (g->d_gsamp) (void)pg_free(g->d_gsamp);
  g->d_gsamp = nt; g->gsamp_cap = cap;
  return PG_OK;
}
static uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

extern "C" {

void pg_granular_sampler_options_default(pg_granular_sampler_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  pg_granular_params_default(&o->params);
}
int pg_granular_sampler_options_check(const pg_granular_sampler_options* o) {
  if (!o) return set_error(PG_ERR_PARAMETER, "granular sampler options must not be null");
  { const int rc = pg_granular_params_check(&o->params); if (rc) return rc; }
  if (o->modulation) { const int rc = pg_modulation_params_check(o->modulation); if (rc) return rc; }
  return PG_OK;
}
void pg_granular_sampler_rng_state(const uint64_t given[4], uint32_t slot, uint32_t generator, uint64_t out[4]) {
  if (!out) return;
  uint64_t base[4] = {0, 0, 0, 0};
  rng_state_from(given ? given : base, base);
  const uint64_t index = (uint64_t)slot * 3u + (uint64_t)(generator % 3u);
  uint64_t z = (base[0] ^ rotl64(base[1], 16) ^ rotl64(base[2], 32) ^ rotl64(base[3], 48)) + (index + 1u) * 0xD1B54A32D192ED03ull;
  for (int i = 0; i < 4; ++i) out[i] = splitmix64_next(z);
  out[3] = (out[3] & ~0xFFull) | (index & 0xFFull);
  if ((out[0] | out[1] | out[2] | out[3]) == 0) out[0] = 1;
}
// pg_graph_add_granular_sampler and pg_graph_add_granular_sampler_to_main: `to_main` and `gen` as add_file_sampler's
static int add_granular_sampler(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt, const pg_granular_sampler_options* gopt, bool to_main, const pg_generator_options* gen) {
  pg_sampler_options def;
  if (!opt) { pg_sampler_options_default(&def); opt = &def; }
  { const int rc = sampler_pool_check(g, mixer_id, buffer_id, opt, true, gopt, to_main, gen); if (rc) return -rc; }
  { const int rc = pg_graph_prepare_granular_buffer(g, buffer_id); if (rc) return -rc; }   // Sampler::create_granular_sample_buffer, shared by all slots
  drain_control_messages(g);
  if (graph_quiesce(g)) return -graph_fail(g, PG_ERR_DEVICE);
  const SampleBuffer sb = g->sample_buffers[buffer_id];
  const int n = (int)opt->voice_count, sampler_id = (int)g->samplers.size();
  // the pool's loop range: Sampler::set_loop_range (voice.rs:329-338) where the options carry one, else the parameters' own, else the file's
  // embedded one (enable_granular_playback, voice.rs:353-360) — source frames over the FILE's frame count, as f32
  pg_granular_params q = gopt->params;
  const float total = (float)sb.n_frames;
  if (opt->has_loop_range) { q.has_loop_range = 1; q.loop_start = (float)opt->loop_start / total; q.loop_end = (float)opt->loop_end / total; }
  else if (!q.has_loop_range && sb.has_loop) { q.has_loop_range = 1; q.loop_start = (float)sb.loop_start / total; q.loop_end = (float)sb.loop_end / total; }
  // a slot as the mixer sees it: a stereo source at the graph's rate that the mixer keeps, whose frames pg_grain_kernel stages; always `active` —
  // whether the slot plays is the note layer's (PgGSampler::active), a free slot's staged frames are zero
  const pg_voice_options vo = sampler_pool_voice_options(opt);
  PgVoice v;
  voice_init_grain_staged(g, v, &vo);
  if (graph_samp_reserve(g, g->samplers.size() + 1) || graph_gsamp_reserve(g, g->samplers.size() + 1) || graph_gran_reserve(g, g->gran_n + (size_t)n)) return -graph_fail(g, PG_ERR_DEVICE);
  {  // the launch lists hold every granular sampler's record and slots: graph_gsampler_upload_live runs inside write and must not allocate
    size_t slots = (size_t)n;
    for (const HostSampler& hs : g->samplers) if (hs.granular) slots += (size_t)hs.n_voices;
    if (g->d_gsamp_live.reserve(g->n_gsamplers + 1) || g->d_gsamp_grains.reserve(slots)) return -graph_fail(g, PG_ERR_DEVICE);
    g->gsamp_live.reserve(g->d_gsamp_live.cap); g->gsamp_grains.reserve(g->d_gsamp_grains.cap);
  }
  if (!g->gran_voices.empty()) g->gran_live_dirty = true;   // (graph_gran_reserve may have moved the lone voices' launch list: it is uploaded again)
  std::vector<void*> stages;
  auto release = [&]() { for (void* p : stages) (void)pg_free(p); };
  for (int k = 0; k < n; ++k) {
    void* p = nullptr;
    const hipError_t err = grain_stage_alloc(&p);
    if (p) stages.push_back(p);
    if (err != hipSuccess) { release(); return -graph_fail(g, set_error(PG_ERR_DEVICE, "granular sampler allocation failed")); }
  }
  int voice0 = -1;
  { const int rc = sampler_pool_push(g, v, n, &voice0); if (rc) { release(); return -rc; } }
  auto fail_upload = [&]() { release(); return -graph_fail(g, set_error(PG_ERR_DEVICE, "granular sampler upload failed")); };
  // The slots' grain records: GrainPool::new and, with a matrix, create_matrix per slot — no note yet, so no start() and no note_on: the trigger
  // phase and the playhead stand at 0, speed / volume / panning are neutral until a note's GrainPool::start, and a start time of UINT64_MAX says the
  // slot is free. Generator 0 of a slot is the pool's, 1 and 2 are its LFOs'.
  auto slot_rng = [&](int k, int generator, const uint64_t given[4], uint64_t out[4]) {
    if (gopt->rng_states) memcpy(out, gopt->rng_states + ((size_t)k * 3 + (size_t)generator) * 4, 4 * sizeof(uint64_t));
    else pg_granular_sampler_rng_state(given, (uint32_t)k, (uint32_t)generator, out);
  };
  const int grain0 = (int)g->gran_n;
  std::unique_ptr<PgGrainVoice> r(new PgGrainVoice);
  for (int k = 0; k < n; ++k) {
    uint64_t rng[3][4];
    slot_rng(k, 0, q.rng_state, rng[0]);
    grain_rec_init(*r, q, rng[0], /*speed*/ 1.0, /*volume*/ 1.0f, /*panning*/ 0.0f, /*trigger_phase*/ 0.0f, /*playhead*/ 0.0f,
                   sb.d_mono, (uint64_t)sb.mono_frames, stages[(size_t)k], /*start_time*/ UINT64_MAX, voice0 + k);
    if (gopt->modulation) {
      for (int l = 0; l < 2; ++l) slot_rng(k, 1 + l, gopt->modulation->lfo[l].rng_state, rng[1 + l]);
      mod_matrix_init(r->mod, *gopt->modulation, g->sample_rate, rng[1], rng[2]);
    }
    const int32_t rec = grain0 + k;
    if (pg_memcpy(g->d_gran + rec, r.get(), sizeof(PgGrainVoice), hipMemcpyHostToDevice) != hipSuccess ||
        pg_memcpy(g->d_grain_of_voice + voice0 + k, &rec, sizeof rec, hipMemcpyHostToDevice) != hipSuccess) return fail_upload();
    g->gran_ended[(size_t)rec] = 0;
  }
  g->gran_n += (size_t)n;
  // the note layer's record; the PgSamplerRec of the same index stays inert (n_voices 0): the unit kernel's sampler_command leaves the commands alone
  const int unit = to_main ? graph_new_sampler_unit(g, sampler_id) : -1;
  if (to_main && unit < 0) { release(); return -graph_fail(g, PG_ERR_DEVICE); }
  std::unique_ptr<PgGSampler> gs(new PgGSampler);
  memset(gs.get(), 0, sizeof(PgGSampler));
  note_rec_init(gs->note, to_main ? unit : g->mixers[mixer_id].unit_slot, voice0, n, opt);
  gs->grain0 = grain0; gs->index = sampler_id; gs->start_time = opt->start_time; gs->span_t0 = UINT64_MAX;
  if (opt->has_envelope) gs->env_params = ahdsr_build_params(opt->envelope, g->sample_rate);   // (every slot's envelope: Idle until its first note_on)
  std::unique_ptr<PgSamplerRec> inert(new PgSamplerRec);
  memset(inert.get(), 0, sizeof(PgSamplerRec));
  inert->unit = -1;
  // (the output stage of a sampler on the main mixer stands in THIS record for both kinds of pool: the unit kernel finds it by the sampler's index)
  if (to_main) { pg_generator_options go; if (gen) go = *gen; else pg_generator_options_default(&go); genout_init(g, inert->out, go.volume, go.panning); }
  if (pg_memcpy(g->d_gsamp + sampler_id, gs.get(), sizeof(PgGSampler), hipMemcpyHostToDevice) != hipSuccess ||
      pg_memcpy((PgSamplerRec*)(g->d_samp + 1) + sampler_id, inert.get(), sizeof(PgSamplerRec), hipMemcpyHostToDevice) != hipSuccess ||
      samp_head_upload(g, (size_t)sampler_id + 1) != hipSuccess || graph_env_head_refresh(g)) return fail_upload();
  HostSampler hs;
  hs.granular = true; hs.with_mod = gopt->modulation != nullptr; hs.grain0 = grain0;
  return sampler_pool_register(g, mixer_id, buffer_id, opt, vo, voice0, hs, SAMPLER_TAB_GRANULAR | (gopt->modulation ? SAMPLER_TAB_MATRIX : 0), &stages, unit);
}
int pg_graph_add_granular_sampler(pg_graph* g, int mixer_id, int buffer_id, const pg_sampler_options* opt, const pg_granular_sampler_options* gopt) {
  return add_granular_sampler(g, mixer_id, buffer_id, opt, gopt, false, nullptr);
}
int pg_graph_add_granular_sampler_to_main(pg_graph* g, int buffer_id, const pg_sampler_options* opt, const pg_granular_sampler_options* gopt, const pg_generator_options* gen) {
  return add_granular_sampler(g, PG_MAIN_MIXER, buffer_id, opt, gopt, true, gen);
}
int pg_graph_sampler_set_granular_parameter(pg_graph* g, int sampler_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time) {
  const int pi = find_granular_param(fourcc);
  if (pi < 0) return set_error(PG_ERR_PARAMETER, "Invalid/unknown granular playback parameter 0x%08x", fourcc);
  if (value != value) return set_error(PG_ERR_PARAMETER, "Granular playback parameter '%s' is not a number", GRANULAR_PARAMS[pi].name);
  const int w = sampler_tab_word(g, sampler_id);
  if (!w) return sampler_tab_error(g);
  if (!(w & SAMPLER_TAB_GRANULAR)) return set_error(PG_ERR_STATE, "Sampler with id %d plays files: it has no granular parameters", sampler_id);
  float raw;
  if (!resolve_update(GRANULAR_PARAMS[pi], value, is_normalized != 0, raw)) return PG_OK;   // a raw enum index out of range: logged + ignored in the reference (enum.rs:256-290)
  return sampler_message(g, sampler_id, pgc::CT_SAMPLER_GRAIN_PARAM, sample_time, pi, raw);
}
// ---- what changes every voice of the pool while notes sound: the envelope's knobs, the matrix, the loop range (Sampler::process_playback_messages,
// sampler.rs:656-731: SetParameter(AMP_* | ML1R | ML2R | ML1W | ML2W), SetModulation, ClearModulation, SamplerMessage::SetLoopRange). Any thread. ----
// ... of a granular sampler with a matrix (the reference: "only available when granular playback is enabled"; a pool without a matrix is this implementation's)
static int sampler_matrix_message(pg_graph* g, int sampler_id, int type, uint64_t sample_time, int param, float value) {
  const int w = sampler_tab_word(g, sampler_id);
  if (!w) return sampler_tab_error(g);
  if (!(w & SAMPLER_TAB_GRANULAR)) return set_error(PG_ERR_STATE, "Sampler with id %d plays files: modulation is only available when granular playback is enabled", sampler_id);
  if (!(w & SAMPLER_TAB_MATRIX)) return set_error(PG_ERR_STATE, "Sampler with id %d has no modulation matrix", sampler_id);
  return sampler_message(g, sampler_id, type, sample_time, param, value);
}
int pg_sampler_envelope_param_count(void) { return PG_SE_COUNT; }
int pg_sampler_envelope_param(int index, pg_param_desc* out) {   // Sampler::envelope_parameters() (sampler.rs:173-181)
  if (!out) return set_error(PG_ERR_PARAMETER, "output is null");
  if (index < 0 || index >= PG_SE_COUNT) return set_error(PG_ERR_NOT_FOUND, "no such parameter");
  param_desc_from_spec(SAMPLER_ENV_PARAMS[index], out);
  return PG_OK;
}
int pg_graph_sampler_set_envelope_parameter(pg_graph* g, int sampler_id, uint32_t fourcc, float value, int is_normalized, uint64_t sample_time) {
  const int pi = find_sampler_env_param(fourcc);
  if (pi < 0) return set_error(PG_ERR_PARAMETER, "Invalid/unknown envelope parameter 0x%08x", fourcc);
  if (value != value) return set_error(PG_ERR_PARAMETER, "Envelope parameter '%s' is not a number", SAMPLER_ENV_PARAMS[pi].name);
  float raw = 0.0f;
  (void)resolve_update(SAMPLER_ENV_PARAMS[pi], value, is_normalized != 0, raw);   // parameter_update_value (:862-883): clamped, or clamped to 0..=1 and denormalized
  const int w = sampler_tab_word(g, sampler_id);
  if (!w) return sampler_tab_error(g);
  if (!(w & SAMPLER_TAB_ENVELOPE)) return set_error(PG_ERR_PARAMETER, "Invalid or unknown sampler parameter 0x%08x: sampler %d has no envelope", fourcc, sampler_id);   // (:1128-1131, :1189)
  return sampler_message(g, sampler_id, pgc::CT_SAMPLER_ENV_PARAM, sample_time, pi, raw);
}
int pg_graph_sampler_set_modulation(pg_graph* g, int sampler_id, int source, int target, float amount, int bipolar, uint64_t sample_time) {
  { const int rc = mod_check_route(source, target, amount); if (rc) return rc; }
  const bool keep = fabsf(amount) >= 0.001f;   // update_target's threshold (matrix.rs:61), as pg_graph_set_voice_modulation has it
  return sampler_matrix_message(g, sampler_id, pgc::CT_SAMPLER_MOD_ROUTE, sample_time, source | (target << 8) | ((keep && bipolar) ? 1 << 16 : 0), keep ? amount : 0.0f);
}
int pg_graph_sampler_clear_modulation(pg_graph* g, int sampler_id, int source, int target, uint64_t sample_time) {
  return pg_graph_sampler_set_modulation(g, sampler_id, source, target, 0.0f, 0, sample_time);
}
int pg_graph_sampler_set_lfo_rate(pg_graph* g, int sampler_id, int lfo, float rate_hz, uint64_t sample_time) {
  if (lfo < 0 || lfo > 1) return set_error(PG_ERR_PARAMETER, "Invalid LFO index: %d", lfo);
  if (rate_hz != rate_hz) return set_error(PG_ERR_PARAMETER, "LFO %d rate is not a number", lfo + 1);
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  return sampler_matrix_message(g, sampler_id, pgc::CT_SAMPLER_LFO_RATE, sample_time, lfo, mod_phase_inc(rate_hz, g->sample_rate));
}
int pg_graph_sampler_set_lfo_waveform(pg_graph* g, int sampler_id, int lfo, int waveform, uint64_t sample_time) {
  if (lfo < 0 || lfo > 1) return set_error(PG_ERR_PARAMETER, "Invalid LFO index: %d", lfo);
  if (waveform < 0 || waveform > 6) return set_error(PG_ERR_PARAMETER, "Invalid LFO %d waveform: %d", lfo + 1, waveform);
  return sampler_matrix_message(g, sampler_id, pgc::CT_SAMPLER_LFO_WAVEFORM, sample_time, lfo | (waveform << 8), 0.0f);
}
int pg_graph_sampler_set_loop_range(pg_graph* g, int sampler_id, int has_loop_range, uint64_t loop_start, uint64_t loop_end, uint64_t sample_time) {
  if (has_loop_range && loop_start >= loop_end) return set_error(PG_ERR_PARAMETER, "Invalid loop range: %llu..%llu", (unsigned long long)loop_start, (unsigned long long)loop_end);
  const int w = sampler_tab_word(g, sampler_id);
  if (!w) return sampler_tab_error(g);
  if (!(w & SAMPLER_TAB_GRANULAR)) return set_error(PG_ERR_STATE, "Sampler with id %d plays files: its loop range is set when it is created", sampler_id);
  const uint64_t frames = g->sampler_frames_tab.get((size_t)sampler_id);
  if (has_loop_range && (loop_start >= frames || loop_end > frames))   // (:1251-1269)
    return set_error(PG_ERR_PARAMETER, "Invalid loop range: %llu..%llu not in range 0..%llu", (unsigned long long)loop_start, (unsigned long long)loop_end, (unsigned long long)frames);
  // SamplerVoice::set_loop_range (voice.rs:329-338): source frames over the FILE's frame count, as f32 — as at creation. None is no loop at all.
  const float total = (float)frames;
  return sampler_message(g, sampler_id, pgc::CT_SAMPLER_GRAIN_LOOP, sample_time, has_loop_range ? 1 : 0, has_loop_range ? (float)loop_start / total : 0.0f, has_loop_range ? (float)loop_end / total : 0.0f);
}
int pg_graph_sampler_envelope_params(pg_graph* g, int sampler_id, int slot, pg_sampler_envelope_state* out) {
  if (!out) return set_error(PG_ERR_PARAMETER, "output is null");
  if (!g) return set_error(PG_ERR_PARAMETER, "graph handle is null");
  const HostSampler* found = sampler_for_readback(g, sampler_id);
  if (!found) return PG_ERR_NOT_FOUND;
  const HostSampler& hs = *found;
  if (slot < 0 || slot >= hs.n_voices) return set_error(PG_ERR_PARAMETER, "Invalid slot: %d. The sampler has %d", slot, hs.n_voices);
  if (!hs.has_envelope) return set_error(PG_ERR_STATE, "Sampler with id %d has no envelope", sampler_id);
  PgEnvParams p;
  (void)hipSetDevice(g->device);
  if (hs.granular) { const int rc = graph_read_back(g, &p, (const char*)(g->d_gsamp + hs.rec) + offsetof(PgGSampler, env_params), sizeof p); if (rc) return rc; }
  else {   // slot 0's voice has the pool's first record, the slots follow it (pg_graph_add_sampler)
    const int voice0 = g->voices[hs.voice_id_slot0].dev_index;
    const int rc = graph_read_back(g, &p, (const char*)(g->d_env + voice0 + slot) + offsetof(PgEnv, params), sizeof p);
    if (rc) return rc;
  }
  out->attack_rate = p.attack_rate; out->decay_rate = p.decay_rate; out->release_rate = p.release_rate; out->sustain_level = p.sustain_level; out->hold_samples = p.hold_samples;
  out->attack_scaling = p.attack_scaling; out->decay_scaling = p.decay_scaling; out->release_scaling = p.release_scaling; out->zero_times = p.zero_times;
  return PG_OK;
}
// The granular sampler behind `sampler_id` for a read-back (as pg_graph_sampler_state finds it) and the grain record of its slot; < 0: -PG_ERR_*
static int gsampler_slot_record(pg_graph* g, int sampler_id, int slot, const void* out, bool need_mod) {
  if (!out) return -set_error(PG_ERR_PARAMETER, "output is null");
  if (!g) return -set_error(PG_ERR_PARAMETER, "graph handle is null");
  const HostSampler* found = sampler_for_readback(g, sampler_id);
  if (!found) return -PG_ERR_NOT_FOUND;
  const HostSampler& hs = *found;
  if (!hs.granular) return -set_error(PG_ERR_STATE, "Sampler with id %d plays files: it has no grain pools", sampler_id);
  if (slot < 0 || slot >= hs.n_voices) return -set_error(PG_ERR_PARAMETER, "Invalid slot: %d. The sampler has %d", slot, hs.n_voices);
  if (need_mod && !hs.with_mod) return -set_error(PG_ERR_STATE, "Sampler with id %d has no modulation matrix", sampler_id);
  return hs.grain0 + slot;
}
int pg_graph_sampler_voice_grain_state(pg_graph* g, int sampler_id, int slot, pg_grain_state* out) {
  const int rec = gsampler_slot_record(g, sampler_id, slot, out, false);
  return rec < 0 ? -rec : grain_state_read(g, rec, out);
}
int pg_graph_sampler_voice_modulation_state(pg_graph* g, int sampler_id, int slot, pg_modulation_state* out) {
  const int rec = gsampler_slot_record(g, sampler_id, slot, out, true);
  return rec < 0 ? -rec : modulation_state_read(g, rec, out);
}
int pg_graph_sampler_granular_params(pg_graph* g, int sampler_id, pg_granular_params* out) {   // (every slot holds the sampler's one parameter set)
  const int rec = gsampler_slot_record(g, sampler_id, 0, out, false);
  return rec < 0 ? -rec : granular_params_read(g, rec, out);
}

}  // extern "C"
