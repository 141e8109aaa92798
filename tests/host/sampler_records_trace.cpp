// A transcript of what the sampler host code (phonic_amd/csrc/pg_sampler.hip) WRITES: the records its constructors upload, the command records its
// timed calls turn into, the refusals of its calls and what its read-backs return — against the stub HIP runtime (hip_stub.cpp), whose "device"
// memory is plain host memory: the program reads the tables straight from the graph (pg_host_internal.h) and prints every record field by field.
// Floats and doubles appear as hex bit patterns, pointers as a<allocation ordinal>+<byte offset> (hip_stub_locate; the observer is installed before
// the first graph is created), consecutive records with identical fields are folded into one line. One `== scenario` header per step. All graphs
// run at 48 kHz with max_frames 256; the sample buffers are a 3001-frame mono one with an embedded loop, a stereo one and a mono one without a loop.
// pow() may differ in its last bit between C libraries: only transpose values that are multiples of 12 with finetune 0 are sent, no normalized
// value goes to a parameter with a curved scaling, and speed_from_note's table is not printed. The output is compared byte for byte with
// tests/golden/sampler_records_trace.txt (tests/test_host_sampler_records.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "hip_stub_observer.h"
#include "../../phonic_amd/csrc/pg_host_internal.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, pg_last_error_message()); exit(1); } } while (0)
#define ID4(s) PG_FOURCC(s[0], s[1], s[2], s[3])

// ---- formatting ---------------------------------------------------------------------------------------------------------------------------
static std::string F(const char* fmt, ...) {
  char buf[4096];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}
static std::string H(float f) { uint32_t u; memcpy(&u, &f, 4); return F("%08x", u); }
static std::string D(double d) { uint64_t u; memcpy(&u, &d, 8); return F("%016llx", (unsigned long long)u); }
static std::string U(uint64_t v) { return v == UINT64_MAX ? "max" : F("%llu", (unsigned long long)v); }
static std::string P(const void* p) {
  if (!p) return "null";
  size_t off = 0;
  const int a = hip_stub_locate(p, &off);
  return a < 0 ? "host" : F("a%d+%zu", a, off);
}
static std::string R4(const uint64_t r[4]) { return F("%016llx:%016llx:%016llx:%016llx", (unsigned long long)r[0], (unsigned long long)r[1], (unsigned long long)r[2], (unsigned long long)r[3]); }
// `name[i] body` per entry, a run of entries equal to the one in front of it as one line
static void fold(const char* name, const std::vector<std::string>& bodies, int first = 0) {
  for (size_t i = 0; i < bodies.size();) {
    size_t j = i + 1;
    while (j < bodies.size() && bodies[j] == bodies[i]) ++j;
    printf("  %s[%d] %s\n", name, first + (int)i, bodies[i].c_str());
    if (j > i + 1) printf("  %s[%d..%d] identical to %d\n", name, first + (int)i + 1, first + (int)j - 1, first + (int)i);
    i = j;
  }
}

// ---- records ------------------------------------------------------------------------------------------------------------------------------
static std::string smooth_str(const PgSmooth& s) { return F("{%d %s %s %s %s %s %u}", s.kind, H(s.current).c_str(), H(s.target).c_str(), H(s.a).c_str(), H(s.b).c_str(), H(s.comp).c_str(), s.pending); }
static std::string voice_str(const PgVoice& v) {
  std::string s = F("pcm=%s n_samples=%s ch=%u rates=%u,%u input=", P(v.pcm).c_str(), U(v.n_samples).c_str(), v.channels, v.src_rate, v.out_rate);
  for (int c = 0; c < 2; ++c) for (int i = 0; i < 4; ++i) s += H(v.input[c][i]) + (c == 1 && i == 3 ? "" : ",");
  s += F(" sub_pos=%s,%s ratio=%s init=%d,%d pos=%s repeat=%s,%s eof=%d finished=%d loop=%d,%s,%s", H(v.sub_pos[0]).c_str(), H(v.sub_pos[1]).c_str(), H(v.ratio).c_str(),
         v.initialized[0], v.initialized[1], U(v.playback_pos).c_str(), U(v.repeat).c_str(), U(v.repeat_count).c_str(), v.pos_eof, v.finished, v.has_loop, U(v.loop_start).c_str(), U(v.loop_end).c_str());
  s += F(" fader=%d,%s,%s,%s fade_out=%s volume=%s panning=%s start=%s stop=%s has_stop=%d active=%d", v.fader_state, H(v.fader_current).c_str(), H(v.fader_target).c_str(), H(v.fader_inertia).c_str(),
         H(v.fade_out_seconds).c_str(), smooth_str(v.volume).c_str(), smooth_str(v.panning).c_str(), U(v.start_time).c_str(), U(v.stop_time).c_str(), v.has_stop, v.active);
  s += F(" speed=%s,%s glide=%s next_speed=%u sched=%d,%d,%d stop_pos=%u,%u", D(v.current_speed).c_str(), D(v.target_speed).c_str(), H(v.speed_glide_rate).c_str(), v.samples_to_next_speed_update,
         v.sched_class, v.sched_rep, v.sched_hit, v.stop_pos_lo, v.stop_pos_hi);
  s += F(" outer=%d,%d,%d,%d,%s,%s,%s in=", v.outer_on, v.outer_pending_stop, v.outer_init[0], v.outer_init[1], H(v.outer_ratio).c_str(), H(v.outer_sub_pos[0]).c_str(), H(v.outer_sub_pos[1]).c_str());
  for (int c = 0; c < 2; ++c) for (int i = 0; i < 4; ++i) s += H(v.outer_input[c][i]) + (c == 1 && i == 3 ? "" : ",");
  s += F(" temp=%u,%u,%u,%u stage=%s,%s stream=%d,%u,%s zombie_end=%s chunk_skip=%d persistent=%d", v.in_start, v.in_end, v.out_start, v.out_end, P(v.stage_in).c_str(), P(v.stage_out).c_str(),
         v.stream_on, v.stream_cap, U(v.stream_fed).c_str(), U(v.zombie_end).c_str(), v.chunk_skip, v.persistent);
  return s;
}
static std::string env_params_str(const PgEnvParams& p) {
  return F("rates=%s,%s,%s scalings=%s,%s,%s sustain=%s hold=%s zero=%d", H(p.attack_rate).c_str(), H(p.decay_rate).c_str(), H(p.release_rate).c_str(), H(p.attack_scaling).c_str(),
           H(p.decay_scaling).c_str(), H(p.release_scaling).c_str(), H(p.sustain_level).c_str(), H(p.hold_samples).c_str(), p.zero_times);
}
static std::string env_state_str(const PgEnvState& s) {
  return F("stage=%d target=%s hold_left=%s release_out=%s out=%s", s.stage, H(s.target_volume).c_str(), H(s.hold_samples_remaining).c_str(), H(s.release_output).c_str(), H(s.output).c_str());
}
static std::string env_str(const PgEnv& e) { return F("on=%d %s | %s", e.on, env_state_str(e.state).c_str(), env_params_str(e.params).c_str()); }
static void dump_env_head(const pg_graph* g) {
  if (!g->d_env_tab) { printf("  env_table none\n"); return; }
  const PgEnvTable& t = *g->d_env_tab;
  printf("  env_table at=%s done=%s cap=%s grain_of_voice=%s grains=%s n_grains=%u n_stats=%u stat_of_voice=%s stats=%s samplers=%s | host: env=%s done_cap=%zu\n", P(g->d_env_tab).c_str(), P(t.done).c_str(),
         U(t.cap).c_str(), P(t.grain_of_voice).c_str(), P(t.grains).c_str(), t.n_grains, t.n_stats, P(t.stat_of_voice).c_str(), P(t.stats).c_str(), P(t.samplers).c_str(), P(g->d_env).c_str(), g->env_done.cap);
}
static void dump_samp_head(const pg_graph* g) {
  if (!g->d_samp) { printf("  sampler_table none\n"); return; }
  const PgSamplerTab& t = *g->d_samp;
  printf("  sampler_table at=%s n=%u speed_tab=%s stopped=%s | host: samp_cap=%zu gsamp=%s gsamp_cap=%zu gran=%s gran_n=%zu gran_cap=%zu\n", P(g->d_samp).c_str(), t.n, P(t.speed_tab).c_str(), P(t.stopped).c_str(),
         g->samp_cap, P(g->d_gsamp).c_str(), g->gsamp_cap, P(g->d_gran).c_str(), g->gran_n, g->gran_ended.cap);
}
static void dump_note_rec(const char* name, const PgSamplerRec& r) {
  printf("  %s unit=%d voice0=%d n_voices=%d has_envelope=%d transient=%d stopping=%d stopped=%d transpose=%d finetune=%d base=%s,%s pitch_factor=%s\n", name, r.unit, r.voice0, r.n_voices, r.has_envelope,
         r.transient, r.stopping, r.stopped, r.transpose, r.finetune, H(r.base_volume).c_str(), H(r.base_panning).c_str(), D(r.pitch_factor).c_str());
  std::vector<std::string> slots;
  for (int k = 0; k < PG_SAMPLER_MAX_VOICES; ++k) {
    const PgSamplerSlot& s = r.slots[k];
    slots.push_back(F("note_id=%s release_start=%s volume=%s panning=%s note=%d", U(s.note_id).c_str(), U(s.release_start_frame).c_str(), H(s.note_volume).c_str(), H(s.note_panning).c_str(), s.note));
  }
  fold("  slot", slots);
}
static void dump_grain_rec(const pg_graph* g, int rec) {
  const PgGrainVoice& r = g->d_gran[rec];
  const PgGrainParams& q = r.params;
  printf("  grain_rec[%d] params: overlap=%d window=%d size=%s density=%s variation=%s spray=%s pan_spread=%s direction=%d position=%s step=%s loop=%d,%s,%s\n", rec, q.overlap_mode, q.window, H(q.size).c_str(),
         H(q.density).c_str(), H(q.variation).c_str(), H(q.spray).c_str(), H(q.pan_spread).c_str(), q.direction, H(q.position).c_str(), H(q.step).c_str(), q.has_loop, H(q.loop_start).c_str(), H(q.loop_end).c_str());
  const PgGrainPool& p = r.pool;
  printf("    pool: rng=%s speed=%s trigger_phase=%s playhead=%s volume=%s panning=%s playing_loop=%d trigger_new=%d primary=%d overlap=%d\n", R4(p.rng).c_str(), D(p.speed).c_str(), H(p.trigger_phase).c_str(),
         H(p.playhead).c_str(), H(p.volume).c_str(), H(p.panning).c_str(), p.playing_loop_range, p.trigger_new_grains, p.primary, p.overlap_mode);
  printf("    pcm=%s n_frames=%s staged=%s stage_pos=%s start=%s stop=%s exhausted_at=%s voice=%d has_env=%d pos_trace=%s ended_word=%d\n", P(r.pcm).c_str(), U(r.n_frames).c_str(), P(r.staged).c_str(), U(r.stage_pos).c_str(),
         U(r.start_time).c_str(), U(r.stop_time).c_str(), U(r.exhausted_at).c_str(), r.voice, r.has_env, P(r.pos_trace).c_str(), (int)g->gran_ended[(size_t)rec]);
  std::vector<std::string> grains;
  for (int i = 0; i < PG_GRAIN_POOL; ++i) {
    const PgGrain& s = r.grains[i];
    grains.push_back(F("pos=%s inc=%s wphase=%s winc=%s loop=%d,%s,%s left=%s volume=%s panning=%s active=%d window=%d", D(s.position).c_str(), D(s.increment).c_str(), D(s.window_phase).c_str(),
                       D(s.window_increment).c_str(), s.has_loop, D(s.loop_start).c_str(), D(s.loop_end).c_str(), U(s.samples_remaining).c_str(), H(s.volume).c_str(), H(s.panning).c_str(), s.active, s.window_mode));
  }
  fold("  grain", grains);
  const PgGrainMod& m = r.mod;
  printf("    mod: on=%d velocity=%s note_pitch=%s\n", m.on, H(m.velocity).c_str(), H(m.note_pitch).c_str());
  if (!m.on) {   // (no matrix: the rest must be zero; say so in one word)
    static const PgGrainMod zero = {};
    PgGrainMod copy = m;
    copy.pad = 0; copy.pad_last = 0; copy.lfo[0].pad[0] = copy.lfo[0].pad[1] = copy.lfo[1].pad[0] = copy.lfo[1].pad[1] = 0;
    printf("    mod rest %s\n", memcmp(&copy, &zero, sizeof zero) == 0 ? "zero" : "NOT ZERO");
    return;
  }
  for (int l = 0; l < 2; ++l) {
    const PgModLfo& o = m.lfo[l];
    printf("    lfo[%d] phase=%s phase_inc=%s waveform=%d sample_hold=%s jitter=%s,%s rng=%s\n", l, H(o.phase).c_str(), H(o.phase_inc).c_str(), o.waveform, H(o.sample_hold).c_str(), H(o.jitter_current).c_str(),
           H(o.jitter_target).c_str(), R4(o.rng).c_str());
  }
  printf("    routes:");
  for (int s = 0; s < PG_GMOD_SOURCES; ++s) for (int t = 0; t < PG_GMOD_TARGETS; ++t) if (m.amount[s][t] != 0.0f || m.bipolar[s][t]) printf(" %d>%d=%s,%d", s, t, H(m.amount[s][t]).c_str(), m.bipolar[s][t]);
  printf("\n    last:");
  for (int t = 0; t < PG_GMOD_TARGETS; ++t) printf(" %s", H(m.last[t]).c_str());
  printf("\n");
}
// What the host keeps of sampler `id`, its table words, its mixer's list of voices and the pool's voices as the host registered them
static void dump_host_sampler(pg_graph* g, int id) {
  const HostSampler& hs = g->samplers[id];
  printf("  host_sampler[%d] mixer=%d rec=%d voice_id_slot0=%d n_voices=%d has_envelope=%d transient=%d start=%s alive=%d transpose=%d finetune=%d granular=%d with_mod=%d grain0=%d tab_word=%d frames=%s stopped_word=%d\n", id,
         hs.mixer, hs.rec, hs.voice_id_slot0, hs.n_voices, hs.has_envelope, hs.transient, U(hs.start_time).c_str(), hs.alive, hs.transpose, hs.finetune, hs.granular, hs.with_mod, hs.grain0,
         (int)g->sampler_alive_tab.get((size_t)id), U(g->sampler_frames_tab.get((size_t)id)).c_str(), (int)g->samp_stopped[(size_t)id]);
  printf("    env: %s\n", env_params_str(hs.env).c_str());
  printf("    mixer_voices:");
  for (int v : g->mixers[hs.mixer].voices) printf(" %d", v);
  printf("\n");
  std::vector<std::string> hv;
  for (int k = 0; k < hs.n_voices; ++k) {
    const int vid = hs.voice_id_slot0 - k;
    const HostVoice& v = g->voices[vid];
    hv.push_back(F("id_minus_slot0=%d dev_minus_k=%d mixer=%d start=%s transient=%d sbuf=%d sampler=%d gran=%d pcm=%s stage_owned=%d file=%u,%u,%s kind=%d", vid - hs.voice_id_slot0 + k, v.dev_index - k, v.mixer, U(v.start_time).c_str(),
                   v.transient, v.sbuf, v.sampler, v.gran, P(v.d_pcm).c_str(), v.d_stage ? 1 : 0, v.file_channels, v.file_rate, U(v.file_samples).c_str(), (int)voice_kind(g, vid)));
  }
  fold("  host_voice", hv);
}
static void dump_pool_voices(pg_graph* g, int voice0, int n, bool envs) {
  CHECK(g->d_voices.flush() == PG_OK);
  std::vector<std::string> vs, es, gv;
  for (int k = 0; k < n; ++k) {
    vs.push_back(voice_str(g->d_voices.d[voice0 + k]));
    if (envs && g->d_env) es.push_back(env_str(g->d_env[voice0 + k]) + F(" done_word=%d", (int)g->env_done[(size_t)(voice0 + k)]));
    if (g->d_grain_of_voice) gv.push_back(F("rec_minus_k=%d", g->d_grain_of_voice[voice0 + k] < 0 ? -1000 : g->d_grain_of_voice[voice0 + k] - k));
  }
  fold("voice", vs, voice0);
  fold("env", es, voice0);
  fold("grain_of_voice", gv, voice0);
}
static void dump_file_sampler(pg_graph* g, int id) {
  dump_samp_head(g);
  dump_env_head(g);
  const PgSamplerRec& r = ((const PgSamplerRec*)(g->d_samp + 1))[id];
  dump_note_rec(F("sampler_rec[%d]", id).c_str(), r);
  dump_host_sampler(g, id);
  dump_pool_voices(g, r.voice0, r.n_voices, true);
}
static void dump_granular_sampler(pg_graph* g, int id) {
  dump_samp_head(g);
  dump_env_head(g);
  const PgGSampler& q = g->d_gsamp[id];
  dump_note_rec(F("gsampler[%d].note", id).c_str(), q.note);
  printf("  gsampler[%d] grain0=%d index=%d start=%s span_t0=%s env_params: %s\n", id, q.grain0, q.index, U(q.start_time).c_str(), U(q.span_t0).c_str(), env_params_str(q.env_params).c_str());
  std::vector<std::string> env, act;
  for (int k = 0; k < PG_SAMPLER_MAX_VOICES; ++k) { env.push_back(env_state_str(q.env[k])); act.push_back(F("%d", q.active[k])); }
  fold("  slot_env", env);
  fold("  slot_active", act);
  dump_note_rec(F("sampler_rec[%d] (inert)", id).c_str(), ((const PgSamplerRec*)(g->d_samp + 1))[id]);
  dump_host_sampler(g, id);
  dump_pool_voices(g, q.note.voice0, q.note.n_voices, true);
  for (int k = 0; k < q.note.n_voices; ++k) dump_grain_rec(g, q.grain0 + k);
  printf("  launch lists: gsamp_live cap>=%d gsamp_grains cap>=%d n_gsamplers=%zu gsamp_dirty=%d gran_live_dirty=%d\n", g->d_gsamp_live.cap >= g->n_gsamplers, g->d_gsamp_grains.cap >= (size_t)q.note.n_voices, g->n_gsamplers,
         g->gsamp_dirty, g->gran_live_dirty);
}
static void dump_lone_voice(pg_graph* g, int vid) {
  CHECK(g->d_voices.flush() == PG_OK);
  const HostVoice& hv = g->voices[vid];
  printf("  host_voice[%d] dev=%d mixer=%d start=%s gran=%d gran_live=%d env=%d env_live=%d mod=%d sbuf=%d pcm=%s stage=%s file=%u,%u,%s kind=%d\n", vid, hv.dev_index, hv.mixer, U(hv.start_time).c_str(), hv.gran, hv.gran_live,
         hv.env, hv.env_live, hv.mod, hv.sbuf, P(hv.d_pcm).c_str(), P(hv.d_stage).c_str(), hv.file_channels, hv.file_rate, U(hv.file_samples).c_str(), (int)voice_kind(g, vid));
  printf("  voice[%d] %s\n", hv.dev_index, voice_str(g->d_voices.d[hv.dev_index]).c_str());
  if (g->d_env) printf("  env[%d] %s done_word=%d\n", hv.dev_index, env_str(g->d_env[hv.dev_index]).c_str(), (int)g->env_done[(size_t)hv.dev_index]);
  if (g->d_grain_of_voice) printf("  grain_of_voice[%d] %d\n", hv.dev_index, g->d_grain_of_voice[hv.dev_index]);
  if (hv.gran >= 0) dump_grain_rec(g, hv.gran);
}

// ---- calls ----------------------------------------------------------------------------------------------------------------------------------
// a call's text, what it returned and, for an error, the message it left
#define CALL(expr) do { const long long rc_ = (long long)(expr); printf("  %s -> %lld%s%s\n", #expr, rc_, rc_ != 0 ? " | " : "", rc_ != 0 ? pg_last_error_message() : ""); } while (0)
#define CALLID(expr) do { const long long rc_ = (long long)(expr); printf("  %s -> %lld%s%s\n", #expr, rc_, rc_ < 0 ? " | " : "", rc_ < 0 ? pg_last_error_message() : ""); } while (0)

static bool g_tracing = false;
static int observe(const StubCall* c) {
  if (!g_tracing || c->kind != STUB_LAUNCH || !c->name || !strstr(c->name, "pg_gsampler_kernel")) return 0;
  const PgGSamplerLaunch* L = (const PgGSamplerLaunch*)c->args[0];
  printf("  boundary t=%s frame=%u first=%d closing=%d n_live=%u cmds:", U(L->t).c_str(), L->frame, L->chunk_first, L->closing, L->n_live);
  if (!L->closing && L->cmds) for (int i = 0; i < L->n_cmds; ++i) {
    const PgCmd& cmd = L->cmds[i];
    if (cmd.frame == L->frame) printf(" [type=%d target=%d unit=%d frame=%u param=%d value=%s value64=%llx]", cmd.type, cmd.target, cmd.unit, cmd.frame, cmd.param, H(cmd.value).c_str(), (unsigned long long)cmd.value64);
  }
  printf("\n");
  return 0;
}
static void write_frames(pg_graph* g, uint64_t& pos, size_t frames) {
  std::vector<float> out(frames * 2);
  printf("  write pos=%s frames=%zu\n", U(pos).c_str(), frames);
  g_tracing = true;
  const size_t n = pg_graph_write(g, out.data(), out.size(), pos);
  g_tracing = false;
  printf("  write -> %zu\n", n);
  pos += frames;
}

static void print_sampler_state(pg_graph* g, int id) {
  std::unique_ptr<pg_sampler_state> st(new pg_sampler_state);
  memset(st.get(), 0xee, sizeof(pg_sampler_state));
  const int rc = pg_graph_sampler_state(g, id, st.get());
  printf("  pg_graph_sampler_state(%d) -> %d%s%s\n", id, rc, rc ? " | " : "", rc ? pg_last_error_message() : "");
  if (rc) return;
  printf("    voices=%d active=%d stopping=%d stopped=%d transpose=%d finetune=%d volume=%s panning=%s\n", st->voice_count, st->active_voices, st->stopping, st->stopped, st->transpose, st->finetune, H(st->volume).c_str(), H(st->panning).c_str());
  std::vector<std::string> slots;
  for (int k = 0; k < PG_SAMPLER_MAX_VOICES; ++k) {
    const pg_sampler_slot_state& s = st->slots[k];
    slots.push_back(F("note_id=%lld release_start=%s volume=%s panning=%s note=%d stage=%d", (long long)s.note_id, U(s.release_start_frame).c_str(), H(s.note_volume).c_str(), H(s.note_panning).c_str(), s.note, s.envelope_stage));
  }
  fold("  slot", slots);
}
static void print_envelope_params(pg_graph* g, int id, int slot) {
  pg_sampler_envelope_state e;
  const int rc = pg_graph_sampler_envelope_params(g, id, slot, &e);
  printf("  pg_graph_sampler_envelope_params(%d, %d) -> %d%s%s\n", id, slot, rc, rc ? " | " : "", rc ? pg_last_error_message() : "");
  if (!rc) printf("    rates=%s,%s,%s sustain=%s hold=%s scalings=%s,%s,%s zero=%d\n", H(e.attack_rate).c_str(), H(e.decay_rate).c_str(), H(e.release_rate).c_str(), H(e.sustain_level).c_str(), H(e.hold_samples).c_str(),
                  H(e.attack_scaling).c_str(), H(e.decay_scaling).c_str(), H(e.release_scaling).c_str(), e.zero_times);
}
static void print_grain_state(const char* what, int rc, const pg_grain_state& s) {
  printf("  %s -> %d%s%s\n", what, rc, rc ? " | " : "", rc ? pg_last_error_message() : "");
  if (rc) return;
  printf("    trigger_phase=%s playhead=%s playing_loop=%d trigger_new=%d primary=%d overlap=%d speed=%s volume=%s panning=%s rng=%s\n", H(s.trigger_phase).c_str(), H(s.playhead).c_str(), s.playing_loop_range,
         s.trigger_new_grains, s.primary_slot, s.overlap_mode, D(s.speed).c_str(), H(s.volume).c_str(), H(s.panning).c_str(), R4(s.rng_state).c_str());
  std::vector<std::string> slots;
  for (int i = 0; i < PG_GRAIN_POOL; ++i) {
    const pg_grain_slot& o = s.slots[i];
    slots.push_back(F("pos=%s inc=%s wphase=%s winc=%s left=%s volume=%s panning=%s active=%d window=%d loop=%d", D(o.position).c_str(), D(o.increment).c_str(), D(o.window_phase).c_str(), D(o.window_increment).c_str(),
                      U(o.samples_remaining).c_str(), H(o.volume).c_str(), H(o.panning).c_str(), o.active, o.window_mode, o.has_loop_range));
  }
  fold("  slot", slots);
}
static void print_modulation_state(const char* what, int rc, const pg_modulation_state& m) {
  printf("  %s -> %d%s%s\n", what, rc, rc ? " | " : "", rc ? pg_last_error_message() : "");
  if (rc) return;
  for (int l = 0; l < 2; ++l) {
    const pg_mod_lfo_state& o = m.lfo[l];
    printf("    lfo[%d] phase=%s phase_inc=%s sample_hold=%s jitter=%s,%s waveform=%d rng=%s\n", l, H(o.phase).c_str(), H(o.phase_inc).c_str(), H(o.sample_hold).c_str(), H(o.jitter_current).c_str(), H(o.jitter_target).c_str(),
           o.waveform, R4(o.rng_state).c_str());
  }
  printf("    velocity=%s note_pitch=%s routes:", H(m.velocity).c_str(), H(m.note_pitch).c_str());
  for (int s = 0; s < PG_MOD_SOURCES; ++s) for (int t = 0; t < PG_MOD_TARGETS; ++t) if (m.routes[s][t].amount != 0.0f || m.routes[s][t].bipolar) printf(" %d>%d=%s,%d", s, t, H(m.routes[s][t].amount).c_str(), m.routes[s][t].bipolar);
  printf(" last:");
  for (int t = 0; t < PG_MOD_TARGETS; ++t) printf(" %s", H(m.last[t]).c_str());
  printf("\n");
}
static void print_granular_params(const char* what, int rc, const pg_granular_params& p) {
  printf("  %s -> %d%s%s\n", what, rc, rc ? " | " : "", rc ? pg_last_error_message() : "");
  if (rc) return;
  printf("    overlap=%d window=%d size=%s density=%s variation=%s spray=%s pan_spread=%s direction=%d position=%s step=%s loop=%d,%s,%s reserved=%d rng=%s\n", p.overlap_mode, p.window, H(p.size).c_str(), H(p.density).c_str(),
         H(p.variation).c_str(), H(p.spray).c_str(), H(p.pan_spread).c_str(), p.playback_direction, H(p.position).c_str(), H(p.step).c_str(), p.has_loop_range, H(p.loop_start).c_str(), H(p.loop_end).c_str(), p.reserved, R4(p.rng_state).c_str());
}
static void print_readbacks(pg_graph* g, int id, int slot) {
  print_sampler_state(g, id);
  print_envelope_params(g, id, slot);
  std::unique_ptr<pg_grain_state> gs(new pg_grain_state);
  int rc = pg_graph_sampler_voice_grain_state(g, id, slot, gs.get());
  print_grain_state(F("pg_graph_sampler_voice_grain_state(%d, %d)", id, slot).c_str(), rc, *gs);
  pg_modulation_state ms;
  rc = pg_graph_sampler_voice_modulation_state(g, id, slot, &ms);
  print_modulation_state(F("pg_graph_sampler_voice_modulation_state(%d, %d)", id, slot).c_str(), rc, ms);
  pg_granular_params gp;
  rc = pg_graph_sampler_granular_params(g, id, &gp);
  print_granular_params(F("pg_graph_sampler_granular_params(%d)", id).c_str(), rc, gp);
}

// every timed pg_graph_sampler_* call once on sampler `s`, stamped from `t` on in steps of 3 (out of order where `shuffle`)
static void send_all(pg_graph* g, int s, uint64_t t, bool shuffle) {
  auto at = [&](int i) { return t + (uint64_t)(shuffle ? (i * 7) % 16 : i) * 3; };
  const int64_t note = pg_graph_sampler_note_on(g, s, 72, 0.5f, -0.25f, at(0));
  printf("  pg_graph_sampler_note_on(%d, 72, 0.5, -0.25) -> %s\n", s, note > 0 ? "a note id" : F("%lld | %s", (long long)note, pg_last_error_message()).c_str());
  const int64_t id = note > 0 ? note : 1;
  CALL(pg_graph_sampler_set_note_speed(g, s, id, 2.0, 12.0f, at(1)));
  CALL(pg_graph_sampler_set_note_volume(g, s, id, 0.75f, at(2)));
  CALL(pg_graph_sampler_set_note_panning(g, s, id, 0.5f, at(3)));
  CALL(pg_graph_sampler_set_parameter(g, s, ID4("STRN"), 12.0f, 0, at(4)));
  CALL(pg_graph_sampler_set_parameter(g, s, ID4("SVOL"), 0.5f, 0, at(5)));
  CALL(pg_graph_sampler_set_parameter(g, s, ID4("SPAN"), 0.75f, 1, at(5)));
  CALL(pg_graph_sampler_set_granular_parameter(g, s, ID4("GVAR"), 0.25f, 1, at(6)));
  CALL(pg_graph_sampler_set_granular_parameter(g, s, ID4("GWND"), 3.0f, 0, at(6)));
  CALL(pg_graph_sampler_set_granular_parameter(g, s, ID4("GWND"), 99.0f, 0, at(6)));   // a raw enum index out of range: ignored
  CALL(pg_graph_sampler_set_envelope_parameter(g, s, ID4("ASTN"), 0.5f, 1, at(7)));
  CALL(pg_graph_sampler_set_envelope_parameter(g, s, ID4("ADCY"), 0.25f, 0, at(8)));
  CALL(pg_graph_sampler_set_envelope_parameter(g, s, ID4("AHLD"), 0.0f, 0, at(8)));
  CALL(pg_graph_sampler_set_modulation(g, s, 1, 3, -0.5f, 1, at(9)));
  CALL(pg_graph_sampler_set_modulation(g, s, 0, 2, 0.0005f, 1, at(9)));
  CALL(pg_graph_sampler_clear_modulation(g, s, 1, 3, at(10)));
  CALL(pg_graph_sampler_set_lfo_rate(g, s, 1, 100.0f, at(11)));
  CALL(pg_graph_sampler_set_lfo_waveform(g, s, 0, 5, at(12)));
  CALL(pg_graph_sampler_set_loop_range(g, s, 1, 300, 1500, at(13)));
  CALL(pg_graph_sampler_set_loop_range(g, s, 0, 9, 3, at(13)));
  CALL(pg_graph_sampler_note_off(g, s, id, at(14)));
  CALL(pg_graph_sampler_note_off(g, s, (int64_t)1 << 40, at(14)));   // a note id this graph never handed out
  CALL(pg_graph_sampler_all_notes_off(g, s, at(15)));
  CALL(pg_graph_sampler_stop(g, s, at(15)));
}

int main() {
  uint64_t c0[4], c1[4];
  pg_debug_hip_calls(c0);
  hip_stub_set_observer(observe);
  pg_graph* g = pg_graph_create(48000, 2, 256, 0);
  CHECK(g);
  std::vector<float> pcm(3001 * 2);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (float)((i * 37) % 101) / 101.0f - 0.5f;
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = 1; d.rate = 48000; d.has_loop_range = 1; d.loop_start = 100; d.loop_end = 2900;
  const int buf = pg_graph_add_sample_buffer(g, pcm.data(), 3001, &d);
  d.channels = 2; d.rate = 44100; d.has_loop_range = 0;
  const int buf_st = pg_graph_add_sample_buffer(g, pcm.data(), 1000, &d);
  d.channels = 1; d.rate = 48000;
  const int buf_plain = pg_graph_add_sample_buffer(g, pcm.data(), 2000, &d);
  CHECK(buf == 0 && buf_st == 1 && buf_plain == 2);
  const int m1 = pg_graph_add_mixer(g), m2 = pg_graph_add_mixer(g);
  CHECK(m1 > 0 && m2 > 0);
  pg_ahdsr_params env;
  pg_ahdsr_params_default(&env);
  env.attack_s = 0.002f; env.hold_s = 0.003f; env.decay_s = 0.004f; env.sustain_level = 0.6f; env.release_s = 0.005f; env.attack_scaling = 0.25f; env.release_scaling = -0.5f;

  // ---- 1. file samplers ----
  pg_sampler_options o;
  printf("== file sampler: default options (null)\n");
  const int f_def = pg_graph_add_sampler(g, m1, buf, nullptr);
  CHECK(f_def == 0);
  dump_file_sampler(g, f_def);
  printf("== file sampler: 1 voice, stereo buffer at another rate\n");
  pg_sampler_options_default(&o);
  o.voice_count = 1;
  const int f_one = pg_graph_add_sampler(g, m1, buf_st, &o);
  CHECK(f_one == 1);
  dump_file_sampler(g, f_one);
  printf("== file sampler: 64 voices, envelope, transient, start time\n");
  pg_sampler_options_default(&o);
  o.voice_count = 64; o.has_envelope = 1; o.envelope = env; o.transient = 1; o.start_time = 12345;
  const int f_big = pg_graph_add_sampler(g, m2, buf, &o);
  CHECK(f_big == 2);
  dump_file_sampler(g, f_big);
  printf("== file sampler: an explicit loop range, zero envelope times\n");
  pg_sampler_options_default(&o);
  o.voice_count = 3; o.has_loop_range = 1; o.loop_start = 7; o.loop_end = 3001; o.has_envelope = 1; o.envelope = env; o.envelope.attack_s = 0.0f; o.envelope.decay_s = 0.0f; o.envelope.release_s = 0.0f; o.envelope.hold_s = 0.0f;
  const int f_loop = pg_graph_add_sampler(g, m1, buf, &o);
  CHECK(f_loop == 3);
  dump_file_sampler(g, f_loop);
  printf("== file sampler: a buffer without an embedded loop (the sampler table grows)\n");
  pg_sampler_options_default(&o);
  o.voice_count = 2;
  const int f_plain = pg_graph_add_sampler(g, m1, buf_plain, &o);
  CHECK(f_plain == 4);
  dump_file_sampler(g, f_plain);
  printf("== file sampler 0 again, behind the growth\n");
  dump_file_sampler(g, f_def);

  // ---- 2. granular samplers ----
  pg_granular_sampler_options go;
  pg_modulation_params mp;
  pg_modulation_params_default(&mp);
  mp.lfo[0].rate_hz = 0.001f; mp.lfo[0].waveform = 5; mp.lfo[1].rate_hz = 50.0f; mp.lfo[1].waveform = 6; mp.velocity = 0.5f; mp.note = 72;
  mp.routes[0][0].amount = 0.5f; mp.routes[0][0].bipolar = 1; mp.routes[1][5].amount = -1.0f; mp.routes[2][3].amount = 0.0005f; mp.routes[2][3].bipolar = 1; mp.routes[3][6].amount = 0.25f; mp.routes[3][6].bipolar = 7;
  printf("== granular sampler: no matrix, derived rng states\n");
  pg_granular_sampler_options_default(&go);
  go.params.size = 3.0f; go.params.density = 100.0f; go.params.rng_state[0] = 11; go.params.rng_state[3] = 99;
  pg_sampler_options_default(&o);
  o.voice_count = 3;
  const int g_plain = pg_graph_add_granular_sampler(g, m1, buf, &o, &go);
  CHECK(g_plain == 5);
  dump_granular_sampler(g, g_plain);
  printf("== granular sampler: matrix, explicit rng states, envelope, start time, transient\n");
  std::vector<uint64_t> states(2 * 3 * 4);
  for (size_t i = 0; i < states.size(); ++i) states[i] = 0x0123456789abcdefull * (i + 1) + i;
  pg_granular_sampler_options_default(&go);
  go.params.overlap_mode = 1; go.params.window = 4; go.params.variation = 0.5f; go.params.spray = 0.25f; go.params.pan_spread = 1.0f; go.params.playback_direction = 2; go.params.position = 0.125f; go.params.step = -2.0f;
  go.modulation = &mp; go.rng_states = states.data();
  o.voice_count = 2; o.has_envelope = 1; o.envelope = env; o.transient = 1; o.start_time = 2000;
  const int g_mod = pg_graph_add_granular_sampler(g, m2, buf, &o, &go);
  CHECK(g_mod == 6);
  dump_granular_sampler(g, g_mod);
  printf("== granular sampler: matrix with all-zero explicit states (the fixed seed's fallback), derived LFO states for the next\n");
  std::vector<uint64_t> zeros(2 * 3 * 4, 0);
  go.rng_states = zeros.data();
  pg_sampler_options_default(&o);
  o.voice_count = 2;
  const int g_zero = pg_graph_add_granular_sampler(g, m1, buf_st, &o, &go);
  CHECK(g_zero == 7);
  dump_granular_sampler(g, g_zero);
  printf("== granular sampler: matrix, derived states; 9 slots (the sampler, granular-sampler and grain tables grow)\n");
  go.rng_states = nullptr;
  mp.lfo[1].rng_state[2] = 5;
  o.voice_count = 9;
  const int g_nine = pg_graph_add_granular_sampler(g, m2, buf_plain, &o, &go);
  CHECK(g_nine == 8);
  dump_granular_sampler(g, g_nine);
  printf("== granular sampler 5 and file sampler 2 again, behind the growth\n");
  dump_granular_sampler(g, g_plain);
  dump_file_sampler(g, f_big);
  printf("== granular sampler: the options' loop range over the parameters' own and the embedded one\n");
  pg_granular_sampler_options_default(&go);
  go.params.has_loop_range = 1; go.params.loop_start = 0.25f; go.params.loop_end = 0.75f;
  pg_sampler_options_default(&o);
  o.voice_count = 1; o.has_loop_range = 1; o.loop_start = 30; o.loop_end = 3000;
  const int g_loop_opt = pg_graph_add_granular_sampler(g, m1, buf, &o, &go);
  CHECK(g_loop_opt == 9);
  dump_granular_sampler(g, g_loop_opt);
  printf("== granular sampler: the parameters' own loop range over the embedded one\n");
  o.has_loop_range = 0;
  const int g_loop_par = pg_graph_add_granular_sampler(g, m1, buf, &o, &go);
  CHECK(g_loop_par == 10);
  dump_granular_sampler(g, g_loop_par);
  printf("== granular sampler: the embedded loop range; then a buffer with none\n");
  go.params.has_loop_range = 0;
  const int g_loop_emb = pg_graph_add_granular_sampler(g, m1, buf, &o, &go);
  CHECK(g_loop_emb == 11);
  dump_granular_sampler(g, g_loop_emb);
  const int g_loop_none = pg_graph_add_granular_sampler(g, m1, buf_plain, nullptr, &go);
  CHECK(g_loop_none == 12);
  dump_granular_sampler(g, g_loop_none);

  // ---- 3. lone granular voices ----
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  printf("== granular voice: owned PCM, default options, fixed seed\n");
  const int v_own = pg_graph_add_granular_voice(g, PG_MAIN_MIXER, pcm.data(), 777, &gp, nullptr);
  CHECK(v_own >= 0);
  dump_lone_voice(g, v_own);
  printf("== granular voice: owned PCM, voice options, an rng state\n");
  pg_voice_options vo;
  pg_voice_options_default(&vo);
  vo.volume = 0.5f; vo.panning = -0.75f; vo.speed = 1.5; vo.start_time = 640; vo.non_transient = 1;
  gp.position = 0.875f; gp.size = 20.0f; gp.window = 6; gp.overlap_mode = 1; gp.rng_state[1] = 0xfeedull; gp.has_loop_range = 1; gp.loop_start = 0.125f; gp.loop_end = 0.5f;
  const int v_opt = pg_graph_add_granular_voice(g, m1, pcm.data(), 500, &gp, &vo);
  CHECK(v_opt >= 0);
  dump_lone_voice(g, v_opt);
  printf("== granular voice: from a buffer with an embedded loop, default options\n");
  pg_granular_params_default(&gp);
  const int v_buf = pg_graph_add_granular_voice_from_buffer(g, PG_MAIN_MIXER, buf, &gp, nullptr);
  CHECK(v_buf >= 0);
  dump_lone_voice(g, v_buf);
  printf("== granular voice: from the stereo buffer, voice options, an rng state\n");
  gp.rng_state[0] = 1;
  const int v_buf_opt = pg_graph_add_granular_voice_from_buffer(g, m2, buf_st, &gp, &vo);
  CHECK(v_buf_opt >= 0);
  dump_lone_voice(g, v_buf_opt);
  printf("== pg_graph_set_voice_envelope: neither attack nor hold zero\n");
  CALL(pg_graph_set_voice_envelope(g, v_own, &env));
  dump_lone_voice(g, v_own);
  printf("== pg_graph_set_voice_envelope: zero attack\n");
  pg_ahdsr_params e2 = env;
  e2.attack_s = 0.0f;
  CALL(pg_graph_set_voice_envelope(g, v_opt, &e2));
  dump_lone_voice(g, v_opt);
  printf("== pg_graph_set_voice_envelope: zero attack and zero hold; then on the same voice again\n");
  e2.hold_s = 0.0f;
  CALL(pg_graph_set_voice_envelope(g, v_buf, &e2));
  dump_lone_voice(g, v_buf);
  e2.attack_s = 0.5f; e2.release_s = 0.0f;
  CALL(pg_graph_set_voice_envelope(g, v_buf, &e2));
  dump_lone_voice(g, v_buf);
  printf("== pg_graph_set_voice_modulation_matrix: fixed seeds\n");
  pg_modulation_params mp2;
  pg_modulation_params_default(&mp2);
  CALL(pg_graph_set_voice_modulation_matrix(g, v_own, &mp2));
  dump_lone_voice(g, v_own);
  printf("== pg_graph_set_voice_modulation_matrix: random shapes, rng states, routes, clamped rates\n");
  mp.lfo[0].rng_state[0] = 42;
  CALL(pg_graph_set_voice_modulation_matrix(g, v_buf_opt, &mp));
  dump_lone_voice(g, v_buf_opt);
  mp.lfo[0].rng_state[0] = 0;

  // ---- 4. messages, on a graph of their own ----
  {
    printf("== messages: a graph with a file and a granular sampler in one sub-mixer, each also starting late, each also removed\n");
    pg_graph* h = pg_graph_create(48000, 2, 256, 0);
    CHECK(h);
    d.channels = 1; d.rate = 48000; d.has_loop_range = 1; d.loop_start = 100; d.loop_end = 2900;
    CHECK(pg_graph_add_sample_buffer(h, pcm.data(), 3001, &d) == 0);
    const int hm = pg_graph_add_mixer(h);
    pg_granular_sampler_options_default(&go);
    go.modulation = &mp;
    pg_sampler_options_default(&o);
    o.voice_count = 2; o.has_envelope = 1; o.envelope = env;
    const int hf = pg_graph_add_sampler(h, hm, 0, &o), hg = pg_graph_add_granular_sampler(h, hm, 0, &o, &go);
    o.start_time = 600;
    const int hf_late = pg_graph_add_sampler(h, hm, 0, &o), hg_late = pg_graph_add_granular_sampler(h, hm, 0, &o, &go);
    o.start_time = 0;
    const int hf_gone = pg_graph_add_sampler(h, hm, 0, &o), hg_gone = pg_graph_add_granular_sampler(h, hm, 0, &o, &go);
    CHECK(hf == 0 && hg == 1 && hf_late == 2 && hg_late == 3 && hf_gone == 4 && hg_gone == 5);
    uint64_t pos = 0;
    printf("== messages: every timed call on the file sampler, in time order\n");
    send_all(h, hf, 10, false);
    write_frames(h, pos, 256);
    printf("== messages: every timed call on the granular sampler, out of time order\n");
    send_all(h, hg, pos + 10, true);
    write_frames(h, pos, 256);
    printf("== messages: in front of the start time (600), file then granular, out of order\n");
    send_all(h, hf_late, pos + 5, true);
    send_all(h, hg_late, pos + 6, false);
    write_frames(h, pos, 256);
    printf("== messages: on removed ids; events queued before the removal\n");
    CALL(pg_graph_sampler_set_parameter(h, hf_gone, ID4("STRN"), -24.0f, 0, pos + 20));
    CALL(pg_graph_sampler_set_granular_parameter(h, hg_gone, ID4("GSIZ"), 5.0f, 0, pos + 21));
    CALL(pg_graph_remove_sampler(h, hf_gone));
    CALL(pg_graph_remove_sampler(h, hg_gone));
    CALL(pg_graph_remove_sampler(h, hg_gone));
    send_all(h, hf_gone, pos + 30, false);
    send_all(h, hg_gone, pos + 30, false);
    write_frames(h, pos, 256);
    printf("== messages: the records behind the writes\n");
    dump_file_sampler(h, hf);
    dump_granular_sampler(h, hg);
    dump_host_sampler(h, hf_gone);
    dump_host_sampler(h, hg_gone);
    pg_graph_destroy(h);
  }

  // ---- 5. refusals ----
  printf("== refusals\n");
  const int NOBODY = 99;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  pg_sampler_state sst;
  pg_sampler_envelope_state ses;
  pg_modulation_state mst;
  std::unique_ptr<pg_grain_state> gst(new pg_grain_state);
  pg_param_desc pd;
  CALL(pg_graph_remove_sampler(g, g_loop_none));
  // constructors
  pg_sampler_options bad;
  pg_sampler_options_default(&bad);
  bad.voice_count = 0;
  CALLID(pg_graph_add_sampler(nullptr, m1, buf, &bad));
  bad.voice_count = 65;
  CALLID(pg_graph_add_sampler(g, m1, buf, &bad));
  pg_sampler_options_default(&bad);
  bad.has_envelope = 1; bad.envelope.sustain_level = 2.0f;
  CALLID(pg_graph_add_sampler(g, m1, buf, &bad));
  pg_sampler_options_default(&bad);
  bad.has_loop_range = 1; bad.loop_start = 5; bad.loop_end = 5;
  CALLID(pg_graph_add_sampler(g, m1, buf, &bad));
  CALLID(pg_graph_add_sampler(nullptr, m1, buf, nullptr));
  CALLID(pg_graph_add_sampler(g, PG_MAIN_MIXER, NOBODY, nullptr));
  CALLID(pg_graph_add_sampler(g, NOBODY, NOBODY, nullptr));
  CALLID(pg_graph_add_sampler(g, -1, buf, nullptr));
  CALLID(pg_graph_add_sampler(g, m1, NOBODY, nullptr));
  bad.loop_start = 3001; bad.loop_end = 3002;
  CALLID(pg_graph_add_sampler(g, m1, buf, &bad));
  bad.loop_start = 0; bad.loop_end = 3002;
  CALLID(pg_graph_add_sampler(g, m1, buf, &bad));
  pg_granular_sampler_options_default(&go);
  CALLID(pg_graph_add_granular_sampler(nullptr, m1, buf, nullptr, nullptr));
  bad.loop_start = 5; bad.loop_end = 5;
  CALLID(pg_graph_add_granular_sampler(nullptr, m1, buf, &bad, nullptr));
  go.params.size = 0.0f;
  CALLID(pg_graph_add_granular_sampler(nullptr, m1, buf, nullptr, &go));
  go.params.size = 10.0f;
  pg_modulation_params badmp;
  pg_modulation_params_default(&badmp);
  badmp.note = 128;
  go.modulation = &badmp;
  CALLID(pg_graph_add_granular_sampler(nullptr, m1, buf, nullptr, &go));
  go.modulation = nullptr;
  CALLID(pg_graph_add_granular_sampler(nullptr, m1, buf, nullptr, &go));
  CALLID(pg_graph_add_granular_sampler(g, PG_MAIN_MIXER, NOBODY, nullptr, &go));
  CALLID(pg_graph_add_granular_sampler(g, NOBODY, NOBODY, nullptr, &go));
  CALLID(pg_graph_add_granular_sampler(g, m1, NOBODY, nullptr, &go));
  bad.loop_start = 3000; bad.loop_end = 3002;
  CALLID(pg_graph_add_granular_sampler(g, m1, buf, &bad, &go));
  pg_granular_params_default(&gp);
  CALLID(pg_graph_add_granular_voice(nullptr, PG_MAIN_MIXER, pcm.data(), 10, nullptr, nullptr));
  CALLID(pg_graph_add_granular_voice(nullptr, PG_MAIN_MIXER, pcm.data(), 10, &gp, nullptr));
  CALLID(pg_graph_add_granular_voice(g, PG_MAIN_MIXER, nullptr, 10, &gp, nullptr));
  CALLID(pg_graph_add_granular_voice(g, PG_MAIN_MIXER, pcm.data(), 0, &gp, nullptr));
  CALLID(pg_graph_add_granular_voice(g, NOBODY, pcm.data(), 10, &gp, nullptr));
  pg_voice_options_default(&vo);
  vo.speed = 0.0;
  CALLID(pg_graph_add_granular_voice(g, PG_MAIN_MIXER, pcm.data(), 10, &gp, &vo));
  vo.speed = 1.0; vo.panning = 2.0f;
  CALLID(pg_graph_add_granular_voice(g, PG_MAIN_MIXER, pcm.data(), 10, &gp, &vo));
  CALLID(pg_graph_add_granular_voice_from_buffer(nullptr, PG_MAIN_MIXER, buf, &gp, nullptr));
  CALLID(pg_graph_add_granular_voice_from_buffer(g, NOBODY, buf, &gp, nullptr));
  CALLID(pg_graph_add_granular_voice_from_buffer(g, PG_MAIN_MIXER, NOBODY, &gp, nullptr));
  // the lone voices' attachments
  CALL(pg_graph_set_voice_envelope(nullptr, v_own, nullptr));
  CALL(pg_graph_set_voice_envelope(nullptr, v_own, &env));
  CALL(pg_graph_set_voice_envelope(g, NOBODY * 100, &env));
  e2 = env; e2.hold_s = -1.0f;
  CALL(pg_graph_set_voice_envelope(g, v_own, &e2));
  CALL(pg_graph_set_voice_modulation_matrix(nullptr, v_own, nullptr));
  CALL(pg_graph_set_voice_modulation_matrix(nullptr, v_own, &mp2));
  CALL(pg_graph_set_voice_modulation_matrix(g, NOBODY * 100, &mp2));
  CALL(pg_graph_set_voice_modulation_matrix(g, v_own, &badmp));
  {
    pg_voice_options fo;
    pg_voice_options_default(&fo);
    const int v_file = pg_graph_add_voice_from_buffer(g, PG_MAIN_MIXER, buf, &fo);
    CHECK(v_file >= 0);
    CALL(pg_graph_set_voice_modulation_matrix(g, v_file, &mp2) != PG_ERR_NOT_FOUND);   // (the message names the voice id)
    CALL(pg_graph_voice_grain_state(g, v_file, gst.get()) != PG_ERR_NOT_FOUND);
  }
  // descriptors
  CALL(pg_sampler_param(0, nullptr));
  CALL(pg_sampler_param(-1, &pd));
  CALL(pg_sampler_param(PG_SP_COUNT, &pd));
  CALL(pg_sampler_envelope_param(0, nullptr));
  CALL(pg_sampler_envelope_param(PG_SE_COUNT, &pd));
  for (int i = 0; i < PG_SP_COUNT; ++i) { CHECK(pg_sampler_param(i, &pd) == PG_OK); printf("  sampler_param[%d] %08x type=%d %s..%s def=%s scaling=%d,%s,%s n=%d %s\n", i, pd.fourcc, pd.type, H(pd.min).c_str(), H(pd.max).c_str(), H(pd.default_value).c_str(), pd.scaling, H(pd.scaling_arg0).c_str(), H(pd.scaling_arg1).c_str(), pd.n_values, pd.name); }
  for (int i = 0; i < PG_SE_COUNT; ++i) { CHECK(pg_sampler_envelope_param(i, &pd) == PG_OK); printf("  envelope_param[%d] %08x type=%d %s..%s def=%s scaling=%d,%s,%s n=%d %s\n", i, pd.fourcc, pd.type, H(pd.min).c_str(), H(pd.max).c_str(), H(pd.default_value).c_str(), pd.scaling, H(pd.scaling_arg0).c_str(), H(pd.scaling_arg1).c_str(), pd.n_values, pd.name); }
  for (int i = 0; i < pg_granular_param_count(); ++i) { CHECK(pg_granular_param(i, &pd) == PG_OK); printf("  granular_param[%d] %08x type=%d %s..%s def=%s scaling=%d,%s,%s n=%d %s\n", i, pd.fourcc, pd.type, H(pd.min).c_str(), H(pd.max).c_str(), H(pd.default_value).c_str(), pd.scaling, H(pd.scaling_arg0).c_str(), H(pd.scaling_arg1).c_str(), pd.n_values, pd.name); }
  CHECK(pg_effect_kind_param(PG_FX_REVERB, 0, &pd) == PG_OK);
  printf("  effect_param[reverb][0] %08x type=%d %s..%s def=%s scaling=%d,%s,%s n=%d %s\n", pd.fourcc, pd.type, H(pd.min).c_str(), H(pd.max).c_str(), H(pd.default_value).c_str(), pd.scaling, H(pd.scaling_arg0).c_str(), H(pd.scaling_arg1).c_str(), pd.n_values, pd.name);
  // the timed calls: argument errors in front of the handle check, the handle check in front of the id, the id in front of the kind
  for (int s : {f_def, f_big, g_plain, g_mod, g_loop_none, NOBODY, -1}) {
    printf("  -- sampler %d\n", s);
    CALLID(pg_graph_sampler_note_on(g, s, 60, 1.0f, 0.0f, 0));
    CALL(pg_graph_sampler_note_off(g, s, 1, 0));
    CALL(pg_graph_sampler_all_notes_off(g, s, 0));
    CALL(pg_graph_sampler_set_note_speed(g, s, 1, 1.0, 0.0f, 0));
    CALL(pg_graph_sampler_set_note_volume(g, s, 1, 1.0f, 0));
    CALL(pg_graph_sampler_set_note_panning(g, s, 1, 0.0f, 0));
    CALL(pg_graph_sampler_set_parameter(g, s, ID4("SVOL"), 1.0f, 0, 0));
    CALL(pg_graph_sampler_set_granular_parameter(g, s, ID4("GSIZ"), 10.0f, 0, 0));
    CALL(pg_graph_sampler_set_granular_parameter(g, s, ID4("GDIR"), 7.0f, 0, 0));
    CALL(pg_graph_sampler_set_envelope_parameter(g, s, ID4("AATK"), 0.5f, 0, 0));
    CALL(pg_graph_sampler_set_modulation(g, s, 0, 0, 0.5f, 0, 0));
    CALL(pg_graph_sampler_clear_modulation(g, s, 0, 0, 0));
    CALL(pg_graph_sampler_set_lfo_rate(g, s, 0, 1.0f, 0));
    CALL(pg_graph_sampler_set_lfo_waveform(g, s, 0, 1, 0));
    CALL(pg_graph_sampler_set_loop_range(g, s, 1, 10, 20, 0));
    CALL(pg_graph_sampler_set_loop_range(g, s, 1, 10, 5000, 0));
    CALL(pg_graph_sampler_set_loop_range(g, s, 1, 5000, 5001, 0));
    CALL(pg_graph_sampler_stop(g, s, 1 << 30));
    CALL(pg_graph_sampler_state(g, s, &sst));
    CALL(pg_graph_sampler_envelope_params(g, s, 0, &ses));
    CALL(pg_graph_sampler_envelope_params(g, s, -1, &ses));
    CALL(pg_graph_sampler_envelope_params(g, s, 64, &ses));
    CALL(pg_graph_sampler_voice_grain_state(g, s, 0, gst.get()));
    CALL(pg_graph_sampler_voice_grain_state(g, s, 3, gst.get()));
    CALL(pg_graph_sampler_voice_modulation_state(g, s, 0, &mst));
    CALL(pg_graph_sampler_voice_modulation_state(g, s, -1, &mst));
    CALL(pg_graph_sampler_granular_params(g, s, &gp));
  }
  printf("  -- bad arguments, with and without a handle, on sampler ids that exist and do not\n");
  for (pg_graph* q : {g, (pg_graph*)nullptr}) for (int s : {g_mod, NOBODY}) {
    printf("  -- handle %s, sampler %d\n", q ? "set" : "null", s);
    CALLID(pg_graph_sampler_note_on(q, s, 60, nan, 0.0f, 0));
    CALLID(pg_graph_sampler_note_on(q, s, 60, -1.0f, nan, 0));
    CALLID(pg_graph_sampler_note_on(q, s, 60, 1.0f, nan, 0));
    CALLID(pg_graph_sampler_note_on(q, s, 60, 1.0f, 0.0f, 0));
    CALL(pg_graph_sampler_note_off(q, s, 1, 0));
    CALL(pg_graph_sampler_all_notes_off(q, s, 0));
    CALL(pg_graph_sampler_set_note_speed(q, s, 1, 0.0, 0.0f, 0));
    CALL(pg_graph_sampler_set_note_speed(q, s, 1, (double)nan, 0.0f, 0));
    CALL(pg_graph_sampler_set_note_speed(q, s, 1, 1.0, nan, 0));
    CALL(pg_graph_sampler_set_note_volume(q, s, 1, nan, 0));
    CALL(pg_graph_sampler_set_note_volume(q, s, 1, -0.5f, 0));
    CALL(pg_graph_sampler_set_note_volume(q, s, 1, 0.5f, 0));
    CALL(pg_graph_sampler_set_note_panning(q, s, 1, nan, 0));
    CALL(pg_graph_sampler_set_note_panning(q, s, 1, 0.5f, 0));
    CALL(pg_graph_sampler_set_parameter(q, s, ID4("AATK"), nan, 0, 0));
    CALL(pg_graph_sampler_set_parameter(q, s, ID4("STRN"), nan, 1, 0));
    CALL(pg_graph_sampler_set_parameter(q, s, ID4("STRN"), 1.5f, 1, 0));
    CALL(pg_graph_sampler_set_parameter(q, s, ID4("STRN"), -0.5f, 1, 0));
    CALL(pg_graph_sampler_set_parameter(q, s, ID4("STRN"), 480.0f, 0, 0));
    CALL(pg_graph_sampler_set_granular_parameter(q, s, ID4("STRN"), nan, 0, 0));
    CALL(pg_graph_sampler_set_granular_parameter(q, s, ID4("GSIZ"), nan, 0, 0));
    CALL(pg_graph_sampler_set_granular_parameter(q, s, ID4("GVAR"), 1.5f, 1, 0));
    CALL(pg_graph_sampler_set_granular_parameter(q, s, ID4("GWND"), -3.0f, 0, 0));
    CALL(pg_graph_sampler_set_envelope_parameter(q, s, ID4("SVOL"), nan, 0, 0));
    CALL(pg_graph_sampler_set_envelope_parameter(q, s, ID4("ASTN"), nan, 0, 0));
    CALL(pg_graph_sampler_set_envelope_parameter(q, s, ID4("ASTN"), 1.5f, 1, 0));
    CALL(pg_graph_sampler_set_modulation(q, s, 4, 0, 0.5f, 0, 0));
    CALL(pg_graph_sampler_set_modulation(q, s, -1, 7, 0.5f, 0, 0));
    CALL(pg_graph_sampler_set_modulation(q, s, 0, 7, nan, 0, 0));
    CALL(pg_graph_sampler_set_modulation(q, s, 0, 0, nan, 0, 0));
    CALL(pg_graph_sampler_set_modulation(q, s, 0, 0, 1.5f, 0, 0));
    CALL(pg_graph_sampler_set_modulation(q, s, 0, 0, 1.0f, 0, 0));
    CALL(pg_graph_sampler_clear_modulation(q, s, 0, 9, 0));
    CALL(pg_graph_sampler_clear_modulation(q, s, 0, 0, 0));
    CALL(pg_graph_sampler_set_lfo_rate(q, s, 2, nan, 0));
    CALL(pg_graph_sampler_set_lfo_rate(q, s, 1, nan, 0));
    CALL(pg_graph_sampler_set_lfo_rate(q, s, 1, 3.0f, 0));
    CALL(pg_graph_sampler_set_lfo_waveform(q, s, -1, 9, 0));
    CALL(pg_graph_sampler_set_lfo_waveform(q, s, 1, 7, 0));
    CALL(pg_graph_sampler_set_lfo_waveform(q, s, 1, 6, 0));
    CALL(pg_graph_sampler_set_loop_range(q, s, 1, 20, 20, 0));
    CALL(pg_graph_sampler_set_loop_range(q, s, 0, 20, 20, 0));
    CALL(pg_graph_sampler_stop(q, s, 1 << 30));
    CALL(pg_graph_remove_sampler(q, NOBODY));
    CALL(pg_graph_sampler_state(q, s, nullptr));
    CALL(pg_graph_sampler_state(q, s, &sst));
    CALL(pg_graph_sampler_envelope_params(q, s, 99, nullptr));
    CALL(pg_graph_sampler_envelope_params(q, s, 99, &ses));
    CALL(pg_graph_sampler_voice_grain_state(q, s, 99, nullptr));
    CALL(pg_graph_sampler_voice_grain_state(q, s, 99, gst.get()));
    CALL(pg_graph_sampler_voice_modulation_state(q, s, 99, nullptr));
    CALL(pg_graph_sampler_voice_modulation_state(q, s, 99, &mst));
    CALL(pg_graph_sampler_granular_params(q, s, nullptr));
    CALL(pg_graph_sampler_granular_params(q, s, &gp));
  }
  // the lone voices' timed calls and read-backs that share code with the samplers'
  CALL(pg_graph_voice_grain_state(g, NOBODY * 100, gst.get()));
  CALL(pg_graph_voice_grain_state(nullptr, v_own, gst.get()));
  CALL(pg_graph_voice_modulation_state(g, v_buf, &mst));
  CALL(pg_graph_voice_modulation_state(g, v_own, nullptr));
  CALL(pg_graph_voice_granular_params(g, NOBODY * 100, &gp));
  CALL(pg_graph_set_voice_granular_parameter(nullptr, v_own, ID4("GSIZ"), nan, 0, 0));
  CALL(pg_graph_set_voice_granular_parameter(nullptr, v_own, ID4("GSIZ"), 5.0f, 0, 0));
  CALL(pg_graph_set_voice_granular_parameter(g, NOBODY * 100, ID4("GWND"), 50.0f, 0, 0));
  CALL(pg_graph_set_voice_granular_parameter(g, v_own, ID4("GWND"), 50.0f, 0, 0));

  // ---- 6. read-backs ----
  printf("== read-backs: a file sampler with an envelope, a granular sampler with a matrix and an envelope\n");
  print_readbacks(g, f_big, 63);
  print_readbacks(g, g_mod, 1);
  printf("== read-backs: a file sampler and a granular sampler without envelope and matrix\n");
  print_readbacks(g, f_def, 0);
  print_readbacks(g, g_plain, 2);
  printf("== read-backs: the lone voices\n");
  {
    int rc = pg_graph_voice_grain_state(g, v_opt, gst.get());
    print_grain_state("pg_graph_voice_grain_state(v_opt)", rc, *gst);
    rc = pg_graph_voice_modulation_state(g, v_buf_opt, &mst);
    print_modulation_state("pg_graph_voice_modulation_state(v_buf_opt)", rc, mst);
    rc = pg_graph_voice_granular_params(g, v_buf, &gp);
    print_granular_params("pg_graph_voice_granular_params(v_buf)", rc, gp);
    printf("  pg_graph_voice_envelope_stage: %d %d %d %d\n", pg_graph_voice_envelope_stage(g, v_own), pg_graph_voice_envelope_stage(g, v_opt), pg_graph_voice_envelope_stage(g, v_buf), pg_graph_voice_envelope_stage(g, v_buf_opt));
  }
  printf("== read-backs: transient samplers whose `stopped` word is set, before and behind the write that retires them; a non-transient one\n");
  g->samp_stopped[(size_t)f_big] = 1;
  g->samp_stopped[(size_t)g_mod] = 1;
  g->samp_stopped[(size_t)f_one] = 1;
  print_readbacks(g, f_big, 0);
  {
    uint64_t pos = 0;
    write_frames(g, pos, 64);
  }
  dump_host_sampler(g, f_big);
  dump_host_sampler(g, g_mod);
  dump_host_sampler(g, f_one);
  print_readbacks(g, f_big, 0);
  print_readbacks(g, g_mod, 0);
  print_sampler_state(g, f_one);
  CALL(pg_graph_sampler_note_off(g, f_big, 1, 0));
  CALL(pg_graph_remove_sampler(g, g_mod));
  CALL(pg_graph_remove_sampler(g, f_one));
  {
    uint64_t pos = 64;
    write_frames(g, pos, 64);
  }
  print_sampler_state(g, f_one);
  print_envelope_params(g, f_one, 0);
  CALL(pg_graph_sampler_granular_params(g, g_loop_none, &gp));

  pg_graph_destroy(g);
  hip_stub_set_observer(nullptr);
  pg_debug_hip_calls(c1);
  if (c1[0] - c0[0] != c1[1] - c0[1]) { fprintf(stderr, "%llu allocations, %llu frees\n", (unsigned long long)(c1[0] - c0[0]), (unsigned long long)(c1[1] - c0[1])); return 1; }
  printf("== done: %llu allocations, as many frees\n", (unsigned long long)(c1[0] - c0[0]));
  return 0;
}
