// The host side of the sampler messages that change every voice while notes sound (pg_graph_sampler_set_envelope_parameter, _set_modulation,
// _clear_modulation, _set_lfo_rate, _set_lfo_waveform, _set_loop_range, pg_graph_sampler_envelope_params) against the stub HIP runtime
// (hip_stub.cpp), built with -fsanitize=address,undefined: every call on a file sampler with and without an envelope and on a granular sampler
// with and without a matrix, the refusals that need a graph, messages out of time order, in front of the start time, on removed ids, with events
// queued at remove and destroy — allocations and releases must balance. Through the stub's observer it reads the COMMAND RECORDS the host wrote
// for the launches (a graph with a living granular sampler sends every piece's list by copy, and every event of that sampler's mixer is a
// boundary launch of pg_gsampler_kernel that names the list): the values sampler_stage_command resolved must be those of the TIME-ordered
// sequence, whatever the sending order was. "Device" memory is malloc'ed and no kernel runs, so nothing the device decides is checked here.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_stub_observer.h"
#include "../../phonic_amd/csrc/pg_host_internal.h"   // PgGSamplerLaunch, PgCmd: what the observer reads of a launch's argument

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, pg_last_error_message()); exit(1); } } while (0)
#define ID4(s) PG_FOURCC(s[0], s[1], s[2], s[3])

// the sampler commands of the new kinds, as the boundary launch at their frame finds them in its piece's list
struct Seen { uint64_t t; PgCmd c; };
static std::vector<Seen> g_seen;
static int observe(const StubCall* c) {
  if (c->kind != STUB_LAUNCH || !c->name || !strstr(c->name, "pg_gsampler_kernel")) return 0;
  const PgGSamplerLaunch* L = (const PgGSamplerLaunch*)c->args[0];
  if (L->closing || !L->cmds) return 0;
  for (int i = 0; i < L->n_cmds; ++i) {
    const PgCmd& cmd = L->cmds[i];
    if (cmd.frame == L->frame && cmd.type >= CMD_SAMPLER_ENV_PARAM && cmd.type <= CMD_SAMPLER_GRAIN_LOOP) g_seen.push_back({L->t, cmd});
  }
  return 0;
}
static void write_frames(pg_graph* g, uint64_t& pos, size_t frames) {
  std::vector<float> out(frames * 2);
  (void)pg_graph_write(g, out.data(), out.size(), pos);
  pos += frames;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
// one expected record: (sample time, sampler, command type, param / low words, value, value64)
struct Want { uint64_t t; int target, type, param; float value; uint64_t value64; };
static void expect(const std::vector<Want>& want, int line) {
  bool ok = g_seen.size() == want.size();
  for (size_t i = 0; ok && i < want.size(); ++i) {
    const PgCmd& c = g_seen[i].c;
    ok = g_seen[i].t == want[i].t && c.target == want[i].target && c.type == want[i].type && c.param == want[i].param && bits(c.value) == bits(want[i].value) && c.value64 == want[i].value64;
  }
  if (!ok) {
    fprintf(stderr, "line %d: the command records differ from the time-ordered sequence\n", line);
    for (const Seen& s : g_seen) fprintf(stderr, "  got  t=%llu target=%d type=%d param=%d value=%.9g value64=%llx\n", (unsigned long long)s.t, s.c.target, s.c.type, s.c.param, (double)s.c.value, (unsigned long long)s.c.value64);
    for (const Want& w : want) fprintf(stderr, "  want t=%llu target=%d type=%d param=%d value=%.9g value64=%llx\n", (unsigned long long)w.t, w.target, w.type, w.param, (double)w.value, (unsigned long long)w.value64);
    exit(1);
  }
  g_seen.clear();
}

int main() {
  uint64_t c0[4], c1[4];
  pg_debug_hip_calls(c0);
  const float SR = 48000.0f;
  pg_graph* g = pg_graph_create(48000, 2, 256, 0);
  CHECK(g);
  std::vector<float> pcm(3001);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (float)((i * 37) % 101) / 101.0f - 0.5f;
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = 1; d.rate = 48000; d.has_loop_range = 1; d.loop_start = 100; d.loop_end = 2900;
  const int buf = pg_graph_add_sample_buffer(g, pcm.data(), 3001, &d);
  CHECK(buf == 0);
  const int m1 = pg_graph_add_mixer(g);
  CHECK(m1 > 0);

  // ---- the five kinds of sampler, all in one sub-mixer: every event of it is a boundary of the granular ones ----
  pg_sampler_options o;
  pg_sampler_options_default(&o);
  o.voice_count = 33; o.has_envelope = 1;
  o.envelope.attack_s = 0.002f; o.envelope.hold_s = 0.003f; o.envelope.decay_s = 0.004f; o.envelope.sustain_level = 0.6f; o.envelope.release_s = 0.005f;
  const int f_env = pg_graph_add_sampler(g, m1, buf, &o);                 // a file sampler with an envelope, voices beyond lane 32
  pg_granular_sampler_options go;
  pg_granular_sampler_options_default(&go);
  go.params.size = 3.0f; go.params.density = 100.0f;
  pg_modulation_params mp;
  pg_modulation_params_default(&mp);
  go.modulation = &mp;
  o.voice_count = 3;
  const int g_mod = pg_graph_add_granular_sampler(g, m1, buf, &o, &go);   // granular, envelope, matrix
  o.start_time = 2000;
  const int g_late = pg_graph_add_granular_sampler(g, m1, buf, &o, &go);  // ... that starts at frame 2000
  pg_sampler_options_default(&o);
  o.voice_count = 2;
  const int f_plain = pg_graph_add_sampler(g, m1, buf, &o);               // a file sampler without an envelope
  go.modulation = nullptr;
  const int g_plain = pg_graph_add_granular_sampler(g, m1, buf, &o, &go); // granular, no envelope, no matrix
  o.has_envelope = 1;
  const int f_gone = pg_graph_add_sampler(g, m1, buf, &o);                // removed below with events queued
  CHECK(f_env == 0 && g_mod == 1 && g_late == 2 && f_plain == 3 && g_plain == 4 && f_gone == 5);

  // ---- descriptors ----
  CHECK(pg_sampler_envelope_param_count() == 5);
  pg_param_desc pd;
  const char* ids[5] = {"AATK", "AHLD", "ADCY", "ASTN", "AREL"};
  for (int i = 0; i < 5; ++i) CHECK(pg_sampler_envelope_param(i, &pd) == PG_OK && pd.fourcc == ID4(ids[i]) && pd.min == 0.0f && pd.max == (i == 3 ? 1.0f : 10.0f));

  // ---- refusals that need a graph ----
  CHECK(pg_graph_sampler_set_envelope_parameter(g, f_plain, ID4("AATK"), 0.1f, 0, 0) == PG_ERR_PARAMETER && strstr(pg_last_error_message(), "no envelope"));
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_plain, ID4("ASTN"), 0.1f, 0, 0) == PG_ERR_PARAMETER);
  CHECK(pg_graph_sampler_set_envelope_parameter(g, 99, ID4("ASTN"), 0.1f, 0, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_envelope_parameter(g, -1, ID4("ASTN"), 0.1f, 0, 0) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_set_parameter(g, f_env, ID4("AATK"), 0.1f, 0, 0) == PG_ERR_PARAMETER);   // the base parameters' call keeps refusing AMP_*
  for (int s : {f_env, f_plain}) {   // "only available when granular playback is enabled"
    CHECK(pg_graph_sampler_set_modulation(g, s, 0, 0, 0.5f, 1, 0) == PG_ERR_STATE && pg_graph_sampler_clear_modulation(g, s, 0, 0, 0) == PG_ERR_STATE);
    CHECK(pg_graph_sampler_set_lfo_rate(g, s, 0, 1.0f, 0) == PG_ERR_STATE && pg_graph_sampler_set_lfo_waveform(g, s, 0, 1, 0) == PG_ERR_STATE);
    CHECK(pg_graph_sampler_set_loop_range(g, s, 1, 10, 20, 0) == PG_ERR_STATE && pg_graph_sampler_set_loop_range(g, s, 0, 0, 0, 0) == PG_ERR_STATE);
  }
  CHECK(pg_graph_sampler_set_modulation(g, g_plain, 0, 0, 0.5f, 1, 0) == PG_ERR_STATE && strstr(pg_last_error_message(), "no modulation matrix"));
  CHECK(pg_graph_sampler_set_lfo_rate(g, g_plain, 0, 1.0f, 0) == PG_ERR_STATE && pg_graph_sampler_set_lfo_waveform(g, g_plain, 1, 2, 0) == PG_ERR_STATE);
  CHECK(pg_graph_sampler_set_modulation(g, 99, 0, 0, 0.5f, 1, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_lfo_rate(g, 99, 0, 1.0f, 0) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_set_lfo_waveform(g, 99, 0, 1, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_loop_range(g, 99, 1, 1, 2, 0) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_set_modulation(g, 99, 9, 0, 0.5f, 1, 0) == PG_ERR_PARAMETER);   // the argument check comes first
  CHECK(pg_graph_sampler_set_loop_range(g, g_plain, 1, 3001, 3002, 0) == PG_ERR_PARAMETER && pg_graph_sampler_set_loop_range(g, g_plain, 1, 0, 3002, 0) == PG_ERR_PARAMETER);
  CHECK(pg_graph_sampler_set_loop_range(g, g_plain, 1, 3000, 3001, 0) == PG_OK);          // the last frame alone: inside
  pg_sampler_envelope_state es;
  CHECK(pg_graph_sampler_envelope_params(g, f_plain, 0, &es) == PG_ERR_STATE && pg_graph_sampler_envelope_params(g, g_plain, 0, &es) == PG_ERR_STATE);
  CHECK(pg_graph_sampler_envelope_params(g, f_env, 33, &es) == PG_ERR_PARAMETER && pg_graph_sampler_envelope_params(g, g_mod, 3, &es) == PG_ERR_PARAMETER);
  CHECK(pg_graph_sampler_envelope_params(g, g_mod, -1, &es) == PG_ERR_PARAMETER && pg_graph_sampler_envelope_params(g, 99, 0, &es) == PG_ERR_NOT_FOUND);
  const float decay0 = (1.0f - 0.6f) / (0.004f * SR);
  for (int slot : {0, 32}) {
    CHECK(pg_graph_sampler_envelope_params(g, f_env, slot, &es) == PG_OK && es.sustain_level == 0.6f && es.decay_rate == decay0 && es.attack_rate == 1.0f / (0.002f * SR));
    CHECK(es.hold_samples == 0.003f * SR && es.release_rate == 1.0f / (0.005f * SR) && es.zero_times == 0 && es.attack_scaling == 0.0f);
  }
  CHECK(pg_graph_sampler_envelope_params(g, g_mod, 2, &es) == PG_OK && es.sustain_level == 0.6f && es.decay_rate == decay0 && es.zero_times == 0);

  // ---- messages out of time order: the records carry what the TIME-ordered setters compute ----
  hip_stub_set_observer(observe);
  uint64_t pos = 0;
  CHECK(pg_graph_sampler_note_on(g, f_env, 60, 1.0f, 0.0f, 10) > 0 && pg_graph_sampler_note_on(g, g_mod, 60, 1.0f, 0.0f, 10) > 0);
  CHECK(pg_graph_sampler_set_envelope_parameter(g, f_env, ID4("ADCY"), 0.008f, 0, 200) == PG_OK);      // sent first, due last: it must divide by the NEW sustain
  CHECK(pg_graph_sampler_set_envelope_parameter(g, f_env, ID4("ASTN"), 0.2f, 0, 100) == PG_OK);
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_mod, ID4("ASTN"), 0.5f, 1, 150) == PG_OK);        // normalized, linear
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_mod, ID4("ADCY"), 0.5f, 1, 160) == PG_OK);        // normalized, Exponential(2.0): 2.5 s
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_mod, ID4("AREL"), 0.6e-9f, 0, 140) == PG_OK);     // 1 ns
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_mod, ID4("AHLD"), 0.0f, 0, 130) == PG_OK);
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_mod, ID4("AATK"), 4e-10f, 0, 120) == PG_OK);      // a zero Duration
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_mod, ID4("ADCY"), 12.0f, 0, 121) == PG_OK);       // clamped to 10 s; sustain still 0.6
  write_frames(g, pos, 256);
  const float ns = 1.0f / 1e9f;
  expect({{0, g_plain, CMD_SAMPLER_GRAIN_LOOP, 0, 3000.0f / 3001.0f, 1 | (uint64_t)bits(1.0f) << 32},   // (the accepted call above, stamped 0: the first frame)
          {100, f_env, CMD_SAMPLER_ENV_PARAM, PG_SE_SUSTAIN, 0.2f, 0},
          {120, g_mod, CMD_SAMPLER_ENV_PARAM, PG_SE_ATTACK, FLT_MAX, 0},
          {121, g_mod, CMD_SAMPLER_ENV_PARAM, PG_SE_DECAY, (1.0f - 0.6f) / (10.0f * SR), 0},
          {130, g_mod, CMD_SAMPLER_ENV_PARAM, PG_SE_HOLD, 0.0f, PG_AHDSR_HOLD_ZERO},
          {140, g_mod, CMD_SAMPLER_ENV_PARAM, PG_SE_RELEASE, 1.0f / (ns * SR), PG_AHDSR_HOLD_ZERO},
          {150, g_mod, CMD_SAMPLER_ENV_PARAM, PG_SE_SUSTAIN, 0.5f, PG_AHDSR_HOLD_ZERO},
          {160, g_mod, CMD_SAMPLER_ENV_PARAM, PG_SE_DECAY, (1.0f - 0.5f) / (2.5f * SR), PG_AHDSR_HOLD_ZERO},
          {200, f_env, CMD_SAMPLER_ENV_PARAM, PG_SE_DECAY, (1.0f - 0.2f) / ((8000000.0f / 1e9f) * SR), 0}}, __LINE__);

  // ---- the matrix's and the loop range's records: the words of the lone voices' commands ----
  CHECK(pg_graph_sampler_set_loop_range(g, g_mod, 0, 7, 3, pos + 90) == PG_OK);                         // None: the numbers are not read
  CHECK(pg_graph_sampler_set_loop_range(g, g_mod, 1, 300, 1500, pos + 80) == PG_OK);
  CHECK(pg_graph_sampler_set_lfo_waveform(g, g_mod, 1, 6, pos + 70) == PG_OK);
  CHECK(pg_graph_sampler_set_lfo_rate(g, g_mod, 0, 100.0f, pos + 60) == PG_OK);                          // clamped to 20 Hz
  CHECK(pg_graph_sampler_clear_modulation(g, g_mod, 3, 6, pos + 50) == PG_OK);
  CHECK(pg_graph_sampler_set_modulation(g, g_mod, 1, 2, 0.0005f, 1, pos + 40) == PG_OK);                 // below the threshold: removed, not bipolar
  CHECK(pg_graph_sampler_set_modulation(g, g_mod, 3, 6, -0.75f, 1, pos + 30) == PG_OK);
  write_frames(g, pos, 256);
  const uint64_t e1500 = (uint64_t)bits(1500.0f / 3001.0f) << 32;
  expect({{256 + 30, g_mod, CMD_SAMPLER_MOD_ROUTE, 0, -0.75f, 3 | (6 << 8) | (1 << 16)},
          {256 + 40, g_mod, CMD_SAMPLER_MOD_ROUTE, 0, 0.0f, 1 | (2 << 8)},
          {256 + 50, g_mod, CMD_SAMPLER_MOD_ROUTE, 0, 0.0f, 3 | (6 << 8)},
          {256 + 60, g_mod, CMD_SAMPLER_LFO_RATE, 0, (float)(20.0 / 48000.0), 0},
          {256 + 70, g_mod, CMD_SAMPLER_LFO_WAVEFORM, 0, 0.0f, 1 | (6 << 8)},
          {256 + 80, g_mod, CMD_SAMPLER_GRAIN_LOOP, 0, 300.0f / 3001.0f, 1 | e1500},
          {256 + 90, g_mod, CMD_SAMPLER_GRAIN_LOOP, 0, 0.0f, 0}}, __LINE__);

  // ---- in front of the start time: applied AT the start time, in the order of the stamps; a no-op cut where each was stamped ----
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_late, ID4("ADCY"), 0.004f, 0, pos + 20) == PG_OK);   // stamped later: it sees sustain 0.3
  CHECK(pg_graph_sampler_set_envelope_parameter(g, g_late, ID4("ASTN"), 0.3f, 0, pos + 10) == PG_OK);
  CHECK(pg_graph_sampler_set_modulation(g, g_late, 0, 0, 0.25f, 0, pos + 15) == PG_OK);
  write_frames(g, pos, 256);
  expect({}, __LINE__);                                                                                  // nothing reaches the sampler before frame 2000
  write_frames(g, pos, 1500);
  expect({{2000, g_late, CMD_SAMPLER_ENV_PARAM, PG_SE_SUSTAIN, 0.3f, 0},
          {2000, g_late, CMD_SAMPLER_MOD_ROUTE, 0, 0.25f, 0},
          {2000, g_late, CMD_SAMPLER_ENV_PARAM, PG_SE_DECAY, (1.0f - 0.3f) / ((4000000.0f / 1e9f) * SR), 0}}, __LINE__);

  // ---- a removed id: its queued events become no-ops, later calls find nothing ----
  CHECK(pg_graph_sampler_set_envelope_parameter(g, f_gone, ID4("ASTN"), 0.1f, 0, pos + 100) == PG_OK);
  CHECK(pg_graph_sampler_set_envelope_parameter(g, f_gone, ID4("ADCY"), 1.0f, 0, pos + 50000) == PG_OK);
  write_frames(g, pos, 64);                                                                              // the events are queued in the mixer now
  CHECK(pg_graph_remove_sampler(g, f_gone) == PG_OK);
  CHECK(pg_graph_sampler_set_envelope_parameter(g, f_gone, ID4("ASTN"), 0.1f, 0, 0) == PG_ERR_NOT_FOUND);
  write_frames(g, pos, 256);
  expect({}, __LINE__);
  CHECK(pg_graph_sampler_envelope_params(g, f_gone, 0, &es) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_remove_sampler(g, g_late) == PG_OK);
  for (int s : {f_gone, g_late}) {
    CHECK(pg_graph_sampler_set_modulation(g, s, 0, 0, 0.5f, 1, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_lfo_rate(g, s, 0, 1.0f, 0) == PG_ERR_NOT_FOUND);
    CHECK(pg_graph_sampler_set_lfo_waveform(g, s, 0, 1, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_loop_range(g, s, 1, 1, 2, 0) == PG_ERR_NOT_FOUND);
  }
  write_frames(g, pos, 100);
  hip_stub_set_observer(nullptr);

  // ---- destroy with events of every new kind queued ----
  for (uint64_t t : {pos + 999999, pos + 5}) {
    CHECK(pg_graph_sampler_set_envelope_parameter(g, f_env, ID4("AREL"), 0.0f, 0, t) == PG_OK && pg_graph_sampler_set_envelope_parameter(g, g_mod, ID4("AATK"), 1.0f, 1, t) == PG_OK);
    CHECK(pg_graph_sampler_set_modulation(g, g_mod, 2, 1, 1.0f, 0, t) == PG_OK && pg_graph_sampler_set_lfo_rate(g, g_mod, 1, 0.001f, t) == PG_OK);
    CHECK(pg_graph_sampler_set_lfo_waveform(g, g_mod, 0, 0, t) == PG_OK && pg_graph_sampler_set_loop_range(g, g_mod, 1, 0, 3001, t) == PG_OK);
  }
  write_frames(g, pos, 1);   // drained into the mixer's list; the late ones stay queued
  pg_graph_destroy(g);
  pg_debug_hip_calls(c1);
  if (c1[0] - c0[0] != c1[1] - c0[1]) { fprintf(stderr, "%llu allocations, %llu frees\n", (unsigned long long)(c1[0] - c0[0]), (unsigned long long)(c1[1] - c0[1])); return 1; }
  printf("ok\n");
  return 0;
}
