// The host side of the granular-mode samplers (pg_graph_add_granular_sampler, the pg_graph_sampler_* messages on such a sampler,
// pg_graph_sampler_set_granular_parameter, the three read-backs) against the stub HIP runtime (hip_stub.cpp), built with -fsanitize=address,undefined:
// add, messages in and out of time order, the refusals, remove with notes sounding, a mixer removed with its sampler, destroy with live samplers —
// allocations and releases must balance — and, through the stub's observer, the ORDER of the launches a write enqueues per span of the sampler's
// source-write grid:  pg_gsampler_kernel (close / open), pg_grain_kernel, ..., pg_gsampler_kernel (closing), then the unit kernels.
// "Device" memory is malloc'ed and no kernel runs, so nothing the device decides is checked here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_stub_observer.h"
#include "../../phonic_amd/csrc/pg_host_internal.h"   // PgGSamplerLaunch, PgGrainLaunch: what the observer reads of a launch's argument

#define EXPECT_TRACE(want) do { const std::string got_ = span_trace(); if (got_ != (want)) { fprintf(stderr, "%s:%d: launches \"%s\", expected \"%s\"\n", __FILE__, __LINE__, got_.c_str(), want); exit(1); } } while (0)
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, pg_last_error_message()); exit(1); } } while (0)

// 'n' pg_gsampler_kernel (with the boundary's position and kind), 'g' pg_grain_kernel (with its span), 'u' any other kernel
struct Launch { char kind; uint64_t t; uint32_t n; int first, closing; };
static std::vector<Launch> g_launches;
static int observe(const StubCall* c) {
  if (c->kind != STUB_LAUNCH) return 0;
  const std::string name = c->name ? c->name : "?";
  Launch l = {'u', 0, 0, 0, 0};
  if (name.find("pg_gsampler_kernel") != std::string::npos) {
    const PgGSamplerLaunch* L = (const PgGSamplerLaunch*)c->args[0];
    l = {'n', L->t, 0, L->chunk_first, L->closing};
  } else if (name.find("pg_grain_kernel") != std::string::npos) {
    const PgGrainLaunch* L = (const PgGrainLaunch*)c->args[0];
    l = {'g', L->t0, L->n, 0, 0};
  }
  g_launches.push_back(l);
  return 0;
}

static void write_frames(pg_graph* g, uint64_t& pos, size_t frames) {
  std::vector<float> out(frames * 2);
  g_launches.clear();
  (void)pg_graph_write(g, out.data(), out.size(), pos);
  pos += frames;
}
// The launches of the last write (one chunk) from the first of the note layer up to the first unit kernel: the boundaries' positions and the grain spans, as a string like
// "N0 G0+100 n100 G100+156 c256 |" (N: chunk start, n: inner boundary, c: closing, G: grain span)
static std::string span_trace() {
  std::string s;
  char buf[64];
  size_t i = 0;
  while (i < g_launches.size() && g_launches[i].kind == 'u') ++i;   // (what the write's prologue enqueues: topology patches, uploads)
  for (; i < g_launches.size() && g_launches[i].kind != 'u'; ++i) {
    const Launch& l = g_launches[i];
    if (l.kind == 'n') snprintf(buf, sizeof buf, "%c%llu ", l.closing ? 'c' : (l.first ? 'N' : 'n'), (unsigned long long)l.t);
    else snprintf(buf, sizeof buf, "G%llu+%u ", (unsigned long long)l.t, l.n);
    s += buf;
  }
  for (; i < g_launches.size(); ++i) if (g_launches[i].kind != 'u') return s + "| LATE";   // nothing of the note layer stands behind a unit kernel of the chunk
  return s + "|";
}
static int use_count(pg_graph* g, int buffer) {
  pg_sample_buffer_info info;
  CHECK(pg_graph_sample_buffer_info(g, buffer, &info) == PG_OK);
  return info.use_count;
}

int main() {
  uint64_t c0[4], c1[4];
  pg_debug_hip_calls(c0);
  pg_graph* g = pg_graph_create(48000, 2, 256, 0);
  CHECK(g);
  std::vector<float> pcm(3001);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (float)((i * 37) % 101) / 101.0f - 0.5f;
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = 1; d.rate = 48000; d.has_loop_range = 1; d.loop_start = 100; d.loop_end = 2900;
  const int buf = pg_graph_add_sample_buffer(g, pcm.data(), 3001, &d);
  CHECK(buf == 0);
  const int m1 = pg_graph_add_mixer(g), m2 = pg_graph_add_mixer_to(g, m1), m3 = pg_graph_add_mixer(g);
  CHECK(m1 > 0 && m2 > 0 && m3 > 0);
  const int fx = pg_graph_add_effect(g, m3, PG_FX_GAIN, nullptr);
  CHECK(fx >= 0);

  // ---- construction and refusals ----
  pg_sampler_options o;
  pg_sampler_options_default(&o);
  pg_granular_sampler_options go;
  pg_granular_sampler_options_default(&go);
  go.params.size = 3.0f; go.params.density = 100.0f;
  CHECK(pg_graph_add_granular_sampler(g, PG_MAIN_MIXER, buf, &o, &go) == -PG_ERR_PARAMETER && strstr(pg_last_error_message(), "sub-mixer"));
  CHECK(pg_graph_add_granular_sampler(g, 99, buf, &o, &go) == -PG_ERR_NOT_FOUND && pg_graph_add_granular_sampler(g, m1, 99, &o, &go) == -PG_ERR_NOT_FOUND);
  CHECK(pg_graph_add_granular_sampler(g, m1, buf, &o, nullptr) == -PG_ERR_PARAMETER);
  o.has_loop_range = 1; o.loop_start = 10; o.loop_end = 3002;
  CHECK(pg_graph_add_granular_sampler(g, m1, buf, &o, &go) == -PG_ERR_PARAMETER);   // the range leaves the buffer
  pg_sampler_options_default(&o);
  CHECK(use_count(g, buf) == 0);
  const int s0 = pg_graph_add_granular_sampler(g, m3, buf, nullptr, &go);            // 8 slots, no matrix
  CHECK(s0 == 0 && use_count(g, buf) == 8);
  pg_modulation_params mp;
  pg_modulation_params_default(&mp);
  mp.routes[0][0].amount = 0.5f; mp.routes[0][0].bipolar = 1; mp.lfo[1].waveform = 5;
  std::vector<uint64_t> states(64 * 3 * 4);
  for (size_t i = 0; i < states.size(); ++i) states[i] = 0x9E3779B97F4A7C15ull * (i + 1);
  o.voice_count = 64; o.has_envelope = 1; o.transient = 1; o.start_time = 9000;   // (behind the writes whose launches are read below: a start time inside a chunk is a boundary)
  go.modulation = &mp; go.rng_states = states.data();
  const int s1 = pg_graph_add_granular_sampler(g, m2, buf, &o, &go);                 // the largest pool, enveloped, a matrix, explicit states, nested
  CHECK(s1 == 1 && use_count(g, buf) == 72);
  pg_sampler_options_default(&o);
  const int file_sampler = pg_graph_add_sampler(g, m1, buf, &o);                     // a FILE sampler beside them
  CHECK(file_sampler == 2);
  go.rng_states = nullptr;
  std::vector<int> more;
  o.voice_count = 2;
  for (int i = 0; i < 5; ++i) { more.push_back(pg_graph_add_granular_sampler(g, m1, buf, &o, &go)); CHECK(more.back() == 3 + i); }   // the tables grow
  pg_sampler_state st;
  CHECK(pg_graph_sampler_state(g, s1, &st) == PG_OK && st.voice_count == 64 && st.active_voices == 0 && st.slots[63].envelope_stage == 0 && st.slots[0].note == 60);
  CHECK(pg_graph_sampler_state(g, s0, &st) == PG_OK && st.voice_count == 8 && st.slots[7].envelope_stage == -1 && st.slots[3].release_start_frame == UINT64_MAX && st.volume == 1.0f);
  std::vector<pg_grain_state> gs(1);
  pg_modulation_state ms;
  pg_granular_params gp;
  CHECK(pg_graph_sampler_voice_grain_state(g, s1, 63, gs.data()) == PG_OK && gs[0].rng_state[0] == states[(63 * 3) * 4] && gs[0].trigger_phase == 0.0f && gs[0].primary_slot == -1);
  CHECK(pg_graph_sampler_voice_modulation_state(g, s1, 5, &ms) == PG_OK && ms.routes[0][0].amount == 0.5f && ms.velocity == 0.0f && ms.lfo[1].waveform == 5);
  CHECK(pg_graph_sampler_granular_params(g, s1, &gp) == PG_OK && gp.size == 3.0f && gp.has_loop_range == 1 && gp.loop_start == 100.0f / 3001.0f);   // the buffer's embedded loop
  uint64_t derived[4];
  pg_granular_sampler_rng_state(go.params.rng_state, 7, 0, derived);
  CHECK(pg_graph_sampler_voice_grain_state(g, s0, 7, gs.data()) == PG_OK && memcmp(gs[0].rng_state, derived, sizeof derived) == 0);
  CHECK(pg_graph_sampler_voice_grain_state(g, s0, 8, gs.data()) == PG_ERR_PARAMETER && pg_graph_sampler_voice_grain_state(g, s0, -1, gs.data()) == PG_ERR_PARAMETER);
  CHECK(pg_graph_sampler_voice_modulation_state(g, s0, 0, &ms) == PG_ERR_STATE);      // no matrix
  // a file sampler given a granular call, unknown ids
  CHECK(pg_graph_sampler_set_granular_parameter(g, file_sampler, PG_FOURCC('G', 'S', 'I', 'Z'), 5.0f, 0, 0) == PG_ERR_STATE);
  CHECK(pg_graph_sampler_voice_grain_state(g, file_sampler, 0, gs.data()) == PG_ERR_STATE && pg_graph_sampler_granular_params(g, file_sampler, &gp) == PG_ERR_STATE);
  CHECK(pg_graph_sampler_voice_modulation_state(g, file_sampler, 0, &ms) == PG_ERR_STATE);
  CHECK(pg_graph_sampler_set_granular_parameter(g, 99, PG_FOURCC('G', 'S', 'I', 'Z'), 5.0f, 0, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_granular_params(g, 99, &gp) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_set_granular_parameter(g, s0, PG_FOURCC('G', 'D', 'I', 'R'), 7.0f, 0, 0) == PG_OK);   // a raw enum index out of range: ignored

  // ---- the launch order per span (s0 sits in m3 with a Gain: its events are the mixer's other events) ----
  hip_stub_set_observer(observe);
  uint64_t pos = 0;
  write_frames(g, pos, 256);                                   // a piece with 0 cuts
  EXPECT_TRACE("N0 G0+256 c256 |");
  CHECK(pg_graph_sampler_note_on(g, s0, 60, 1.0f, 0.0f, 256 + 100) > 0);
  write_frames(g, pos, 256);                                   // 1 cut
  EXPECT_TRACE("N256 G256+100 n356 G356+156 c512 |");
  CHECK(pg_graph_sampler_note_on(g, s0, 62, 1.0f, 0.0f, 512 + 200) > 0 && pg_graph_schedule_param(g, fx, PG_FOURCC('g', 'a', 'i', 'n'), 1.0f, 0, 512 + 31) == PG_OK);
  CHECK(pg_graph_sampler_set_granular_parameter(g, s0, PG_FOURCC('G', 'S', 'I', 'Z'), 9.0f, 0, 512 + 32) == PG_OK);   // sent later ...
  write_frames(g, pos, 256);                                   // 3 cuts: an effect's event, a parameter, a note
  EXPECT_TRACE("N512 G512+31 n543 G543+1 n544 G544+168 n712 G712+56 c768 |");
  CHECK(pg_graph_sampler_note_on(g, s0, 64, 1.0f, 0.0f, 768 + 256) > 0);
  write_frames(g, pos, 600);                                   // a cut on a piece edge: pieces at 768, 1024, 1280
  EXPECT_TRACE("N768 G768+256 n1024 G1024+344 c1368 |");
  const int64_t a = pg_graph_sampler_note_on(g, s0, 65, 1.0f, 0.0f, 1400), b = pg_graph_sampler_note_on(g, s0, 66, 1.0f, 0.0f, 1400);
  CHECK(a > 0 && b > a && pg_graph_sampler_note_off(g, s0, a, 1400) == PG_OK);
  write_frames(g, pos, 100);                                   // three messages on one frame: ONE boundary
  EXPECT_TRACE("N1368 G1368+32 n1400 G1400+68 c1468 |");
  write_frames(g, pos, 4096 + 10);                             // two chunks: each closes its own last span
  {
    std::vector<uint64_t> chunk_starts;
    for (const Launch& l : g_launches) if (l.kind == 'n' && l.first) chunk_starts.push_back(l.t);
    CHECK(chunk_starts.size() == 2 && chunk_starts[0] == 1468 && chunk_starts[1] == 1468 + 4096);
    int closings = 0;
    for (const Launch& l : g_launches) closings += l.kind == 'n' && l.closing;
    CHECK(closings == 2);
  }
  hip_stub_set_observer(nullptr);

  // ---- messages in and out of time order, in front of the start time, short writes in between ----
  const uint64_t times[] = {pos + 5000, pos + 10, 0, pos + 3000, pos + 3000, pos + 700, pos + 100000, pos + 1};
  int64_t last = b;
  std::vector<int64_t> ids;
  for (uint64_t t : times) { const int64_t id = pg_graph_sampler_note_on(g, s1, (uint8_t)(48 + ids.size()), 0.5f, -0.25f, t); CHECK(id > last); last = id; ids.push_back(id); }
  CHECK(pg_graph_sampler_set_parameter(g, s1, PG_FOURCC('S', 'T', 'R', 'N'), 7.0f, 0, pos + 4000) == PG_OK && pg_graph_sampler_set_parameter(g, s1, PG_FOURCC('S', 'V', 'O', 'L'), 0.5f, 1, pos + 20) == PG_OK);
  CHECK(pg_graph_sampler_set_granular_parameter(g, s1, PG_FOURCC('G', 'O', 'V', 'M'), 1.0f, 1, pos + 2000) == PG_OK && pg_graph_sampler_set_granular_parameter(g, s1, PG_FOURCC('G', 'W', 'N', 'D'), 3.0f, 0, pos + 50) == PG_OK);
  write_frames(g, pos, 1);
  write_frames(g, pos, 17);
  CHECK(pg_graph_sampler_note_off(g, s1, ids[1], pos + 600) == PG_OK && pg_graph_sampler_set_note_speed(g, s1, ids[2], 1.5, 12.0f, pos + 650) == PG_OK);
  CHECK(pg_graph_sampler_set_note_volume(g, s1, ids[0], 0.0f, pos + 5001) == PG_OK && pg_graph_sampler_set_note_panning(g, s1, ids[0], 3.0f, pos + 5002) == PG_OK);
  CHECK(pg_graph_sampler_all_notes_off(g, s1, pos + 5500) == PG_OK && pg_graph_sampler_stop(g, s1, pos + 6000) == PG_OK);
  write_frames(g, pos, 1024);
  write_frames(g, pos, 333);
  write_frames(g, pos, 4096 + 7);
  CHECK(pg_graph_sampler_state(g, s1, &st) == PG_OK && st.voice_count == 64);

  // ---- removal with notes sounding; removed ids ----
  CHECK(pg_graph_sampler_note_on(g, more[0], 60, 1.0f, 0.0f, pos + 5) > 0 && pg_graph_sampler_note_on(g, more[0], 61, 1.0f, 0.0f, pos + 50000) > 0);
  write_frames(g, pos, 64);
  CHECK(pg_graph_remove_sampler(g, more[0]) == PG_OK);
  CHECK(pg_graph_remove_sampler(g, more[0]) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_granular_parameter(g, more[0], PG_FOURCC('G', 'S', 'I', 'Z'), 5.0f, 0, 0) == PG_ERR_NOT_FOUND);
  write_frames(g, pos, 64);                                    // the removal takes effect here ...
  write_frames(g, pos, 1024);
  CHECK(pg_graph_sampler_state(g, more[0], &st) == PG_ERR_NOT_FOUND && pg_graph_sampler_voice_grain_state(g, more[0], 0, gs.data()) == PG_ERR_NOT_FOUND);
  const int m4 = pg_graph_add_mixer(g);                        // a graph-changing call: the removed pool's buffer references return
  CHECK(m4 > 0 && use_count(g, buf) == 8 + 64 + 8 + 4 * 2);

  // ---- a mixer goes with its samplers ----
  CHECK(pg_graph_sampler_note_on(g, s1, 62, 1.0f, 0.0f, pos + 10) > 0);
  CHECK(pg_graph_remove_mixer(g, m1) == PG_OK);                // m2, nested in it, holds s1; m1 the file sampler and more[1..]
  CHECK(pg_graph_sampler_note_on(g, s1, 62, 1.0f, 0.0f, 0) == -PG_ERR_NOT_FOUND && pg_graph_sampler_granular_params(g, s1, &gp) == PG_ERR_NOT_FOUND);
  write_frames(g, pos, 2048);
  CHECK(pg_graph_sampler_note_on(g, s0, 64, 0.3f, 0.9f, pos + 5) > 0);
  write_frames(g, pos, 100);

  // ---- destroy with live samplers and queued events ----
  CHECK(pg_graph_sampler_note_on(g, s0, 64, 0.3f, 0.9f, pos + 999999) > 0);
  pg_graph_destroy(g);
  pg_debug_hip_calls(c1);
  if (c1[0] - c0[0] != c1[1] - c0[1]) { fprintf(stderr, "%llu allocations, %llu frees\n", (unsigned long long)(c1[0] - c0[0]), (unsigned long long)(c1[1] - c0[1])); return 1; }
  printf("ok\n");
  return 0;
}
