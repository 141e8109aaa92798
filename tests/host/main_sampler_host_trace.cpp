// The host side of samplers on the MAIN mixer (pg_graph_add_sampler_to_main, pg_graph_add_granular_sampler_to_main, pg_graph_sampler_set_volume,
// _set_panning, pg_graph_sampler_output_state) against the stub HIP runtime (hip_stub.cpp), built with -fsanitize=address,undefined: both add
// calls and every refusal in its stated order, messages out of time order and in front of the start time, a source added in front of and behind
// the pool, remove and destroy with events queued, the transient drop — allocations and releases must balance. From the records the stub's
// observer sees it checks what the device is told: ONE source unit with the whole pool at the run's place in the order, the sampler's commands
// addressed to that unit at frame 0 of a launch, and the main mixer's chunk grid begun again at every message's frame.
// "Device" memory is malloc'ed and no kernel runs, so nothing the device decides is checked here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "hip_stub_observer.h"
#include "../../phonic_amd/csrc/pg_host_internal.h"   // pg_graph, PgLaunch, PgCmd, PgSamplerRec: what the observer and the checks read

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, pg_last_error_message()); exit(1); } } while (0)
#define MSG(text) (strstr(pg_last_error_message(), text) != nullptr)

struct SeenCmd { uint64_t pos; PgCmd c; };
static std::vector<SeenCmd> g_cmds;          // sampler commands as a unit-kernel launch carries them
static std::set<uint64_t> g_chunk_starts;    // positions of launches that begin a chunk of the main mixer
static int observe(const StubCall* c) {
  if (c->kind != STUB_LAUNCH || !c->name || !strstr(c->name, "pg_unit_kernel")) return 0;
  PgLaunch L;
  memcpy((void*)&L, c->args[0], sizeof L);
  if (!L.voices) return 0;
  if (L.grid_off == 0) g_chunk_starts.insert(L.pos);
  if (L.mode == 1 || !L.cmds) return 0;   // (the generic kernel's launches carry the list the exact path applies)
  for (int i = 0; i < L.n_cmds; ++i)
    if (pg_cmd_is_sampler_message(L.cmds[i].type) || pg_cmd_is_sampler_output(L.cmds[i].type)) {
      bool dup = false;
      for (const SeenCmd& s : g_cmds) dup |= s.pos == L.pos && memcmp(&s.c, &L.cmds[i], sizeof(PgCmd)) == 0;
      if (!dup) g_cmds.push_back({L.pos, L.cmds[i]});
    }
  return 0;
}
static void write_frames(pg_graph* g, uint64_t& pos, size_t frames) {
  std::vector<float> out(frames * 2);
  (void)pg_graph_write(g, out.data(), out.size(), pos);
  pos += frames;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static const PgSamplerRec& rec_of(const pg_graph* g, int id) { return ((const PgSamplerRec*)(g->d_samp + 1))[id]; }
// The unit that holds sampler `id`'s pool as the last topology describes it, and its place among the main mixer's sources in g->order
static int unit_place(const pg_graph* g, int unit) {
  for (size_t i = 0; i < g->order.size(); ++i) if (g->order[i] == unit) return (int)i;
  return -1;
}

int main() {
  uint64_t c0[4], c1[4];
  pg_debug_hip_calls(c0);

  // ---- defaults and refusals without a graph, in the stated order: sampler options, granular options, generator options, handle ----
  pg_generator_options gen;
  gen.volume = -7.0f; gen.panning = 9.0f;
  pg_generator_options_default(&gen);
  CHECK(gen.volume == 1.0f && gen.panning == 0.0f && pg_generator_options_check(&gen) == PG_OK);
  pg_generator_options_default(nullptr);
  CHECK(pg_generator_options_check(nullptr) == PG_ERR_PARAMETER);
  pg_generator_options bad = gen;
  bad.volume = -0.5f;
  CHECK(pg_generator_options_check(&bad) == PG_ERR_PARAMETER && MSG("playback options 'volume' value is '-0.5'"));
  bad.volume = NAN;
  CHECK(pg_generator_options_check(&bad) == PG_ERR_PARAMETER && MSG("playback options 'volume' value is"));
  bad = gen; bad.panning = 1.5f;
  CHECK(pg_generator_options_check(&bad) == PG_ERR_PARAMETER && MSG("playback options 'panning' value is '1.5'"));
  bad.panning = NAN;
  CHECK(pg_generator_options_check(&bad) == PG_ERR_PARAMETER && MSG("playback options 'panning' value is"));
  bad.panning = -1.0f; bad.volume = 0.0f;
  CHECK(pg_generator_options_check(&bad) == PG_OK);
  pg_sampler_options o;
  pg_sampler_options_default(&o);
  pg_granular_sampler_options go;
  pg_granular_sampler_options_default(&go);
  bad = gen; bad.volume = -1.0f;
  pg_sampler_options obad = o;
  obad.voice_count = 0;
  pg_granular_sampler_options gbad = go;
  gbad.params.size = 0.0f;
  CHECK(pg_graph_add_sampler_to_main(nullptr, 0, &obad, &bad) == -PG_ERR_PARAMETER && MSG("Invalid voice count"));
  CHECK(pg_graph_add_sampler_to_main(nullptr, 0, &o, &bad) == -PG_ERR_PARAMETER && MSG("playback options 'volume'"));
  CHECK(pg_graph_add_sampler_to_main(nullptr, 0, &o, nullptr) == -PG_ERR_PARAMETER && MSG("graph handle is null"));
  CHECK(pg_graph_add_granular_sampler_to_main(nullptr, 0, &obad, &gbad, &bad) == -PG_ERR_PARAMETER && MSG("Invalid voice count"));
  CHECK(pg_graph_add_granular_sampler_to_main(nullptr, 0, &o, &gbad, &bad) == -PG_ERR_PARAMETER && MSG("Grain size"));
  CHECK(pg_graph_add_granular_sampler_to_main(nullptr, 0, &o, nullptr, &bad) == -PG_ERR_PARAMETER && MSG("granular sampler options must not be null"));
  CHECK(pg_graph_add_granular_sampler_to_main(nullptr, 0, &o, &go, &bad) == -PG_ERR_PARAMETER && MSG("playback options 'volume'"));
  CHECK(pg_graph_add_granular_sampler_to_main(nullptr, 0, &o, &go, &gen) == -PG_ERR_PARAMETER && MSG("graph handle is null"));
  CHECK(pg_graph_sampler_set_volume(nullptr, 0, -1.0f, 0) == PG_ERR_PARAMETER && MSG("Invalid volume"));
  CHECK(pg_graph_sampler_set_volume(nullptr, 0, INFINITY, 0) == PG_ERR_PARAMETER && pg_graph_sampler_set_volume(nullptr, 0, NAN, 0) == PG_ERR_PARAMETER);
  CHECK(pg_graph_sampler_set_panning(nullptr, 0, NAN, 0) == PG_ERR_PARAMETER && MSG("Invalid panning") && pg_graph_sampler_set_panning(nullptr, 0, INFINITY, 0) == PG_ERR_PARAMETER);
  CHECK(pg_graph_sampler_set_volume(nullptr, 0, 1.0f, 0) == PG_ERR_PARAMETER && MSG("graph handle is null"));
  CHECK(pg_graph_sampler_set_panning(nullptr, 0, 5.0f, 0) == PG_ERR_PARAMETER && MSG("graph handle is null"));   // (finite: clamped by the pan law, as a note's)
  pg_sampler_output_state os;
  CHECK(pg_graph_sampler_output_state(nullptr, 0, &os) == PG_ERR_PARAMETER && pg_graph_sampler_output_state(nullptr, 0, nullptr) == PG_ERR_PARAMETER);

  hip_stub_set_observer(observe);
  pg_graph* g = pg_graph_create(48000, 2, 256, 0);
  CHECK(g);
  std::vector<float> pcm(3001);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (float)((i * 37) % 101) / 101.0f - 0.5f;
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = 1; d.rate = 48000;
  const int buf = pg_graph_add_sample_buffer(g, pcm.data(), 3001, &d);
  CHECK(buf == 0);
  const int m1 = pg_graph_add_mixer(g);
  CHECK(m1 > 0);

  // ---- refusals that need a graph: the buffer, the loop range; the old entry points keep refusing the main mixer ----
  CHECK(pg_graph_add_sampler_to_main(g, 7, &o, &gen) == -PG_ERR_NOT_FOUND && pg_graph_add_granular_sampler_to_main(g, 7, &o, &go, &gen) == -PG_ERR_NOT_FOUND);
  obad = o; obad.has_loop_range = 1; obad.loop_start = 10; obad.loop_end = 4000;
  CHECK(pg_graph_add_sampler_to_main(g, buf, &obad, &gen) == -PG_ERR_PARAMETER && MSG("Invalid loop range"));
  CHECK(pg_graph_add_sampler(g, PG_MAIN_MIXER, buf, &o) == -PG_ERR_PARAMETER && MSG("A sampler needs a sub-mixer"));
  CHECK(pg_graph_add_granular_sampler(g, PG_MAIN_MIXER, buf, &o, &go) == -PG_ERR_PARAMETER && MSG("A sampler needs a sub-mixer"));
  CHECK(g->samplers.empty() && g->h_units.size() == 2);   // (nothing was built for a refused call: the bus and the sub-mixer)

  // ---- a plain voice, the file pool, a second plain voice with the same start time, a granular pool, a sub-mixer's sampler ----
  pg_voice_options vo;
  pg_voice_options_default(&vo);
  const int va = pg_graph_add_voice(g, PG_MAIN_MIXER, pcm.data(), 3001, 1, 48000, &vo);
  o.voice_count = 5; o.has_envelope = 1;
  gen.volume = 0.5f; gen.panning = -0.25f;
  const int f_main = pg_graph_add_sampler_to_main(g, buf, &o, &gen);
  const int vb = pg_graph_add_voice(g, PG_MAIN_MIXER, pcm.data(), 3001, 1, 48000, &vo);
  o.voice_count = 3; o.has_envelope = 0; o.transient = 1; o.start_time = 1000;
  const int g_main = pg_graph_add_granular_sampler_to_main(g, buf, &o, &go, nullptr);   // null: the defaults
  pg_sampler_options_default(&o);
  o.voice_count = 2;
  const int f_sub = pg_graph_add_sampler(g, m1, buf, &o);
  CHECK(va >= 0 && vb >= 0 && f_main == 0 && g_main == 1 && f_sub == 2);
  const int u_f = g->samplers[f_main].unit, u_g = g->samplers[g_main].unit;
  CHECK(u_f > 0 && u_g > 0 && u_f != u_g && g->samplers[f_sub].unit == -1);
  CHECK(rec_of(g, f_main).unit == u_f && rec_of(g, f_main).n_voices == 5 && rec_of(g, f_main).out.on == 1);
  CHECK(rec_of(g, f_main).out.volume.current == 0.5f && rec_of(g, f_main).out.volume.target == 0.5f && rec_of(g, f_main).out.panning.target == -0.25f);
  CHECK(rec_of(g, g_main).n_voices == 0 && rec_of(g, g_main).unit == -1 && rec_of(g, g_main).out.on == 1 && rec_of(g, g_main).out.volume.target == 1.0f && rec_of(g, g_main).out.panning.target == 0.0f);
  CHECK(g->d_gsamp[g_main].note.unit == u_g && g->d_gsamp[g_main].note.n_voices == 3);
  CHECK(rec_of(g, f_sub).out.on == 0 && rec_of(g, f_sub).unit == g->mixers[m1].unit_slot);
  CHECK(g->d_samp->gsamp == g->d_gsamp);
  // the sub-mixer's sampler has no output stage
  CHECK(pg_graph_sampler_set_volume(g, f_sub, 0.5f, 0) == PG_ERR_STATE && MSG("lives in a sub-mixer"));
  CHECK(pg_graph_sampler_set_panning(g, f_sub, 0.5f, 0) == PG_ERR_STATE && MSG("no sum of the sampler exists"));
  CHECK(pg_graph_sampler_output_state(g, f_sub, &os) == PG_ERR_STATE && MSG("lives in a sub-mixer"));
  CHECK(pg_graph_sampler_set_volume(g, 99, 0.5f, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_panning(g, -1, 0.5f, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_output_state(g, 99, &os) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_set_volume(g, 99, -0.5f, 0) == PG_ERR_PARAMETER);   // the argument check comes first
  CHECK(pg_graph_sampler_output_state(g, f_main, &os) == PG_OK && os.volume_current == 0.5f && os.volume_target == 0.5f && os.panning_current == -0.25f && os.volume_ramping == 0 && os.panning_ramping == 0);

  // ---- the topology: one source unit per pool, at the run's place ----
  uint64_t pos = 0;
  write_frames(g, pos, 64);
  {
    const PgUnit& uf = g->h_units[u_f];
    const PgUnit& ug = g->h_units[u_g];
    CHECK(uf.kind == UNIT_SOURCE && uf.n_voices == 5 && uf.n_fx == 0 && uf.static_defer == 1 && uf.sampler == f_main + 1);
    CHECK(ug.kind == UNIT_SOURCE && ug.n_voices == 3 && ug.static_defer == 1 && ug.sampler == g_main + 1);
    // the main mixer's list: vb (added last with start time 0) in front of the file pool, the pool in slot order, va behind it, the late granular pool last
    const std::vector<int>& mv = g->mixers[0].voices;
    CHECK(mv.size() == 2 + 5 + 3 && mv[0] == vb && mv[6] == va);
    for (int k = 0; k < 5; ++k) CHECK(mv[1 + k] == g->samplers[f_main].voice_id_slot0 - k && g->source_unit_of_voice[mv[1 + k]] == u_f);
    for (int k = 0; k < 3; ++k) CHECK(mv[7 + k] == g->samplers[g_main].voice_id_slot0 - k && g->source_unit_of_voice[mv[7 + k]] == u_g);
    const int p_b = unit_place(g, g->source_unit_of_voice[vb]), p_f = unit_place(g, u_f), p_a = unit_place(g, g->source_unit_of_voice[va]), p_g = unit_place(g, u_g);
    CHECK(p_b >= 0 && p_f == p_b + 1 && p_a == p_f + 1 && p_g == p_a + 1 && p_g == (int)g->order.size() - 1);
    CHECK(uf.voice0 == rec_of(g, f_main).voice0 && ug.voice0 == g->d_gsamp[g_main].note.voice0);
    CHECK(g->n_main_samplers == 2 && g->n_static_defer >= 3);
  }

  // ---- messages out of time order: each begins a chunk of the main mixer and reaches the sampler's own unit at frame 0 ----
  g_cmds.clear(); g_chunk_starts.clear();
  CHECK(pg_graph_sampler_set_volume(g, f_main, 0.25f, pos + 300) == PG_OK);
  CHECK(pg_graph_sampler_note_on(g, f_main, 60, 1.0f, 0.0f, pos + 100) > 0);
  CHECK(pg_graph_sampler_set_panning(g, f_main, 0.75f, pos + 200) == PG_OK);
  CHECK(pg_graph_sampler_set_volume(g, f_main, 0.125f, pos + 300) == PG_OK);   // the same frame: the last one sent counts
  CHECK(pg_graph_sampler_set_envelope_parameter(g, f_main, PG_FOURCC('A', 'S', 'T', 'N'), 0.5f, 0, pos + 250) == PG_OK);
  const uint64_t t0 = pos;
  write_frames(g, pos, 1000);
  {
    std::vector<SeenCmd> real;
    for (const SeenCmd& s : g_cmds) if (s.c.type != CMD_NOP) real.push_back(s);
    CHECK(real.size() == 4);   // (of the two volumes of frame 300 the earlier one became a no-op: the wrapper's queue holds one message)
    const int types[4] = {CMD_SAMPLER_NOTE_ON, CMD_SAMPLER_OUT_PAN, CMD_SAMPLER_ENV_PARAM, CMD_SAMPLER_OUT_VOLUME};
    const uint64_t at[4] = {t0 + 100, t0 + 200, t0 + 250, t0 + 300};
    for (int i = 0; i < 4; ++i) CHECK(real[i].pos == at[i] && real[i].c.unit == u_f && real[i].c.frame == 0 && real[i].c.target == f_main && real[i].c.type == types[i]);
    CHECK(bits(real[3].c.value) == bits(0.125f));
    CHECK(bits(real[1].c.value) == bits(0.75f));
    for (uint64_t t : {t0, t0 + 100, t0 + 200, t0 + 250, t0 + 300}) CHECK(g_chunk_starts.count(t) == 1);
    CHECK(g_chunk_starts.count(t0 + 256) == 0 && g_chunk_starts.size() == 5);   // (nothing else begins a chunk: the last one runs 700 frames)
  }

  // ---- in front of the start time: a no-op cut where the message was stamped, the command at the start time ----
  g_cmds.clear(); g_chunk_starts.clear();
  pg_graph* g2 = pg_graph_create(48000, 2, 256, 0);
  CHECK(g2);
  {
    const int b2 = pg_graph_add_sample_buffer(g2, pcm.data(), 3001, &d);
    pg_sampler_options o2;
    pg_sampler_options_default(&o2);
    o2.voice_count = 2; o2.start_time = 700;
    const int s2 = pg_graph_add_granular_sampler_to_main(g2, b2, &o2, &go, &gen);
    CHECK(b2 == 0 && s2 == 0);
    CHECK(pg_graph_sampler_set_panning(g2, s2, 0.5f, 350) == PG_OK && pg_graph_sampler_note_on(g2, s2, 64, 1.0f, 0.0f, 200) > 0);
    uint64_t p2 = 0;
    write_frames(g2, p2, 1500);
    std::vector<SeenCmd> real;
    for (const SeenCmd& s : g_cmds) if (s.c.type != CMD_NOP) real.push_back(s);
    CHECK(real.size() == 2 && real[0].pos == 700 && real[0].c.type == CMD_SAMPLER_NOTE_ON && real[1].pos == 700 && real[1].c.type == CMD_SAMPLER_OUT_PAN);
    CHECK(real[0].c.unit == g2->samplers[s2].unit && real[1].c.unit == g2->samplers[s2].unit);
    for (uint64_t t : {(uint64_t)0, (uint64_t)200, (uint64_t)350, (uint64_t)700}) CHECK(g_chunk_starts.count(t) == 1);
    // events queued at destroy
    CHECK(pg_graph_sampler_set_volume(g2, s2, 0.5f, p2 + 999999) == PG_OK && pg_graph_sampler_set_panning(g2, s2, 0.5f, p2 + 5) == PG_OK);
    write_frames(g2, p2, 1);
    CHECK(pg_graph_sampler_set_volume(g2, s2, 0.75f, p2 + 10) == PG_OK);   // still in the ring at destroy
  }
  pg_graph_destroy(g2);

  // ---- the transient drop: the mixer lets go of a stopped transient sampler at the top of the next write; its read-backs stay ----
  g_cmds.clear();
  CHECK(pg_graph_sampler_set_volume(g, g_main, 0.5f, pos + 40) == PG_OK && pg_graph_sampler_set_volume(g, g_main, 0.25f, pos + 5000) == PG_OK);
  write_frames(g, pos, 64);
  g->samp_stopped[(size_t)g_main] = 1;   // (what pg_gsampler_kernel writes when the stopping sampler has no active slot left)
  write_frames(g, pos, 64);
  CHECK(!g->samplers[g_main].alive && g->n_main_samplers == 1 && unit_place(g, u_g) < 0 && g->mixers[0].voices.size() == 2 + 5);
  for (const Event& e : g->mixers[0].events) CHECK(!pg_cmd_is_sampler_output(e.cmd.type) || e.cmd.target != g_main);   // its queued event became a no-op
  CHECK(pg_graph_sampler_set_volume(g, g_main, 0.5f, 0) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_output_state(g, g_main, &os) == PG_OK && os.volume_target == 1.0f);   // (no kernel runs here: the record is as it was built)
  pg_sampler_state st;
  CHECK(pg_graph_sampler_state(g, g_main, &st) == PG_OK && st.voice_count == 3);

  // ---- remove with events queued: they become no-ops, the unit leaves the order, later calls find nothing ----
  CHECK(pg_graph_sampler_set_panning(g, f_main, -0.5f, pos + 100) == PG_OK && pg_graph_sampler_set_volume(g, f_main, 0.5f, pos + 50000) == PG_OK);
  write_frames(g, pos, 32);
  CHECK(pg_graph_remove_sampler(g, f_main) == PG_OK);
  CHECK(pg_graph_sampler_set_volume(g, f_main, 0.5f, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_set_panning(g, f_main, 0.5f, 0) == PG_ERR_NOT_FOUND);
  g_cmds.clear();
  write_frames(g, pos, 256);
  for (const SeenCmd& s : g_cmds) CHECK(s.c.type == CMD_NOP || s.c.target != f_main);
  CHECK(unit_place(g, u_f) < 0 && g->n_main_samplers == 0 && g->mixers[0].voices.size() == 2);
  CHECK(pg_graph_sampler_output_state(g, f_main, &os) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_stop_all_voices(g) == PG_OK);
  write_frames(g, pos, 64);
  hip_stub_set_observer(nullptr);
  pg_graph_destroy(g);
  pg_debug_hip_calls(c1);
  if (c1[0] - c0[0] != c1[1] - c0[1]) { fprintf(stderr, "%llu allocations, %llu frees\n", (unsigned long long)(c1[0] - c0[0]), (unsigned long long)(c1[1] - c0[1])); return 1; }
  printf("ok\n");
  return 0;
}
