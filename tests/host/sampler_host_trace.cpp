// The host side of the samplers (pg_graph_add_sampler and the pg_graph_sampler_* messages) against the stub HIP runtime (hip_stub.cpp), built
// with -fsanitize=address,undefined: every new entry point — add, messages in and out of time order, removed and unknown ids, the main-mixer
// refusal, remove during pending events, short writes in between, a mixer removed with its sampler, destroy with a live sampler. "Device"
// memory is malloc'ed and no kernel runs, so the records read back are what the host wrote; what is checked here is the host's bookkeeping:
// ids, errors, buffer references, table growth, and that allocations and releases balance. No audio comes out of this.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/phonic_gpu.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, pg_last_error_message()); exit(1); } } while (0)

static void write_frames(pg_graph* g, uint64_t& pos, size_t frames) {
  std::vector<float> out(frames * 2);
  (void)pg_graph_write(g, out.data(), out.size(), pos);
  pos += frames;
}
static int use_count(pg_graph* g, int buffer) {
  pg_sample_buffer_info info;
  CHECK(pg_graph_sample_buffer_info(g, buffer, &info) == PG_OK);
  return info.use_count;
}

int main() {
  uint64_t c0[4], c1[4];
  pg_debug_hip_calls(c0);
  pg_graph* g = pg_graph_create(48000, 2, 1024, 0);
  CHECK(g);
  std::vector<float> pcm(2 * 3001);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (float)((i * 37) % 101) / 101.0f - 0.5f;
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = 2; d.rate = 44100; d.has_loop_range = 1; d.loop_start = 100; d.loop_end = 2900;
  const int buf = pg_graph_add_sample_buffer(g, pcm.data(), 3001, &d);
  d.has_loop_range = 0; d.channels = 1; d.rate = 48000;
  const int mono = pg_graph_add_sample_buffer(g, pcm.data(), 777, &d);
  CHECK(buf == 0 && mono == 1);
  const int m1 = pg_graph_add_mixer(g), m2 = pg_graph_add_mixer_to(g, m1), m3 = pg_graph_add_mixer(g);
  CHECK(m1 > 0 && m2 > 0 && m3 > 0 && pg_graph_add_effect(g, m1, PG_FX_GAIN, nullptr) >= 0);

  // ---- construction ----
  pg_sampler_options o;
  pg_sampler_options_default(&o);
  CHECK(pg_graph_add_sampler(g, PG_MAIN_MIXER, buf, &o) == -PG_ERR_PARAMETER && strstr(pg_last_error_message(), "sub-mixer"));
  CHECK(pg_graph_add_sampler(g, 99, buf, &o) == -PG_ERR_NOT_FOUND && pg_graph_add_sampler(g, m1, 99, &o) == -PG_ERR_NOT_FOUND);
  o.has_loop_range = 1; o.loop_start = 10; o.loop_end = 3002;
  CHECK(pg_graph_add_sampler(g, m1, buf, &o) == -PG_ERR_PARAMETER);   // the range leaves the buffer
  o.loop_end = 3001;
  CHECK(use_count(g, buf) == 0);
  const int s0 = pg_graph_add_sampler(g, m1, buf, &o);                // 8 voices, a loop range of its own
  CHECK(s0 == 0 && use_count(g, buf) == 8);
  pg_sampler_options_default(&o);
  o.voice_count = 64; o.has_envelope = 1; o.transient = 1; o.start_time = 500;
  const int s1 = pg_graph_add_sampler(g, m2, mono, &o);               // the largest pool, enveloped, in a nested mixer
  CHECK(s1 == 1 && use_count(g, mono) == 64);
  const int plain = pg_graph_add_voice_from_buffer(g, m1, buf, nullptr);
  CHECK(plain >= 0 && use_count(g, buf) == 9);
  std::vector<int> more;
  pg_sampler_options_default(&o);
  o.voice_count = 1;
  for (int i = 0; i < 6; ++i) { more.push_back(pg_graph_add_sampler(g, m3, buf, i % 2 ? nullptr : &o)); CHECK(more.back() == 2 + i); }   // the table grows past its first four records
  CHECK(use_count(g, buf) == 9 + 3 * 1 + 3 * 8);
  pg_sampler_state st;
  CHECK(pg_graph_sampler_state(g, s1, &st) == PG_OK && st.voice_count == 64 && st.active_voices == 0 && st.slots[63].envelope_stage == 0 && st.slots[0].note == 60);
  CHECK(pg_graph_sampler_state(g, s0, &st) == PG_OK && st.voice_count == 8 && st.slots[7].envelope_stage == -1 && st.slots[3].release_start_frame == UINT64_MAX && st.volume == 1.0f);
  CHECK(pg_graph_sampler_state(g, 99, &st) == PG_ERR_NOT_FOUND && pg_graph_sampler_state(g, -1, &st) == PG_ERR_NOT_FOUND);
  // the pool's voices carry no public id: the ids behind the last public one answer like removed voices
  CHECK(pg_graph_set_voice_volume(g, plain - 1, 0.5f, 0) == PG_ERR_NOT_FOUND && pg_graph_remove_voice(g, plain - 1) == PG_ERR_NOT_FOUND);

  // ---- messages: in and out of time order, short writes in between ----
  uint64_t pos = 0;
  int64_t last = 0;
  std::vector<int64_t> ids;
  const uint64_t times[] = {5000, 10, 0, 3000, 3000, 700, 100000, 1};
  for (uint64_t t : times) {
    const int64_t id = pg_graph_sampler_note_on(g, s0, (uint8_t)(48 + ids.size()), 0.5f, -0.25f, t);
    CHECK(id > last);
    last = id;
    ids.push_back(id);
  }
  CHECK(pg_graph_sampler_note_on(g, s1, 60, 1.0f, 0.0f, 900) > last);
  // s1 starts at frame 500: messages due earlier are held until then (each leaves a no-op event where it came due), sent out of time order
  CHECK(pg_graph_sampler_note_on(g, s1, 62, 1.0f, 0.0f, 300) > last && pg_graph_sampler_set_parameter(g, s1, PG_FOURCC('S', 'V', 'O', 'L'), 0.5f, 0, 100) == PG_OK);
  CHECK(pg_graph_sampler_note_off(g, s1, 12345678, 499) == PG_OK && pg_graph_sampler_note_on(g, s1, 64, 1.0f, 0.0f, 500) > last && pg_graph_sampler_all_notes_off(g, s1, 7) == PG_OK);
  CHECK(pg_graph_sampler_set_parameter(g, s0, PG_FOURCC('S', 'T', 'R', 'N'), 7.0f, 0, 4000) == PG_OK);
  CHECK(pg_graph_sampler_set_parameter(g, s0, PG_FOURCC('S', 'F', 'T', 'N'), 0.25f, 1, 2000) == PG_OK);   // sent later, due earlier
  CHECK(pg_graph_sampler_set_parameter(g, s0, PG_FOURCC('S', 'V', 'O', 'L'), 100.0f, 0, 0) == PG_OK);      // clamped
  CHECK(pg_graph_sampler_set_parameter(g, s0, PG_FOURCC('S', 'P', 'A', 'N'), 1.0f, 1, 2500) == PG_OK);
  CHECK(pg_graph_sampler_set_parameter(g, s0, PG_FOURCC('A', 'A', 'T', 'K'), 0.1f, 0, 0) == PG_ERR_PARAMETER);   // envelope parameters: out of scope
  write_frames(g, pos, 1);
  write_frames(g, pos, 17);
  CHECK(pg_graph_sampler_note_off(g, s0, ids[1], 600) == PG_OK && pg_graph_sampler_note_off(g, s0, 12345678, 601) == PG_OK && pg_graph_sampler_note_off(g, s0, -3, 602) == PG_OK);
  CHECK(pg_graph_sampler_set_note_speed(g, s0, ids[2], 1.5, 12.0f, 650) == PG_OK && pg_graph_sampler_set_note_speed(g, s0, ids[2], 0.75, -1.0f, 640) == PG_OK);
  CHECK(pg_graph_sampler_set_note_volume(g, s0, ids[0], 0.0f, 5001) == PG_OK && pg_graph_sampler_set_note_panning(g, s0, ids[0], 3.0f, 5002) == PG_OK);
  CHECK(pg_graph_sampler_all_notes_off(g, s0, 5500) == PG_OK && pg_graph_sampler_stop(g, s1, 1200) == PG_OK && pg_graph_sampler_stop(g, s0, 0) == PG_OK);
  write_frames(g, pos, 1024);
  write_frames(g, pos, 333);
  write_frames(g, pos, 4096 + 7);
  CHECK(pg_graph_sampler_state(g, s0, &st) == PG_OK && st.voice_count == 8);

  // ---- removal: during pending events; removed and unknown ids ----
  CHECK(pg_graph_sampler_note_on(g, more[0], 60, 1.0f, 0.0f, pos + 50000) > 0);
  CHECK(pg_graph_remove_sampler(g, more[0]) == PG_OK);
  CHECK(pg_graph_remove_sampler(g, more[0]) == PG_ERR_NOT_FOUND && pg_graph_sampler_note_on(g, more[0], 60, 1.0f, 0.0f, 0) == -PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_stop(g, more[0], 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_all_notes_off(g, 99, 0) == PG_ERR_NOT_FOUND && pg_graph_remove_sampler(g, -1) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_set_parameter(g, 99, PG_FOURCC('S', 'V', 'O', 'L'), 1.0f, 0, 0) == PG_ERR_NOT_FOUND && pg_graph_sampler_note_off(g, 99, 1, 0) == PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sampler_note_on(g, s0, 61, 1.0f, 0.0f, pos + 100) > 0 && pg_graph_sampler_set_parameter(g, s0, PG_FOURCC('S', 'T', 'R', 'N'), -5.0f, 0, pos + 200) == PG_OK);
  CHECK(pg_graph_remove_sampler(g, s0) == PG_OK);          // two events of it are still queued
  write_frames(g, pos, 64);                                // the removals take effect here ...
  write_frames(g, pos, 1024);                              // ... and the queued events find no sampler when they come due
  CHECK(pg_graph_sampler_state(g, s0, &st) == PG_ERR_NOT_FOUND);
  const int m4 = pg_graph_add_mixer(g);                    // a graph-changing call: the removed pools' buffer references return
  CHECK(m4 > 0 && use_count(g, buf) == 1 + 2 * 1 + 3 * 8);
  CHECK(pg_graph_release_sample_buffer(g, buf) == PG_OK && pg_graph_add_sampler(g, m3, buf, nullptr) == -PG_ERR_NOT_FOUND);   // released: the living pools keep its memory
  write_frames(g, pos, 512);

  // ---- a mixer goes with its samplers ----
  CHECK(pg_graph_sampler_note_on(g, s1, 62, 1.0f, 0.0f, pos + 10) > 0);
  CHECK(pg_graph_remove_mixer(g, m1) == PG_OK);            // m2, nested in it, holds s1
  CHECK(pg_graph_sampler_note_on(g, s1, 62, 1.0f, 0.0f, 0) == -PG_ERR_NOT_FOUND && pg_graph_sampler_state(g, s1, &st) == PG_ERR_NOT_FOUND);
  write_frames(g, pos, 2048);
  CHECK(pg_graph_sampler_note_on(g, more[1], 64, 0.3f, 0.9f, pos + 5) > 0);
  write_frames(g, pos, 100);

  // ---- destroy with live samplers and queued events ----
  CHECK(pg_graph_sampler_note_on(g, more[2], 64, 0.3f, 0.9f, pos + 999999) > 0);
  pg_graph_destroy(g);
  pg_debug_hip_calls(c1);
  if (c1[0] - c0[0] != c1[1] - c0[1]) { fprintf(stderr, "%llu allocations, %llu frees\n", (unsigned long long)(c1[0] - c0[0]), (unsigned long long)(c1[1] - c0[1])); return 1; }
  printf("ok\n");
  return 0;
}
