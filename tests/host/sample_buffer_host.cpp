// The host side of the sample buffers (pg_graph_add_sample_buffer and its family, both handles) against the stub HIP runtime (hip_stub.cpp), built
// with -fsanitize=address,undefined: the reference counts — the host's, one per voice — through release-while-playing, voice removal, mixer
// removal and destroy; "device" memory is malloc'ed, so a buffer freed too early is a use-after-free the sanitizer sees and one never freed a
// leak LeakSanitizer reports at exit. The library's own counters (pg_debug_hip_calls) must balance for every handle. No audio comes out of this.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/phonic_gpu.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, pg_last_error_message()); exit(1); } } while (0)

static std::vector<float> pcm(size_t frames, int ch) {
  std::vector<float> v(frames * ch);
  for (size_t i = 0; i < v.size(); ++i) v[i] = (float)((i * 37) % 101) / 101.0f - 0.5f;
  return v;
}
static pg_sample_buffer_desc desc(uint32_t ch, uint32_t rate, bool loop, uint64_t a = 0, uint64_t b = 0) {
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = ch; d.rate = rate; d.has_loop_range = loop ? 1 : 0; d.loop_start = a; d.loop_end = b;
  return d;
}
static void balance(const uint64_t before[4], const char* what) {
  uint64_t after[4];
  pg_debug_hip_calls(after);
  if (after[0] - before[0] != after[1] - before[1]) { fprintf(stderr, "%s: %llu allocations, %llu frees\n", what, (unsigned long long)(after[0] - before[0]), (unsigned long long)(after[1] - before[1])); exit(1); }
}

static void plain_graph(int order) {
  uint64_t c0[4];
  pg_debug_hip_calls(c0);
  pg_graph* g = pg_graph_create(48000, 2, 1024, 0);
  CHECK(g);
  const std::vector<float> st = pcm(3001, 2), mo = pcm(777, 1);
  pg_sample_buffer_desc ds = desc(2, 44100, true, 100, 2900), dm = desc(1, 48000, false);
  const int bs = pg_graph_add_sample_buffer(g, st.data(), 3001, &ds), bm = pg_graph_add_sample_buffer(g, mo.data(), 777, &dm);
  CHECK(bs == 0 && bm == 1);
  pg_sample_buffer_desc bad = desc(2, 44100, true, 3001, 3001);
  CHECK(pg_graph_add_sample_buffer(g, st.data(), 3001, &bad) == -PG_ERR_PARAMETER);
  const int m1 = pg_graph_add_mixer(g), m2 = pg_graph_add_mixer(g);
  CHECK(m1 > 0 && m2 > 0 && pg_graph_add_effect(g, m1, 0, nullptr) >= 0);
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  std::vector<int> voices;
  for (int i = 0; i < 6; ++i) {
    pg_voice_options o;
    pg_voice_options_default(&o);
    o.speed = i % 2 ? 1.7 : 0.5; o.start_time = 100 * i; o.source_rate = i == 3 ? 32000 : 0;
    voices.push_back(pg_graph_add_voice_from_buffer(g, i < 3 ? m1 : (i < 5 ? m2 : 0), i == 4 ? bm : bs, &o));
    CHECK(voices.back() >= 0);
  }
  voices.push_back(pg_graph_add_granular_voice_from_buffer(g, m2, bs, &gp, nullptr));
  voices.push_back(pg_graph_add_granular_voice_from_buffer(g, 0, bm, &gp, nullptr));
  voices.push_back(pg_graph_add_granular_voice_from_buffer(g, m1, bs, &gp, nullptr));
  CHECK(voices[6] >= 0 && voices[7] >= 0 && voices[8] >= 0);
  pg_sample_buffer_info info;
  CHECK(pg_graph_sample_buffer_info(g, bs, &info) == PG_OK && info.use_count == 7 && info.granular_frames >= 1 && info.has_loop_range == 1 && info.loop_end == 2900);
  CHECK(pg_graph_sample_buffer_info(g, bm, &info) == PG_OK && info.use_count == 2 && info.granular_frames == 777);   // a mono buffer at the graph's rate: itself
  CHECK(pg_graph_prepare_granular_buffer(g, bs) == PG_OK && pg_graph_prepare_granular_buffer(g, bm) == PG_OK);
  std::vector<float> mono(1024), out(2048);
  CHECK(pg_graph_read_granular_buffer(g, bm, mono.data(), mono.size()) == 777 && memcmp(mono.data(), mo.data(), 777 * sizeof(float)) == 0);
  uint64_t pos = 0;
  auto write = [&]() { pg_graph_write(g, out.data(), out.size(), pos); pos += 1024; };
  write();
  if (order == 0) {   // the host lets go first: the voices keep the memory
    CHECK(pg_graph_release_sample_buffer(g, bs) == PG_OK && pg_graph_release_sample_buffer(g, bs) == PG_ERR_NOT_FOUND);
    CHECK(pg_graph_add_voice_from_buffer(g, m1, bs, nullptr) == -PG_ERR_NOT_FOUND && pg_graph_sample_buffer_info(g, bs, &info) == PG_ERR_NOT_FOUND);
    CHECK(pg_graph_read_granular_buffer(g, bs, mono.data(), 4) == -PG_ERR_NOT_FOUND);
    write();
  }
  CHECK(pg_graph_remove_voice(g, voices[0]) == PG_OK && pg_graph_remove_voice(g, voices[6]) == PG_OK);
  write();
  CHECK(pg_graph_remove_mixer(g, m2) == PG_OK);   // takes voices 3, 4 and the granular voice 6 (gone already) with it
  write();
  CHECK(pg_graph_add_mixer(g) > 0);               // a graph-changing call: the retired voices let go of their references
  if (order == 1) {   // the voices go first, then the host
    for (int v : {1, 2, 5, 7, 8}) CHECK(pg_graph_remove_voice(g, voices[v]) == PG_OK);
    write();
    CHECK(pg_graph_add_mixer(g) > 0);
    CHECK(pg_graph_sample_buffer_info(g, bs, &info) == PG_OK && info.use_count == 0);
    CHECK(pg_graph_release_sample_buffer(g, bs) == PG_OK && pg_graph_release_sample_buffer(g, bm) == PG_OK);
  }
  write();
  pg_graph_destroy(g);   // order 0: with voices still playing a released buffer and a held one
  balance(c0, "plain graph");
}

static void sharded_graph() {
  uint64_t c0[4];
  pg_debug_hip_calls(c0);
  const int devices[2] = {0, 1};
  pg_sharded_graph* s = pg_sharded_create(48000, 2, 1024, devices, 2);
  CHECK(s);
  const std::vector<float> st = pcm(2001, 2);
  pg_sample_buffer_desc ds = desc(2, 44100, true, 10, 1500);
  pg_sample_buffer_desc d2 = desc(2, 96000, false);
  const int b = pg_sharded_add_sample_buffer(s, st.data(), 2001, &ds), b2 = pg_sharded_add_sample_buffer(s, st.data(), 500, &d2);
  CHECK(b == 0 && b2 == 1);
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  std::vector<int> voices;
  for (int i = 0; i < 4; ++i) {
    const int m = pg_sharded_add_mixer(s);
    CHECK(m > 0);
    voices.push_back(pg_sharded_add_voice_from_buffer(s, m, b, nullptr));
    voices.push_back(pg_sharded_add_granular_voice_from_buffer(s, m, b, &gp, nullptr));
    CHECK(voices[2 * i] >= 0 && voices[2 * i + 1] >= 0);
  }
  pg_sample_buffer_info info;
  CHECK(pg_sharded_sample_buffer_info(s, b, &info) == PG_OK && info.use_count == 8 && info.n_frames == 2001);
  CHECK(pg_sharded_prepare_granular_buffer(s, b2) == PG_OK);   // reached no shard yet: made on the root
  std::vector<float> mono(64), out(2048);
  CHECK(pg_sharded_read_granular_buffer(s, b, 0, mono.data(), mono.size()) >= 1 && pg_sharded_read_granular_buffer(s, b, 1, mono.data(), mono.size()) >= 1);
  CHECK(pg_sharded_read_granular_buffer(s, b, 2, mono.data(), mono.size()) == -PG_ERR_PARAMETER);
  pg_sharded_write(s, out.data(), out.size(), 0);
  CHECK(pg_sharded_release_sample_buffer(s, b) == PG_OK && pg_sharded_release_sample_buffer(s, b) == PG_ERR_NOT_FOUND);
  CHECK(pg_sharded_add_voice_from_buffer(s, 1, b, nullptr) == -PG_ERR_NOT_FOUND);
  for (int i = 0; i < 8; i += 3) CHECK(pg_sharded_remove_voice(s, voices[i]) == PG_OK);
  pg_sharded_write(s, out.data(), out.size(), 1024);
  CHECK(pg_sharded_add_mixer(s) > 0);
  pg_sharded_write(s, out.data(), out.size(), 2048);
  pg_sharded_destroy(s);   // b2 is still held, some voices of b still play
  balance(c0, "sharded graph");
}

int main() {
  plain_graph(0);
  plain_graph(1);
  sharded_graph();
  printf("ok\n");
  return 0;
}
