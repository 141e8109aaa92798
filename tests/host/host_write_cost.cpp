// Host cost per pg_graph_write_device call against the stub HIP runtime, no observer installed (tools/host_write_cost.py): a graph of 64 Gain -> Reverb
// sub-mixers, 1024-frame calls on a caller's stream; prints microseconds per call: steady at max_blocks 1 and 32, then with one voice command per call
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/phonic_gpu.h"

static double run(int max_blocks, bool with_command, int calls) {
  pg_graph* g = pg_graph_create(48000, 2, 1024, 0);
  pg_graph_set_max_blocks_per_launch(g, max_blocks);
  std::vector<float> pcm(4096, 0.1f);
  std::vector<int> voices;
  for (int i = 0; i < 64; ++i) {
    const int m = pg_graph_add_mixer(g);
    pg_graph_add_effect(g, m, PG_FX_GAIN, nullptr);
    pg_graph_add_effect(g, m, PG_FX_REVERB, nullptr);
    voices.push_back(pg_graph_add_voice(g, m, pcm.data(), pcm.size(), 1, 48000, nullptr));
  }
  float* out = (float*)malloc(2 * 1024 * sizeof(float));
  void* stream = (void*)out;   // (a caller's stream: any non-null token for the stub)
  uint64_t pos = 0;
  for (int i = 0; i < 200; ++i) { pg_graph_write_device(g, out, 2048, pos, stream); pos += 1024; }
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < calls; ++i) {
    if (with_command) pg_graph_set_voice_volume(g, voices[(size_t)i % voices.size()], 0.5f, pos + 10);
    if (pg_graph_write_device(g, out, 2048, pos, stream) != 2048) { fprintf(stderr, "write failed: %s\n", pg_last_error_message()); exit(1); }
    pos += 1024;
  }
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / calls;
  pg_graph_destroy(g);
  free(out);
  return us;
}
int main() {
  printf("%.3f %.3f %.3f %.3f\n", run(1, false, 1000000), run(32, false, 1000000), run(1, true, 1000000), run(32, true, 1000000));
  return 0;
}
