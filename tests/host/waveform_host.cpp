// The host side of pg_graph_sample_buffer_waveform (phonic_amd/csrc/pg_k_waveform.hip) against the stub HIP runtime (hip_stub.cpp), built with
// -fsanitize=address,undefined: mono and stereo buffers, both modes, both sources, up- and downscale, every grid (few frames per bucket, up to a
// wave per bucket, buckets split over workgroups), sub-slices, repeated calls, calls between writes while voices play the buffer, the buffer
// released while a voice holds it, destroy. The stub launches nothing: "device" memory is calloc'ed, so the points read back are zeros and only
// counts and error codes are checked; what the sanitizers watch is the new host code — the staging allocation and its release, the read-back into
// the caller's array (a buffer one point too small would be an overflow AddressSanitizer sees), the arithmetic on sizes. The library's own
// counters (pg_debug_hip_calls) must balance at the end and around every call. No audio comes out of this.
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
static pg_sample_buffer_desc desc(uint32_t ch, uint32_t rate) {
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = ch; d.rate = rate;
  return d;
}

// One call into an array of exactly the points it needs (heap: one point more written is an overflow), bracketed by the allocation counters.
static int64_t overview(pg_graph* g, int buffer, int source, int mode, uint64_t first, uint64_t n, uint32_t res, size_t rows) {
  const size_t p = (size_t)(n < res ? n : res);
  std::vector<pg_waveform_point> out(rows * p);
  uint64_t c0[4], c1[4];
  pg_debug_hip_calls(c0);
  const int64_t rc = pg_graph_sample_buffer_waveform(g, buffer, source, mode, first, n, res, out.data(), out.size());
  pg_debug_hip_calls(c1);
  if (source == PG_WAVEFORM_OF_FILE) CHECK(c1[0] - c0[0] == c1[1] - c0[1]);   // what the call allocates it frees (the granular source may make the mono buffer: it stays)
  if (rc >= 0) for (const pg_waveform_point& q : out) CHECK(q.reserved == 0);
  return rc;
}

int main() {
  uint64_t c0[4];
  pg_debug_hip_calls(c0);
  pg_graph* g = pg_graph_create(48000, 2, 1024, 0);
  CHECK(g);
  const size_t NS = 300007, NM = 70001;
  const std::vector<float> st = pcm(NS, 2), mo = pcm(NM, 1);
  pg_sample_buffer_desc ds = desc(2, 44100), dm = desc(1, 48000);
  const int bs = pg_graph_add_sample_buffer(g, st.data(), NS, &ds), bm = pg_graph_add_sample_buffer(g, mo.data(), NM, &dm);
  CHECK(bs == 0 && bm == 1);

  // argument errors: before the handle, then with it
  pg_waveform_point one[4];
  CHECK(pg_graph_sample_buffer_waveform(nullptr, bs, 0, 0, 0, 10, 4, nullptr, 4) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, 0, 10, 0, one, 4) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, 0, 0, 4, one, 4) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 2, 0, 0, 10, 4, one, 4) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 2, 0, 10, 4, one, 4) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, 0, 10, 4, one, 3) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(nullptr, bs, 0, 0, 0, 10, 4, one, 4) == -PG_ERR_PARAMETER && strstr(pg_last_error_message(), "handle is null"));
  CHECK(pg_graph_sample_buffer_waveform(g, 7, 0, 0, 0, 10, 4, one, 4) == -PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sample_buffer_waveform(g, -1, 0, 0, 0, 10, 4, one, 4) == -PG_ERR_NOT_FOUND);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, NS - 9, 10, 4, one, 4) == -PG_ERR_PARAMETER);               // one frame past the end
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, NS + 1, 1, 4, one, 4) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, UINT64_MAX, 2, 4, one, 4) == -PG_ERR_PARAMETER);            // first + n wraps around
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, 1, UINT64_MAX, 4, one, 4) == -PG_ERR_PARAMETER);
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, PG_WAVEFORM_MULTI_CHANNEL, 0, 10, 2, one, 3) == -PG_ERR_PARAMETER);   // stereo: 2 * P points
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, PG_WAVEFORM_MULTI_CHANNEL, 0, 10, 2, one, 4) == 2);
  CHECK(pg_graph_sample_buffer_waveform(g, bm, 0, PG_WAVEFORM_MULTI_CHANNEL, 0, 10, 4, one, 4) == 4);            // mono: P points suffice
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, NS - 10, 10, 4, one, 4) == 4);                               // ends at the last frame
  CHECK(pg_graph_sample_buffer_waveform(g, bs, 0, 0, NS - 1, 1, 4, one, 1) == 1);                                 // a slice of one frame

  // both buffers, both modes: upscale, the branch edge, every grid of the downscale, sub-slices with odd and even starts
  const uint32_t resolutions[] = {1, 3, 16, 100, 1024, 4096, 69999, 70001, 70002, 400000};
  for (int mode = 0; mode < 2; ++mode) {
    for (uint32_t res : resolutions) {
      const int64_t ps = (int64_t)(NS < res ? NS : res), pm = (int64_t)(NM < res ? NM : res);
      CHECK(overview(g, bs, PG_WAVEFORM_OF_FILE, mode, 0, NS, res, mode ? 2 : 1) == ps);
      CHECK(overview(g, bm, PG_WAVEFORM_OF_FILE, mode, 0, NM, res, 1) == pm);
      CHECK(overview(g, bs, PG_WAVEFORM_OF_FILE, mode, 12345, 100003, res, mode ? 2 : 1) == (int64_t)(100003 < res ? 100003 : res));
      CHECK(overview(g, bm, PG_WAVEFORM_OF_FILE, mode, 12346, 50001, res, 1) == (int64_t)(50001 < res ? 50001 : res));
    }
  }
  // the granular source: made by the first call that asks for it (stereo at another rate), the buffer itself for mono at the graph's rate
  pg_sample_buffer_info info;
  CHECK(pg_graph_sample_buffer_info(g, bs, &info) == PG_OK && info.granular_frames == -1);
  CHECK(overview(g, bs, PG_WAVEFORM_OF_GRANULAR, PG_WAVEFORM_MIXED_DOWN, 0, 1, 1024, 1) == 1);
  CHECK(pg_graph_sample_buffer_info(g, bs, &info) == PG_OK && info.granular_frames >= 1);
  const uint64_t ng = (uint64_t)info.granular_frames;
  for (int mode = 0; mode < 2; ++mode) {
    CHECK(overview(g, bs, PG_WAVEFORM_OF_GRANULAR, mode, 0, ng, 1024, 1) == (int64_t)(ng < 1024 ? ng : 1024));
    CHECK(overview(g, bm, PG_WAVEFORM_OF_GRANULAR, mode, 5, NM - 5, 16, 1) == 16);
  }
  CHECK(pg_graph_sample_buffer_waveform(g, bs, PG_WAVEFORM_OF_GRANULAR, 0, ng, 1, 4, one, 4) == -PG_ERR_PARAMETER);   // past the granular buffer's end

  // between writes, while a file voice and a granular voice play the buffer; then the host lets go and the voices keep the memory
  const int m1 = pg_graph_add_mixer(g);
  CHECK(m1 > 0);
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  const int vf = pg_graph_add_voice_from_buffer(g, m1, bs, nullptr), vg = pg_graph_add_granular_voice_from_buffer(g, 0, bs, &gp, nullptr);
  CHECK(vf >= 0 && vg >= 0);
  std::vector<float> out(2048);
  uint64_t pos = 0;
  for (int k = 0; k < 4; ++k) {
    pg_graph_write(g, out.data(), out.size(), pos);
    pos += 1024;
    CHECK(overview(g, bs, PG_WAVEFORM_OF_FILE, k & 1, 0, NS, 1024, (k & 1) ? 2 : 1) == 1024);
    CHECK(overview(g, bs, PG_WAVEFORM_OF_GRANULAR, 0, 0, ng, 16, 1) == (int64_t)(ng < 16 ? ng : 16));   // (against the stub the conversion delivers its single 0.0)
  }
  CHECK(pg_graph_sample_buffer_info(g, bs, &info) == PG_OK && info.use_count == 2);
  CHECK(pg_graph_release_sample_buffer(g, bs) == PG_OK);
  CHECK(overview(g, bs, PG_WAVEFORM_OF_FILE, 0, 0, NS, 1024, 1) == -PG_ERR_NOT_FOUND);
  CHECK(overview(g, bs, PG_WAVEFORM_OF_GRANULAR, 0, 0, 16, 4, 1) == -PG_ERR_NOT_FOUND);
  pg_graph_write(g, out.data(), out.size(), pos);
  CHECK(overview(g, bm, PG_WAVEFORM_OF_FILE, 0, 0, NM, 4096, 1) == 4096);
  pg_graph_destroy(g);   // with the voices still playing the released buffer and the mono buffer still held
  uint64_t c1[4];
  pg_debug_hip_calls(c1);
  if (c1[0] - c0[0] != c1[1] - c0[1]) { fprintf(stderr, "%llu allocations, %llu frees\n", (unsigned long long)(c1[0] - c0[0]), (unsigned long long)(c1[1] - c0[1])); return 1; }
  printf("ok\n");
  return 0;
}
