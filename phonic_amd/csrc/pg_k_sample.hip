// The granular mono buffer of a sample buffer, made on the device: Sampler::create_granular_sample_buffer (src/generator/sampler.rs:908-952)
// pulls a temporary PreloadedFileSource — the graph's rate, default options, repeat(0), the cubic resampler — in writes of exactly 1024 frames
// until a write returns 0, and pushes per frame the f32 sum of the channels divided by their count. The result here is that sequence bit for
// bit (the sign of an all-zero frame's sum aside: it depends on the identity of the Rust release's f32 `Sum`).
//
// The only serial quantity is the resampler's f32 `sub_pos` schedule (src/utils/resampler/cubic.rs:72-111): which input frames have been
// pushed when an output frame is interpolated, and at which fraction. It is the same for every channel and does not depend on the samples:
//   pass A  pg_sample_sched_kernel, one workgroup: walks the schedule in pieces of 1024 output frames = the temporary source's writes. A piece
//           with ratio in [0.5, 1) whose input cannot run out takes the exact time-parallel scan of the file voices (sched_parallel,
//           pg_source_dev.h); every other piece is the reference's loop on one lane. Per output frame it leaves the count of pushed frames
//           and the fraction in a scratch table, and at the end the number of frames the source delivers.
//   pass B  pg_sample_interp_kernel, one lane per output frame over the whole chip: the Hermite window is the last four frames pushed (zeros
//           in front of the buffer: CubicInterpolator::new), evaluated per channel with cubic_interp — the file voices' form of
//           cubic.rs:125-142, no contraction — then the down-mix.
// Where the source ends: a write in which the input runs dry is the source's last one (PreloadedFileSource::write, preloaded.rs:396-475: the
// end of file makes it exhausted); the outputs the interpolator can still deliver without a new input frame appear only as far as that
// write has room (write_buffer asks again with an empty input slice, preloaded.rs:287-330). So the walk ends at the first output that needs
// a frame behind the buffer's last one, or at the end of the 1024-frame piece whose last output consumed that last frame, whichever comes first.
#include "pg_host_internal.h"
#include "pg_source_dev.h"

constexpr int PG_SAMPLE_PIECE = 1024;   // frames per write of create_granular_sample_buffer's loop (sampler.rs:932)

struct PgSampleConv {
  const float* pcm;            // interleaved, n_frames * channels
  uint64_t n_frames;
  uint32_t channels;           // 1 or 2
  float ratio;                 // CubicResampler's: (file rate / graph rate as f64) as f32 (cubic.rs:164)
  uint32_t* cnt;               // scratch, cap_out entries: input frames pushed when output k is interpolated
  float* frac;                 // ... and its fraction
  uint64_t cap_out;            // a multiple of PG_SAMPLE_PIECE
  unsigned long long* result;  // [0] frames the source delivers, [1] != 0: the scratch table was too small (a bug of the host's bound)
  float* out;                  // pass B: n_out mono frames
  uint64_t n_out;
};

__global__ void __launch_bounds__(256) pg_sample_sched_kernel(PgSampleConv L) {
  __shared__ uint16_t oc16[PG_SAMPLE_PIECE];
  __shared__ uint32_t oc32[PG_SAMPLE_PIECE];
  __shared__ float of[PG_SAMPLE_PIECE];
  __shared__ int scr[32];
  __shared__ unsigned long long s_cons;
  __shared__ float s_sp;
  __shared__ int s_n, s_ended;
  const int tid = pg_tid();
  const float ratio = L.ratio;
  const uint64_t N = L.n_frames;
  // every lane carries the walk's state (the same values): frames pushed, frames produced, sub_pos
  uint64_t cons = N >= 3 ? 3 : 0;   // the first process call pushes three frames when it is offered that many (cubic.rs:61-69), never later:
  uint64_t produced = 0;            // what a later call is offered is what the first one left
  float sp = 0.0f;
  int overflow = 0;
  for (;;) {
    if (produced + PG_SAMPLE_PIECE > L.cap_out) { overflow = 1; break; }
    const float t = sp * 16777216.0f;
    const bool par = ratio >= 0.5f && ratio < 1.0f && N - cons > (uint64_t)PG_SAMPLE_PIECE && sp >= 0.0f && sp < 2.0f && t == floorf(t);
    bool walked = false;
    int n = 0, ended = 0;
    if (par) {   // at most one push per output: the input cannot run out inside the piece
      int c = 0;
      float sp_out = 0.0f;
      if (sched_parallel(ratio, sp, PG_SAMPLE_PIECE, oc16, of, scr, c, sp_out)) {
        for (int k = tid; k < PG_SAMPLE_PIECE; k += 256) { L.cnt[produced + k] = (uint32_t)(cons + oc16[k]); L.frac[produced + k] = of[k]; }
        cons += (uint64_t)c; sp = sp_out; n = PG_SAMPLE_PIECE;
        walked = true;
      }
    }
    if (!walked) {
      __syncthreads();
      if (tid == 0) {   // CubicInterpolator::process, one call with room for the rest of the write (cubic.rs:72-111)
        uint64_t cc = cons;
        float s = sp;
        int k = 0, end = 0;
        if (ratio < 1.0f) {
          while (k < PG_SAMPLE_PIECE) {
            if (s >= 1.0f) {
              if (cc >= N) { end = 1; break; }
              cc += 1; s -= 1.0f;
            }
            oc32[k] = (uint32_t)cc; of[k] = s; ++k;
            s += ratio;
          }
        } else {
          while (k < PG_SAMPLE_PIECE) {
            while (s < ratio) {
              if (cc >= N) { end = 1; break; }
              cc += 1; s += 1.0f;
            }
            if (end) break;
            s -= ratio;
            oc32[k] = (uint32_t)cc; of[k] = 1.0f - s; ++k;
          }
        }
        s_cons = cc; s_sp = s; s_n = k; s_ended = end;
      }
      __syncthreads();
      n = s_n; ended = s_ended; cons = s_cons; sp = s_sp;
      for (int k = tid; k < n; k += 256) { L.cnt[produced + k] = oc32[k]; L.frac[produced + k] = of[k]; }
    }
    __syncthreads();   // (the tables are the next piece's)
    produced += (uint64_t)n;
    if (ended) break;       // the input ran dry inside this write: the source's last one
    if (cons >= N) break;   // a full write whose last output took the last frame: the end of file is seen behind it, nothing follows
  }
  if (tid == 0) { L.result[0] = produced; L.result[1] = (unsigned long long)overflow; }
}

// One lane per output frame. mode 0: the schedule of pass A; mode 1: the resampler's bypass (|ratio - 1| < 1e-6, cubic.rs:56-59) — the source
// delivers the file's frames — which leaves the down-mix.
__global__ void __launch_bounds__(256) pg_sample_interp_kernel(PgSampleConv L, int mode) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + (uint64_t)threadIdx.x;
  if (i >= L.n_out) return;
  const int C = (int)L.channels;
  float v[2] = {0.0f, 0.0f};
  if (mode == 1) {
    for (int ch = 0; ch < C; ++ch) v[ch] = L.pcm[i * (uint64_t)C + (uint64_t)ch];
  } else {
    const uint64_t c = (uint64_t)L.cnt[i];   // <= n_frames: frames c - 4 .. c - 1 are the window, oldest first
    const float f = L.frac[i];
    for (int ch = 0; ch < C; ++ch) {
      float y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = c + (uint64_t)j >= 4 ? L.pcm[(c + (uint64_t)j - 4) * (uint64_t)C + (uint64_t)ch] : 0.0f;
      v[ch] = cubic_interp(y[0], y[1], y[2], y[3], f);
    }
  }
  L.out[i] = C == 2 ? (v[0] + v[1]) / 2.0f : v[0];
}

// file rate -> graph rate as the temporary source's resampler holds it
static float sample_ratio(uint32_t file_rate, uint32_t graph_rate) { return (float)((double)file_rate / (double)graph_rate); }
static bool sample_ratio_bypass(float ratio) { return fabsf(ratio - 1.0f) < 0.000001f; }

int sample_buffer_convert(pg_graph* g, SampleBuffer& b) {
  if (b.mono_frames >= 0) return PG_OK;
  const float ratio = sample_ratio(b.rate, g->sample_rate);
  const bool bypass = sample_ratio_bypass(ratio);
  if (bypass && b.channels == 1) { b.d_mono = (float*)b.d_pcm; b.mono_frames = (int64_t)b.n_frames; return PG_OK; }   // sampler.rs:912-914: the buffer itself
  if (!(ratio > 0.0f) || ratio > 64.0f) return set_error(PG_ERR_PARAMETER, "Invalid resampling ratio");
  if (b.n_frames > (1ull << 31)) return set_error(PG_ERR_PARAMETER, "sample buffer is too long for the conversion");
  (void)hipSetDevice(g->device);
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  uint32_t* d_cnt = nullptr; float* d_frac = nullptr; unsigned long long* d_res = nullptr; float* d_out = nullptr;
  auto cleanup = [&]() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (d_cnt) (void)pg_free(d_cnt);
    if (d_frac) (void)pg_free(d_frac);
    if (d_res) (void)pg_free(d_res);
  };
  auto fail = [&](const char* what) { cleanup(); if (d_out) (void)pg_free(d_out); return set_error(PG_ERR_DEVICE, "granular sample buffer: %s failed", what); };
  const bool timed = sample_buffer_timing();   // (measurement hook: no event otherwise)
  if (timed) for (hipEvent_t& e : ev) if (hipEventCreate(&e) != hipSuccess) return fail("hipEventCreate");
  PgSampleConv L;
  memset(&L, 0, sizeof L);
  L.pcm = (const float*)b.d_pcm; L.n_frames = b.n_frames; L.channels = b.channels; L.ratio = ratio;
  uint64_t n_out = b.n_frames;
  if (timed && hipEventRecord(ev[0], g->stream) != hipSuccess) return fail("hipEventRecord");
  if (!bypass) {
    // frames the source can deliver: an output needs floor(k * ratio) pushes, give or take the f32 accumulator's drift (below 2^-23 per step)
    const uint64_t bound = (uint64_t)(((double)b.n_frames + 4.0) / (double)ratio * 1.0001) + 16;
    L.cap_out = (bound / PG_SAMPLE_PIECE + 2) * PG_SAMPLE_PIECE;
    if (pg_malloc((void**)&d_cnt, L.cap_out * sizeof(uint32_t)) != hipSuccess || pg_malloc((void**)&d_frac, L.cap_out * sizeof(float)) != hipSuccess ||
        pg_malloc((void**)&d_res, 2 * sizeof(unsigned long long)) != hipSuccess) return fail("scratch allocation");
    L.cnt = d_cnt; L.frac = d_frac; L.result = d_res;
    hipLaunchKernelGGL(pg_sample_sched_kernel, dim3(1), dim3(256), 0, g->stream, L);
    if (hipGetLastError() != hipSuccess) return fail("pass A launch");
    unsigned long long res[2] = {0, 0};
    if ((timed && hipEventRecord(ev[1], g->stream) != hipSuccess) || pg_stream_sync(g->stream) != hipSuccess ||
        pg_memcpy(res, d_res, sizeof res, hipMemcpyDeviceToHost) != hipSuccess) return fail("pass A");
    if (res[1] || res[0] > L.cap_out) { cleanup(); return set_error(PG_ERR_STATE, "granular sample buffer: the schedule outgrew its table"); }
    n_out = res[0];
  } else if (timed && hipEventRecord(ev[1], g->stream) != hipSuccess) return fail("hipEventRecord");
  const uint64_t n_alloc = n_out ? n_out : 1;   // "Ensure sample buffer is not empty" (sampler.rs:946-949): a single 0.0
  if (pg_malloc((void**)&d_out, n_alloc * sizeof(float)) != hipSuccess) return fail("allocation");
  if (!n_out && pg_memset(d_out, 0, sizeof(float)) != hipSuccess) return fail("memset");
  if (n_out) {
    L.out = d_out; L.n_out = n_out;
    hipLaunchKernelGGL(pg_sample_interp_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, g->stream, L, bypass ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return fail("pass B launch");
  }
  if ((timed && hipEventRecord(ev[2], g->stream) != hipSuccess) || pg_stream_sync(g->stream) != hipSuccess) return fail("pass B");
  if (timed) { (void)hipEventElapsedTime(&b.sched_ms, ev[0], ev[1]); (void)hipEventElapsedTime(&b.interp_ms, ev[1], ev[2]); }
  cleanup();
  b.d_mono = d_out; b.mono_frames = (int64_t)n_alloc;
  return PG_OK;
}
