// Waveform overviews of a sample buffer, made on the device: phonic::utils::waveform::{mixed_down, multi_channel} (src/utils/waveform.rs:95-199)
// over a slice of the buffer's PCM or of its granular mono buffer — min / max pairs per display column, for a host that draws the sample and keeps
// no copy of it. The arithmetic is the reference's, operation for operation:
//   upscale    (n_frames <= resolution) one point per frame, min == max == the frame's value;
//   downscale  step = n_frames as f32 / resolution as f32; bucket i covers frames [b(i), b(i + 1)), b(i) = min((i as f32 * step) as usize, n_frames):
//              ONE rounded f32 product, truncated. Integer or f64 arithmetic gives other boundaries. A bucket that comes out empty keeps
//              f32::MAX / f32::MIN; the point's frame is b(i) before the clamp, its time b(i) as f32 / rate as f32;
//   mono value fold(0.0, acc + x / ch as f32): every sample is divided first, then added ((0.0 + l / 2) + r / 2, not (l + r) / 2);
//   min / max  f32::min / f32::max skip a NaN, as fminf / fmaxf do. Minimum and maximum do not depend on the order: any partition of a bucket over
//              lanes, waves and workgroups gives the same values (the sign of a zero aside: values are compared).
// Every sample of the slice is read once, whatever the resolution. Three grids, chosen by the mean bucket length `step`:
//   pg_waveform_upscale_kernel   one lane per frame;
//   pg_waveform_bucket_kernel    step < 512: G lanes of a wave per bucket, G = the power of two at or above step / 8 (1 .. 64): about eight frames
//                                per lane, a butterfly over the G lanes, lane 0 writes the point(s);
//   pg_waveform_split_kernel     step >= 512: a bucket is cut into pieces of 2048 frames, one workgroup per piece (a workgroup takes every
//                                `pieces`-th piece of its bucket, so a bucket longer than expected is still covered); the partials go to scratch
//                                with plain vector stores and pg_waveform_combine_kernel, one wave per bucket, folds them into the point(s).
// A range of frames is read as an unaligned head (scalar loads up to the first 16-byte boundary), a float4 body (four mono frames, two stereo
// frames) and a scalar tail: a slice may start at any frame.
#include "pg_host_internal.h"

constexpr int PG_WF_MONO = 0, PG_WF_STEREO_MIXED = 1, PG_WF_STEREO_MULTI = 2;   // what a frame contributes: its sample, its mono value, one value per channel
constexpr uint32_t PG_WF_PIECE = 2048;      // frames per workgroup pass of the split kernel: eight per lane
constexpr float PG_WF_SPLIT_STEP = 512.0f;  // mean bucket length from which buckets are split over workgroups

struct PgWaveform {
  const float* src;            // the slice's first frame, interleaved
  uint64_t n;                  // frames of the slice
  uint32_t res;                // resolution
  uint32_t rate;               // samples_per_sec
  uint32_t g_log2;             // bucket kernel: lanes per bucket = 1 << g_log2
  uint32_t pieces;             // split kernel: workgroups per bucket
  int32_t kind;                // PG_WF_*
  uint32_t pad;
  float4* partial;             // split kernel: [res * pieces] of (min0, max0, min1, max1)
  pg_waveform_point* out;      // [channels out][P]
  uint64_t P;                  // points per channel: min(n, res)
};

struct WfAcc { float mn0, mx0, mn1, mx1; };
__device__ __forceinline__ WfAcc wf_empty() { return WfAcc{FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX}; }   // f32::MAX, f32::MIN (waveform.rs:121-122)
__device__ __forceinline__ void wf_merge(WfAcc& a, const WfAcc& b) { a.mn0 = fminf(a.mn0, b.mn0); a.mx0 = fmaxf(a.mx0, b.mx0); a.mn1 = fminf(a.mn1, b.mn1); a.mx1 = fmaxf(a.mx1, b.mx1); }
__device__ __forceinline__ float wf_mono(float l, float r) { return (0.0f + l / 2.0f) + r / 2.0f; }   // the fold of waveform.rs:107-109 for two channels

template <int KIND>
__device__ __forceinline__ void wf_take1(WfAcc& a, float x) { a.mn0 = fminf(a.mn0, x); a.mx0 = fmaxf(a.mx0, x); }   // mono: 0.0 + x / 1.0 is x (a zero's sign aside)
template <int KIND>
__device__ __forceinline__ void wf_take2(WfAcc& a, float l, float r) {
  if (KIND == PG_WF_STEREO_MIXED) { const float v = wf_mono(l, r); a.mn0 = fminf(a.mn0, v); a.mx0 = fmaxf(a.mx0, v); }
  else { a.mn0 = fminf(a.mn0, l); a.mx0 = fmaxf(a.mx0, l); a.mn1 = fminf(a.mn1, r); a.mx1 = fmaxf(a.mx1, r); }
}

// Frames [a, e) of the slice (a <= e <= L.n), taken by lane l of nl lanes.
template <int KIND>
__device__ __forceinline__ void wf_range(const float* src, uint64_t a, uint64_t e, uint32_t l, uint32_t nl, WfAcc& acc) {
  const uint64_t cnt = e - a;
  if (KIND == PG_WF_MONO) {
    const float* p = src + a;
    uint64_t head = (uint64_t)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);
    if (head > cnt) head = cnt;
    const uint64_t n4 = (cnt - head) >> 2;
    const uint64_t tail0 = head + n4 * 4;
    for (uint64_t t = l; t < head; t += nl) wf_take1<KIND>(acc, p[t]);
    const float4* p4 = (const float4*)(p + head);
    for (uint64_t j = l; j < n4; j += nl) {
      const float4 v = p4[j];
      wf_take1<KIND>(acc, v.x); wf_take1<KIND>(acc, v.y); wf_take1<KIND>(acc, v.z); wf_take1<KIND>(acc, v.w);
    }
    for (uint64_t t = tail0 + l; t < cnt; t += nl) wf_take1<KIND>(acc, p[t]);
  } else {
    const float2* p = (const float2*)src + a;   // a frame is 8 bytes on an 8-byte boundary
    uint64_t head = ((uintptr_t)p & 15u) ? 1 : 0;
    if (head > cnt) head = cnt;
    const uint64_t n2 = (cnt - head) >> 1;
    const uint64_t tail0 = head + n2 * 2;
    for (uint64_t t = l; t < head; t += nl) { const float2 v = p[t]; wf_take2<KIND>(acc, v.x, v.y); }
    const float4* p4 = (const float4*)(p + head);
    for (uint64_t j = l; j < n2; j += nl) {
      const float4 v = p4[j];
      wf_take2<KIND>(acc, v.x, v.y); wf_take2<KIND>(acc, v.z, v.w);
    }
    for (uint64_t t = tail0 + l; t < cnt; t += nl) { const float2 v = p[t]; wf_take2<KIND>(acc, v.x, v.y); }
  }
}

__device__ __forceinline__ float wf_step(const PgWaveform& L) { return __fdiv_rn((float)L.n, (float)L.res); }                 // waveform.rs:119
__device__ __forceinline__ uint64_t wf_bound(uint64_t i, float step) { return (uint64_t)__fmul_rn((float)i, step); }          // :123, :126: before the clamp
__device__ __forceinline__ void wf_shfl_merge(WfAcc& a, int off) {
  WfAcc b;
  b.mn0 = __shfl_xor(a.mn0, off, 64); b.mx0 = __shfl_xor(a.mx0, off, 64); b.mn1 = __shfl_xor(a.mn1, off, 64); b.mx1 = __shfl_xor(a.mx1, off, 64);
  wf_merge(a, b);
}
template <int KIND>
__device__ __forceinline__ void wf_emit(const PgWaveform& L, uint64_t i, uint64_t frame, const WfAcc& a) {
  pg_waveform_point pt;
  pt.frame = frame; pt.time = __fdiv_rn((float)frame, (float)L.rate); pt.min = a.mn0; pt.max = a.mx0; pt.reserved = 0;   // :111, :135
  L.out[i] = pt;
  if (KIND == PG_WF_STEREO_MULTI) { pt.min = a.mn1; pt.max = a.mx1; L.out[L.P + i] = pt; }
}

template <int KIND>
__device__ __forceinline__ void wf_upscale(const PgWaveform& L) {
  const uint64_t f = (uint64_t)blockIdx.x * 256u + (uint64_t)threadIdx.x;
  if (f >= L.n) return;
  WfAcc a;
  if (KIND == PG_WF_MONO) { const float x = L.src[f]; a = WfAcc{x, x, x, x}; }
  else {
    const float2 v = ((const float2*)L.src)[f];
    if (KIND == PG_WF_STEREO_MIXED) { const float m = wf_mono(v.x, v.y); a = WfAcc{m, m, m, m}; }
    else a = WfAcc{v.x, v.x, v.y, v.y};
  }
  wf_emit<KIND>(L, f, f, a);
}

template <int KIND>
__device__ __forceinline__ void wf_bucket(const PgWaveform& L) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256u + (uint64_t)threadIdx.x;
  const uint32_t G = 1u << L.g_log2;
  const uint64_t i = gid >> L.g_log2;   // the same for the G lanes of a group; a group never straddles two waves
  const bool live = i < (uint64_t)L.res;
  WfAcc acc = wf_empty();
  uint64_t frame = 0;
  if (live) {
    const float step = wf_step(L);
    frame = wf_bound(i, step);
    const uint64_t a = frame < L.n ? frame : L.n, e0 = wf_bound(i + 1, step), e = e0 < L.n ? e0 : L.n;
    if (a < e) wf_range<KIND>(L.src, a, e, (uint32_t)gid & (G - 1u), G, acc);
  }
  for (int off = (int)(G >> 1); off > 0; off >>= 1) wf_shfl_merge(acc, off);   // (every lane of the wave takes part)
  if (live && ((uint32_t)gid & (G - 1u)) == 0) wf_emit<KIND>(L, i, frame, acc);
}

template <int KIND>
__device__ __forceinline__ void wf_split(const PgWaveform& L, float4* red) {
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x / L.pieces;
  const uint32_t piece = (uint32_t)((uint64_t)blockIdx.x % L.pieces);
  const float step = wf_step(L);
  const uint64_t a0 = wf_bound(i, step), e0 = wf_bound(i + 1, step);
  const uint64_t a = a0 < L.n ? a0 : L.n, e = e0 < L.n ? e0 : L.n;
  WfAcc acc = wf_empty();
  for (uint64_t s = a + (uint64_t)piece * PG_WF_PIECE; s < e; s += (uint64_t)L.pieces * PG_WF_PIECE) {
    const uint64_t t = e - s < (uint64_t)PG_WF_PIECE ? e : s + PG_WF_PIECE;
    wf_range<KIND>(L.src, s, t, tid, 256u, acc);
  }
  for (int off = 32; off > 0; off >>= 1) wf_shfl_merge(acc, off);
  if ((tid & 63u) == 0) red[tid >> 6] = make_float4(acc.mn0, acc.mx0, acc.mn1, acc.mx1);
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) wf_merge(acc, WfAcc{red[w].x, red[w].y, red[w].z, red[w].w});
    L.partial[blockIdx.x] = make_float4(acc.mn0, acc.mx0, acc.mn1, acc.mx1);
  }
}

template <int KIND>
__device__ __forceinline__ void wf_combine(const PgWaveform& L) {
  const uint64_t i = blockIdx.x;
  WfAcc acc = wf_empty();
  for (uint32_t p = threadIdx.x; p < L.pieces; p += 64u) { const float4 v = L.partial[i * L.pieces + p]; wf_merge(acc, WfAcc{v.x, v.y, v.z, v.w}); }
  for (int off = 32; off > 0; off >>= 1) wf_shfl_merge(acc, off);
  if (threadIdx.x == 0) wf_emit<KIND>(L, i, wf_bound(i, wf_step(L)), acc);
}

// One kernel per grid; the kind of frame, uniform over the launch, picks the body.
#define PG_WF_DISPATCH(body, ...)                                            \
  do {                                                                       \
    if (L.kind == PG_WF_MONO) body<PG_WF_MONO>(__VA_ARGS__);                 \
    else if (L.kind == PG_WF_STEREO_MIXED) body<PG_WF_STEREO_MIXED>(__VA_ARGS__); \
    else body<PG_WF_STEREO_MULTI>(__VA_ARGS__);                              \
  } while (0)
__global__ void __launch_bounds__(256) pg_waveform_upscale_kernel(PgWaveform L) { PG_WF_DISPATCH(wf_upscale, L); }
__global__ void __launch_bounds__(256) pg_waveform_bucket_kernel(PgWaveform L) { PG_WF_DISPATCH(wf_bucket, L); }
__global__ void __launch_bounds__(256) pg_waveform_split_kernel(PgWaveform L) {
  __shared__ float4 red[4];
  PG_WF_DISPATCH(wf_split, L, red);
}
__global__ void __launch_bounds__(64) pg_waveform_combine_kernel(PgWaveform L) { PG_WF_DISPATCH(wf_combine, L); }
#undef PG_WF_DISPATCH

static int waveform_launch(PgWaveform& L, hipStream_t stream) {
  const unsigned long long grid_max = 0x7fffffffull;
  if (L.n <= (uint64_t)L.res) {
    const unsigned long long nb = (L.n + 255) / 256;
    if (nb > grid_max) return set_error(PG_ERR_PARAMETER, "waveform: the slice is too long");
    hipLaunchKernelGGL(pg_waveform_upscale_kernel, dim3((unsigned)nb), dim3(256), 0, stream, L);
    return hipGetLastError() == hipSuccess ? PG_OK : set_error(PG_ERR_DEVICE, "waveform: launch failed");
  }
  if (L.partial) {
    hipLaunchKernelGGL(pg_waveform_split_kernel, dim3(L.res * L.pieces), dim3(256), 0, stream, L);
    if (hipGetLastError() != hipSuccess) return set_error(PG_ERR_DEVICE, "waveform: launch failed");
    hipLaunchKernelGGL(pg_waveform_combine_kernel, dim3(L.res), dim3(64), 0, stream, L);
    return hipGetLastError() == hipSuccess ? PG_OK : set_error(PG_ERR_DEVICE, "waveform: launch failed");
  }
  const unsigned long long nb = (((unsigned long long)L.res << L.g_log2) + 255) / 256;
  if (nb > grid_max) return set_error(PG_ERR_PARAMETER, "waveform: the resolution is too large");
  hipLaunchKernelGGL(pg_waveform_bucket_kernel, dim3((unsigned)nb), dim3(256), 0, stream, L);
  return hipGetLastError() == hipSuccess ? PG_OK : set_error(PG_ERR_DEVICE, "waveform: launch failed");
}

extern "C" {

int64_t pg_graph_sample_buffer_waveform(pg_graph* g, int buffer_id, int source, int mode, uint64_t first_frame, uint64_t n_frames, uint32_t resolution,
                                        pg_waveform_point* out, size_t cap_points) {
  // what can be decided without the buffer: before the handle, before anything touches the device
  if (!out) return -set_error(PG_ERR_PARAMETER, "waveform output must not be null");
  if (resolution == 0) return -set_error(PG_ERR_PARAMETER, "waveform resolution must be > 0");
  if (n_frames == 0) return -set_error(PG_ERR_PARAMETER, "waveform slice must not be empty");
  if (source != PG_WAVEFORM_OF_FILE && source != PG_WAVEFORM_OF_GRANULAR) return -set_error(PG_ERR_PARAMETER, "waveform source must be PG_WAVEFORM_OF_FILE or PG_WAVEFORM_OF_GRANULAR");
  if (mode != PG_WAVEFORM_MIXED_DOWN && mode != PG_WAVEFORM_MULTI_CHANNEL) return -set_error(PG_ERR_PARAMETER, "waveform mode must be PG_WAVEFORM_MIXED_DOWN or PG_WAVEFORM_MULTI_CHANNEL");
  const uint64_t P = std::min<uint64_t>(n_frames, resolution);
  if ((uint64_t)cap_points < P) return -set_error(PG_ERR_PARAMETER, "waveform output holds %zu points, %llu are needed", cap_points, (unsigned long long)P);
  if (!g) return -set_error(PG_ERR_PARAMETER, "graph handle is null");
  SampleBuffer* b = sample_buffer_find(g, buffer_id);
  if (!b) return -PG_ERR_NOT_FOUND;
  if (source == PG_WAVEFORM_OF_GRANULAR) { const int rc = pg_graph_prepare_granular_buffer(g, buffer_id); if (rc) return -rc; }
  const bool gran = source == PG_WAVEFORM_OF_GRANULAR;
  const float* base = gran ? b->d_mono : (const float*)b->d_pcm;
  const uint32_t channels = gran ? 1u : b->channels, rate = gran ? g->sample_rate : b->rate;
  const uint64_t total = gran ? (uint64_t)b->mono_frames : (uint64_t)b->n_frames;
  if (first_frame > total || n_frames > total - first_frame)
    return -set_error(PG_ERR_PARAMETER, "waveform slice [%llu, %llu + %llu) leaves the source's %llu frames", (unsigned long long)first_frame, (unsigned long long)first_frame, (unsigned long long)n_frames, (unsigned long long)total);
  const uint64_t n_out = mode == PG_WAVEFORM_MULTI_CHANNEL ? channels : 1u;
  if ((uint64_t)cap_points < n_out * P) return -set_error(PG_ERR_PARAMETER, "waveform output holds %zu points, %llu are needed", cap_points, (unsigned long long)(n_out * P));

  PgWaveform L;
  memset(&L, 0, sizeof L);
  L.src = base + first_frame * channels; L.n = n_frames; L.res = resolution; L.rate = rate; L.P = P;
  const size_t point_bytes = (size_t)(n_out * P) * sizeof(pg_waveform_point);
  size_t partial_bytes = 0;
  if (n_frames > (uint64_t)resolution) {
    const float step = (float)n_frames / (float)resolution;
    if (step >= PG_WF_SPLIT_STEP) {
      const uint64_t pieces = (uint64_t)(step / (float)PG_WF_PIECE) + 1;
      if (pieces * resolution > 0x7fffffffull) return -set_error(PG_ERR_PARAMETER, "waveform: the slice is too long");
      L.pieces = (uint32_t)pieces;
      partial_bytes = (size_t)(pieces * resolution) * sizeof(float4);
    } else {
      while (L.g_log2 < 6 && (float)(8u << L.g_log2) < step) L.g_log2 += 1;
    }
  }
  (void)hipSetDevice(g->device);
  // behind everything the writes before have enqueued (the buffers are immutable: nothing here changes what a later write renders)
  if (pg_stream_sync(g->stream) != hipSuccess || (g->last_stream && g->last_stream != g->stream && pg_stream_sync(g->last_stream) != hipSuccess))
    return -graph_fail(g, set_error(PG_ERR_DEVICE, "waveform: hipStreamSynchronize failed"));
  char* d_mem = nullptr;   // [points][partials]: the points' size is a multiple of 8, the partials want 16
  const size_t partial_off = (point_bytes + 15) & ~(size_t)15;
  if (pg_malloc((void**)&d_mem, partial_off + partial_bytes) != hipSuccess) return -set_error(PG_ERR_DEVICE, "waveform: allocation of %zu bytes failed", partial_off + partial_bytes);
  L.out = (pg_waveform_point*)d_mem;
  if (partial_bytes) L.partial = (float4*)(d_mem + partial_off);
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool timed = sample_buffer_timing() && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess && hipEventRecord(ev[0], g->stream) == hipSuccess;
  L.kind = channels == 1 ? PG_WF_MONO : (mode == PG_WAVEFORM_MIXED_DOWN ? PG_WF_STEREO_MIXED : PG_WF_STEREO_MULTI);
  int rc = waveform_launch(L, g->stream);
  bool device_failed = rc == PG_ERR_DEVICE;
  if (!rc) {
    const bool stamped = timed && hipEventRecord(ev[1], g->stream) == hipSuccess;
    if (pg_stream_sync(g->stream) != hipSuccess || pg_memcpy(out, d_mem, point_bytes, hipMemcpyDeviceToHost) != hipSuccess) { rc = set_error(PG_ERR_DEVICE, "waveform: the read-back failed"); device_failed = true; }
    else if (stamped) (void)hipEventElapsedTime(&b->waveform_ms, ev[0], ev[1]);
  }
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  (void)pg_free(d_mem);
  if (rc) return device_failed ? -graph_fail(g, rc) : -rc;
  return (int64_t)P;
}

int pg_debug_sample_buffer_waveform_time(pg_graph* g, int buffer_id, float* out_ms) {
  if (!g || !out_ms) return set_error(PG_ERR_PARAMETER, "graph handle or output is null");
  const SampleBuffer* b = sample_buffer_find(g, buffer_id);
  if (!b) return PG_ERR_NOT_FOUND;
  *out_ms = b->waveform_ms;
  return PG_OK;
}

}  // extern "C"
