// A stub HIP runtime for the CPU sanitizer build of the library's HOST side (tests/test_sanitizers.py): "device" memory comes from malloc (so
// AddressSanitizer sees every table upload, staging copy and ring write of the host code), copies are memcpy, kernel launches do nothing,
// streams and events are tokens. Eight devices are reported so that the sharded handle routes across distinct device ids. No audio comes out
// of this: it exists to run graph construction, event / command-list bookkeeping, topology rebuilds and the handles' routing under ASan + UBSan
// without a GPU. Built host-only (hipcc --cuda-host-only) against the real HIP headers, linked INSTEAD of libamdhip64.
// A program may install an observer (hip_stub_observer.h) that sees what the library enqueues; without one nothing below is recorded.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "hip_stub_observer.h"

static thread_local int t_device = 0;
static thread_local dim3 t_grid, t_block;
static thread_local size_t t_shmem = 0;
static thread_local hipStream_t t_stream = nullptr;

// ---- the observer: ordinals of streams, events and allocations, kept only while one is installed ----
static stub_observer_fn g_observer = nullptr;
namespace {
struct Tracked {
  std::mutex mtx;
  std::map<const void*, int> streams, events;
  std::map<uintptr_t, std::pair<size_t, int>> allocs;   // base -> (bytes, ordinal)
  int n_streams = 0, n_events = 0, n_allocs = 0;
};
Tracked& tracked() { static Tracked t; return t; }
std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }   // (filled by the module constructors)
void note_alloc(void* p, size_t n) { if (!g_observer || !p) return; Tracked& t = tracked(); std::lock_guard<std::mutex> l(t.mtx); t.allocs[(uintptr_t)p] = {n ? n : 1, t.n_allocs++}; }
void note_free(void* p) { if (!g_observer || !p) return; Tracked& t = tracked(); std::lock_guard<std::mutex> l(t.mtx); t.allocs.erase((uintptr_t)p); }
void note_token(std::map<const void*, int> Tracked::*which, int Tracked::*count, const void* p) {
  if (!g_observer || !p) return;
  Tracked& t = tracked();
  std::lock_guard<std::mutex> l(t.mtx);
  (t.*which)[p] = (t.*count)++;
}
int token_ordinal(std::map<const void*, int> Tracked::*which, const void* p) {
  Tracked& t = tracked();
  std::lock_guard<std::mutex> l(t.mtx);
  auto it = (t.*which).find(p);
  return it == (t.*which).end() ? -1 : it->second;
}
StubCall make_call(StubCallKind kind, hipStream_t stream) { StubCall c; memset((void*)&c, 0, sizeof c); c.kind = kind; c.stream = stream; return c; }
hipError_t observe_launch(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
  if (!g_observer) return hipSuccess;
  auto it = kernel_names().find(fn);
  StubCall c = make_call(STUB_LAUNCH, stream);
  c.name = it == kernel_names().end() ? "?" : it->second.c_str();
  c.grid = grid; c.block = block; c.lds = lds; c.ev0 = e0; c.ev1 = e1; c.args = args;
  g_observer(&c);
  return hipSuccess;
}
}  // namespace

extern "C" {

void hip_stub_set_observer(stub_observer_fn fn) {   // (installing one starts the ordinals again: what was created before is unknown from here on)
  Tracked& t = tracked();
  std::lock_guard<std::mutex> l(t.mtx);
  t.streams.clear(); t.events.clear(); t.allocs.clear();
  t.n_streams = t.n_events = t.n_allocs = 0;
  g_observer = fn;
}
int hip_stub_stream_ordinal(hipStream_t s) { return token_ordinal(&Tracked::streams, s); }
int hip_stub_event_ordinal(hipEvent_t e) { return token_ordinal(&Tracked::events, e); }
int hip_stub_locate(const void* p, size_t* offset) {
  Tracked& t = tracked();
  std::lock_guard<std::mutex> l(t.mtx);
  auto it = t.allocs.upper_bound((uintptr_t)p);
  if (!p || it == t.allocs.begin()) return -1;
  --it;
  if ((uintptr_t)p - it->first > it->second.first) return -1;
  if (offset) *offset = (size_t)((uintptr_t)p - it->first);
  return it->second.second;
}

hipError_t hipGetDeviceCount(int* n) { *n = 8; return hipSuccess; }
hipError_t hipSetDevice(int d) { if (d < 0 || d >= 8) return hipErrorInvalidDevice; t_device = d; return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = t_device; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub HIP runtime"; }
hipError_t hipGetLastError(void) { return hipSuccess; }

hipError_t hipMalloc(void** p, size_t n) { *p = calloc(n ? n : 1, 1); note_alloc(*p, n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { note_free(p); free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = calloc(n ? n : 1, 1); note_alloc(*p, n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { note_free(p); free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) { *d = h; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memmove(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) {
  if (g_observer) { StubCall c = make_call(STUB_MEMCPY_ASYNC, st); c.dst = d; c.src = s; c.bytes = n; g_observer(&c); }
  memmove(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpyPeerAsync(void* d, int dd, const void* s, int sd, size_t n, hipStream_t st) {
  if (g_observer) { StubCall c = make_call(STUB_MEMCPY_PEER_ASYNC, st); c.dst = d; c.src = s; c.bytes = n; c.dst_device = dd; c.src_device = sd; g_observer(&c); }
  memmove(d, s, n);
  return hipSuccess;
}
hipError_t hipDeviceCanAccessPeer(int* can, int, int) { *can = 1; return hipSuccess; }
hipError_t hipDeviceEnablePeerAccess(int, unsigned int) { static unsigned n = 0; return (++n & 1) ? hipSuccess : hipErrorPeerAccessAlreadyEnabled; }   // (both answers the handle accepts)
hipError_t hipMemcpy2DAsync(void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t) {
  for (size_t r = 0; r < height; ++r) memmove((char*)d + r * dpitch, (const char*)s + r * spitch, width);
  return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
  if (g_observer) { StubCall c = make_call(STUB_MEMSET_ASYNC, st); c.dst = d; c.value = v; c.bytes = n; g_observer(&c); }
  memset(d, v, n);
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = (hipStream_t)malloc(8); note_token(&Tracked::streams, &Tracked::n_streams, *s); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) {
  if (g_observer) { StubCall c = make_call(STUB_STREAM_SYNCHRONIZE, s); g_observer(&c); }
  return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t s) {
  if (g_observer) { StubCall c = make_call(STUB_STREAM_QUERY, s); return g_observer(&c) ? hipErrorNotReady : hipSuccess; }   // (the observer scripts the answer)
  static unsigned n = 0;
  return (++n & 1) ? hipErrorNotReady : hipSuccess;   // (both answers get exercised)
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) {
  if (g_observer) { StubCall c = make_call(STUB_STREAM_WAIT_EVENT, s); c.ev0 = e; g_observer(&c); }
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)malloc(8); note_token(&Tracked::events, &Tracked::n_events, *e); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)malloc(8); note_token(&Tracked::events, &Tracked::n_events, *e); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  if (g_observer) { StubCall c = make_call(STUB_EVENT_RECORD, s); c.ev0 = e; g_observer(&c); }
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.1f; return hipSuccess; }

hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t s) { return observe_launch(fn, grid, block, args, lds, s, nullptr, nullptr); }
hipError_t hipExtLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, int) { return observe_launch(fn, grid, block, args, lds, s, e0, e1); }

// what the compiler-generated kernel stubs and module constructors call
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) { t_grid = grid; t_block = block; t_shmem = shmem; t_stream = stream; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) { *grid = t_grid; *block = t_block; *shmem = t_shmem; *stream = t_stream; return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { static void* handle[1]; return handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned int, void*, void*, void*, void*, int*) { kernel_names()[host_fn] = device_name ? device_name : "?"; }
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}

}  // extern "C"
