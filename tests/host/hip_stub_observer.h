// The optional observer of the stub HIP runtime (hip_stub.cpp). Off by default: a program that installs one is called for every kernel launch,
// asynchronous copy / fill, event record, stream wait, stream synchronisation and stream query of the library, each with its arguments, and
// supplies the answer of hipStreamQuery itself. From the moment an observer is installed the stub numbers streams, events and allocations
// (hipMalloc and hipHostMalloc alike) in creation order, from 0, so that a transcript can name them without a raw address: install it before
// the handle under observation is created (installing it again forgets what was numbered before).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

enum StubCallKind {
  STUB_LAUNCH = 0,        // hipLaunchKernel / hipExtLaunchKernel: name, grid, block, lds, stream, ev0, ev1, args
  STUB_MEMCPY_ASYNC,      // dst, src, bytes, stream
  STUB_MEMCPY_PEER_ASYNC, // dst, dst_device, src, src_device, bytes, stream
  STUB_MEMSET_ASYNC,      // dst, value, bytes, stream
  STUB_EVENT_RECORD,      // ev0, stream
  STUB_STREAM_WAIT_EVENT, // stream, ev0
  STUB_STREAM_SYNCHRONIZE,// stream
  STUB_STREAM_QUERY,      // stream; the observer's return value is the answer: 0 = idle (hipSuccess), else busy (hipErrorNotReady)
};
struct StubCall {
  StubCallKind kind;
  const char* name;       // the kernel's (mangled) name as the module constructor registered it; "?" if it registered none
  dim3 grid, block;
  size_t lds;
  hipStream_t stream;
  hipEvent_t ev0, ev1;    // a launch's start and stop event (null for hipLaunchKernel)
  void** args;
  void* dst;
  const void* src;
  size_t bytes;
  int value, dst_device, src_device;
};
typedef int (*stub_observer_fn)(const StubCall* call);

extern "C" {
void hip_stub_set_observer(stub_observer_fn fn);   // null: off again
int hip_stub_stream_ordinal(hipStream_t s);        // creation order, 0-based; -1: null or unknown
int hip_stub_event_ordinal(hipEvent_t e);
// The live allocation that holds `p` (its end included): its ordinal, with the byte offset in *offset; -1: none (host memory of the program, null)
int hip_stub_locate(const void* p, size_t* offset);
}
