// Internals shared by the host-side translation units of libphonic_gpu.so (pg_host.hip: the mixer graph and its write path;
// pg_sampler.hip: envelopes, granular voices and their modulation, sample buffers, samplers; pg_fxstate.hip: effect construction and parameter descriptors;
// pg_effect.hip: the standalone `Effect` handle; pg_sharded.hip: the multi-GPU handle). Nothing here is part of the ABI (include/phonic_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/phonic_gpu.h"
#include "pg_ctrl.h"
#include "pg_dev.h"
#include "pg_meter.h"
#include "pg_dsp_dev.h"
#include "pg_params.h"
#include "pg_status_host.h"

using namespace pgd;
using namespace pgh;

// ---- kernels' launchers (pg_kernels.hip) ----------------------------------------------------------------
size_t pg_fast_scratch_bytes(uint32_t kind_mask);
size_t pg_unit_lds_bytes(uint32_t n_frames, size_t scratch_bytes = 0);
size_t pg_stage_lds_bytes(int stage, uint32_t n_frames);
size_t pg_stage_lds_bytes(int stage, uint32_t n_frames, bool wide);  // wide: the staged kernel that renders effects in front of the reverb (their state slots)
hipError_t pg_launch_units(const PgLaunch& L, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t pg_launch_defer_scan(const PgLaunch& L, hipStream_t stream, hipEvent_t done = nullptr, const PgCmd* h_cmds = nullptr);
hipError_t pg_launch_stages(const PgLaunch& L, hipStream_t stream, int single_launch, int lean, int wide, int adapt, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, hipEvent_t tail_done = nullptr);
hipError_t pg_launch_mix(const float* unit_out, uint32_t stride, int n_units, float* partial, float* bus, uint32_t n_samples, const int32_t* audible_tab,
                         size_t audible_stride, int* audible_out, hipStream_t stream, int n_chunks = 1, size_t chunk_stride = 0, hipEvent_t done = nullptr);
// ---- granular voices (pg_k_grain.hip): one pg_grain_kernel launch renders frames [t0, t0 + n) of every living granular voice ----
struct PgGrainLaunch {
  PgGrainVoice* recs;          // the graph's granular records ...
  uint32_t n_recs;             // ... and how many there are: no record at or beyond it is taken
  uint32_t n_live;             // workgroups of the launch: live[b] = the record workgroup b renders
  const int32_t* live;
  const PgVoice* voices;
  const PgCmd* cmds;           // the piece's command list (PgLaunch::cmds): the kernel picks the voice commands of its voice
  int32_t n_cmds;
  uint32_t sample_rate;
  const float* lut;            // [PG_GRAIN_WINDOWS][PG_GRAIN_LUT_N]
  int32_t* ended;              // mapped host memory, one word per record: set when the kernel finds the record's voice ended
  uint64_t t0;                 // position of the launch's first frame
  uint32_t n;                  // frames of the launch
  uint32_t pad;
  uint64_t chunk_t0;           // position of frame 0 of the voices' staging buffers: the start of the main mixer's chunk this piece belongs to
};
hipError_t pg_launch_grain(const PgGrainLaunch& L, hipStream_t stream);
void pg_grain_build_lut(float* out);   // GRAIN_WINDOW_LUT, host side
// ---- granular-mode samplers (pg_k_gsampler.hip): one pg_gsampler_kernel launch closes the spans that end at a boundary and opens the next ----
hipError_t pg_launch_gsampler(const PgGSamplerLaunch& L, hipStream_t stream);

// ---- errors ---------------------------------------------------------------------------------------------
int set_error(int code, const char* fmt, ...);  // records the thread's last error message (pg_last_error_message) and returns `code`
#define PG_AUDIBLE_SLOTS 64  // >= the largest pg_graph_set_max_blocks_per_launch
#define PG_CMD_RING 65536   // commands in flight between two points at which the host knows the stream drained (2 MB device + 2 MB pinned)
#define PG_CTRL_RING 65536  // control messages waiting for the next write (the reference: 4096 per mixer; here one ring per graph)
#define HIP_TRY(expr)                                                                                    \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) return set_error(PG_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// ---- device memory helpers ------------------------------------------------------------------------------
// Every allocation, release and host-blocking HIP call of the library goes through these wrappers and is counted
// (pg_debug_hip_calls): the reference wraps its audio callback in assert_no_alloc (src/output/cpal.rs:712-715); the test-suite
// checks the same property here — a write() on a built graph allocates nothing, frees nothing and (on a caller's stream) never blocks.
hipError_t pg_malloc(void** p, size_t bytes);
hipError_t pg_host_malloc(void** p, size_t bytes, unsigned flags);
hipError_t pg_free(void* p);
hipError_t pg_host_free(void* p);
hipError_t pg_stream_sync(hipStream_t s);
hipError_t pg_memcpy(void* d, const void* s, size_t n, hipMemcpyKind k);
hipError_t pg_memset(void* d, int v, size_t n);

// Device array that grows by reallocation + device-to-device copy (device-evolved state survives). New elements are collected in a
// small pinned staging block and travel in batches: a full block is flushed by the (non real-time) call that filled it, the rest by
// flush_async() on the render stream at the next write — one copy per <= STAGE elements instead of one per element.
template <class T>
struct DeviceVec {
  static constexpr size_t STAGE = 256;
  T* d = nullptr;
  size_t n = 0, cap = 0;      // n counts staged elements too
  T* h_stage = nullptr;       // pinned, STAGE elements
  size_t n_staged = 0;        // elements [n - n_staged, n) wait in h_stage
  int reserve(size_t want) {  // allocates: graph construction only
    if (want <= cap) return PG_OK;
    size_t ncap = std::max<size_t>(want, cap ? cap * 2 : 16);
    T* nd = nullptr;
    HIP_TRY(pg_malloc((void**)&nd, ncap * sizeof(T)));
    const size_t on_device = n - n_staged;
    if (d && on_device) HIP_TRY(pg_memcpy(nd, d, on_device * sizeof(T), hipMemcpyDeviceToDevice));
    if (d) (void)pg_free(d);
    d = nd;
    cap = ncap;
    return PG_OK;
  }
  int flush() {  // blocking (graph construction)
    if (n_staged) HIP_TRY(pg_memcpy(d + (n - n_staged), h_stage, n_staged * sizeof(T), hipMemcpyHostToDevice));
    n_staged = 0;
    return PG_OK;
  }
  int flush_async(hipStream_t s) {  // from write(): pinned source, no allocation, no wait; the staging block is not touched again before the
    if (n_staged) HIP_TRY(hipMemcpyAsync(d + (n - n_staged), h_stage, n_staged * sizeof(T), hipMemcpyHostToDevice, s));  // next mutation, which drains the stream first
    n_staged = 0;
    return PG_OK;
  }
  int push(const T& v, int* index) {
    int rc = reserve(n + 1);
    if (rc) return rc;
    if (!h_stage) HIP_TRY(pg_host_malloc((void**)&h_stage, STAGE * sizeof(T), hipHostMallocDefault));
    if (n_staged == STAGE && (rc = flush())) return rc;
    h_stage[n_staged++] = v;
    *index = (int)n++;
    return PG_OK;
  }
  void release() { if (d) (void)pg_free(d); if (h_stage) (void)pg_host_free(h_stage); d = nullptr; h_stage = nullptr; n = cap = n_staged = 0; }
};

// Table rebuilt from the host mirror at every topology change: capacity is reserved by the mutating calls (reserve: may allocate),
// the contents travel with ONE asynchronous copy from pinned staging inside write (upload_async: never allocates).
// A rebuild can also happen inside write WITHOUT a mutating call (and its wait) in front of it — a control message switched a Gain's DC
// filter on, stop_all_voices dropped sources (round-2 advisor finding) — so an upload may follow the previous one while that one's
// asynchronous copy has not run yet: the pinned staging alternates between two halves, and a half is only rewritten once the event
// recorded behind its last copy has passed (waited for in the rare case it has not).
template <class T>
struct DeviceTable {
  T* d = nullptr;
  T* h = nullptr;  // pinned staging: two halves of `cap` elements
  size_t n = 0, cap = 0;
  int turn = 0;
  hipEvent_t copied[2] = {nullptr, nullptr};
  bool in_flight[2] = {false, false};
  int reserve(size_t want) {
    if (want <= cap) return PG_OK;
    size_t ncap = std::max<size_t>(want, cap ? cap * 2 : 64);
    if (d) (void)pg_free(d);
    if (h) (void)pg_host_free(h);
    d = nullptr; h = nullptr; cap = 0;
    HIP_TRY(pg_malloc((void**)&d, ncap * sizeof(T)));
    HIP_TRY(pg_host_malloc((void**)&h, 2 * ncap * sizeof(T), hipHostMallocDefault));
    for (int i = 0; i < 2; ++i) { if (!copied[i]) HIP_TRY(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming)); in_flight[i] = false; }  // (the mutating call drained the streams)
    cap = ncap;
    return PG_OK;
  }
  int upload_async(const std::vector<T>& v, hipStream_t s) {
    if (v.size() > cap) return set_error(PG_ERR_STATE, "device table capacity was not reserved by the mutating call");
    if (!v.empty()) {
      T* half = h + (size_t)turn * cap;
      if (in_flight[turn] && hipEventQuery(copied[turn]) != hipSuccess) HIP_TRY(hipEventSynchronize(copied[turn]));
      memcpy(half, v.data(), v.size() * sizeof(T));
      HIP_TRY(hipMemcpyAsync(d, half, v.size() * sizeof(T), hipMemcpyHostToDevice, s));
      HIP_TRY(hipEventRecord(copied[turn], s));
      in_flight[turn] = true;
      turn ^= 1;
    }
    n = v.size();
    return PG_OK;
  }
  void release() {
    if (d) (void)pg_free(d);
    if (h) (void)pg_host_free(h);
    for (int i = 0; i < 2; ++i) { if (copied[i]) (void)hipEventDestroy(copied[i]); copied[i] = nullptr; in_flight[i] = false; }
    d = nullptr; h = nullptr; n = cap = 0;
  }
};

static inline size_t next_pow2(size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; }

// ---- effect instance: host mirror + construction of the device state (pg_fxstate.hip) -----------------------
struct HostFx {
  int kind = 0;
  std::vector<float> init_raw;   // raw value per parameter after `new()/with_parameters`
  std::vector<float> target;     // shadow of the targets (for nothing on the hot path; introspection only)
  bool with_params = false;
  bool has_seeds = false;
  uint32_t fpd_l = 16386, fpd_r = 16386;
  double vib[16] = {0};
  bool has_lfo_seed = false;     // Delay: explicit Xoshiro256++ state of the LFO's random shapes (pg_effect_init::lfo_rng_state)
  uint64_t lfo_rng[4] = {0, 0, 0, 0};
  void* d_mem = nullptr;         // delay-line memory owned by this effect
  size_t d_mem_bytes = 0;
  int last_mixer = -1;           // graph effects: the mixer the effect belonged to when it was removed (its late events stay that mixer's events)
};

PgSmooth make_smooth(const ParamSpec& p, float value, uint32_t sr);
int host_fx_from_init(int kind, const pg_effect_init* init, HostFx& h);
// State of the effect right after `Effect::initialize(sample_rate, 2, max_frames)`.
int build_fx_device_state(HostFx& h, uint32_t sr, int device, bool standalone, PgFx& fx);
// PgCmd::value64 of a parameter update (time-constant coefficients computed with the host's expf)
uint64_t fx_param_aux(int kind, int param, float raw, uint32_t sr);

// Launch tables of pg_meter_kernel (pg_k_meter.hip): pinned host memory in two halves, filled launch by launch
struct MeterRing {
  PgMeterJob* h_jobs = nullptr; PgMeterJob* d_jobs = nullptr;
  PgMeterSpan* h_spans = nullptr; PgMeterSpan* d_spans = nullptr;
  size_t half_jobs = 0, half_spans = 0, nj = 0, ns = 0;   // entries per half / used in the current half
  int turn = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool in_flight[2] = {false, false};
};
#define PG_METER_PUB_CHUNKS 64   // chunks of 1024 published levels: never moved or freed before the graph dies (read from any thread)
// Words in mapped host memory that a kernel sets and the host polls without a wait (pg_sampler.hip): one `ended` word per record
struct MappedWords {
  int32_t* h = nullptr;   // the host's view ...
  int32_t* d = nullptr;   // ... and the device's
  size_t cap = 0;
  int reserve(size_t n, const MappedWords& from);   // (on an empty one) n zeroed words that begin with `from`'s; PG_ERR_DEVICE leaves it empty
  void release();
  volatile int32_t& operator[](size_t i) const { return *(volatile int32_t*)(h + i); }
};

// ---- the graph --------------------------------------------------------------------------------------------
struct Event {  // MixerEvent (src/source/mixed.rs:47-109) resolved to a device command
  uint64_t sample_time;
  uint64_t seq;
  PgCmd cmd;  // unit/frame filled per launch
  int mixer;  // owning mixer (0 = main)
  uint64_t stamp = 0;  // the sample time the message carried: below sample_time only for a message held back to its sampler's start time (pg_sampler.hip)
};

// What a voice id stands for, as the control calls of any thread see it (pg_graph::voice_alive_tab)
enum VoiceKind : int8_t {
  VOICE_DEAD = 0,          // removed (or never added): takes no messages
  VOICE_FILE = 1,          // pg_graph_add_voice
  VOICE_HOST_FED = 2,      // pg_graph_add_stream_voice: no seek, no speed
  VOICE_GRANULAR = 3,      // pg_graph_add_granular_voice: no seek
  VOICE_GRANULAR_MOD = 4,  // ... with a modulation matrix (pg_graph_set_voice_modulation_matrix)
};
static inline bool voice_kind_is_granular(VoiceKind k) { return k == VOICE_GRANULAR || k == VOICE_GRANULAR_MOD; }

struct HostVoice {
  int mixer = -1; int dev_index = -1; uint64_t start_time = 0; void* d_pcm = nullptr; void* d_stage = nullptr; bool outer = false;
  // host-fed source (pg_graph_add_stream_voice): pinned ring + word the feeds are staged in, device ring = d_pcm
  bool transient = true;           // PlayingSource::is_transient (pg_voice_options::non_transient == 0)
  bool stream = false, ended = false, ended_sent = false;
  float* h_ring = nullptr;         // pinned: [cap_frames * channels] floats
  uint32_t channels = 0;
  size_t cap_frames = 0;
  uint64_t fed = 0, sent = 0;      // frames accepted from the host / frames whose copy to the device ring has been enqueued
  uint64_t consumed_known = 0;     // frames the device is known to have read (pg_graph_stream_voice_consumed): bounds what may be overwritten
  uint64_t added_at_write = 0;     // pg_graph::write_count when the voice was added (an envelope is attached before the voice renders a frame)
  bool env = false;                // an envelope was attached (pg_graph_set_voice_envelope): its state sits in pg_graph::d_env[dev_index]
  bool env_live = false;           // ... and the voice has not ended yet: its unit is rendered by the exact kernel (PgUnit::static_defer)
  int gran = -1;                   // granular voice (pg_graph_add_granular_voice): its record in pg_graph::d_gran; d_pcm = the mono buffer, d_stage = the staging buffer
  bool gran_live = false;          // ... and pg_grain_kernel has not reported the voice ended: it renders the voice, the exact kernel its unit
  bool mod = false;                // ... with a modulation matrix (pg_graph_set_voice_modulation_matrix): PgGrainVoice::mod of its record
  int sbuf = -1;                   // the voice plays pg_graph::sample_buffers[sbuf] (pg_graph_add_*_voice_from_buffer): d_pcm stays null — the PCM is the buffer's
  uint64_t stop_time = UINT64_MAX; // the last StopSource time sent for the voice (pg_graph_stop_voice): what a voice that begins to report may find pending (pg_k_status.hip)
  int pstat = -1;                  // playback status (pg_graph_set_voice_status): its record in pg_graph::pstat.d_recs ...
  bool pstat_on = false;           // ... and whether the voice reports anything (Position records, Stopped records or both)
  float* d_trace = nullptr;        // ... of a granular voice: PgGrainVoice::pos_trace (owned by the voice)
  uint32_t file_channels = 0, file_rate = 0;   // the FILE buffer behind the voice: what a Position record divides by (common.rs:195-196) ...
  uint64_t file_samples = 0;                   // ... and its buffer().len() (voice.rs:463)
  int sampler = -1;                // a pool voice of pg_graph::samplers[sampler] (pg_graph_add_sampler): no public id, its unit stays on the exact kernel
};
// What a sampler id stands for, as the message calls of any thread see it (pg_graph::sampler_alive_tab): one of the first two, plus what it was created with
enum : int8_t { SAMPLER_TAB_FILE = 1, SAMPLER_TAB_GRANULAR = 2, SAMPLER_TAB_ENVELOPE = 4, SAMPLER_TAB_MATRIX = 8, SAMPLER_TAB_MAIN = 16 };   // (_MAIN: a source of the main mixer, with the generator's output stage)
// A sampler (pg_graph_add_sampler): the pool's place in the graph; the note layer's state is the device's (PgSamplerRec `rec` of pg_graph::d_samp)
struct HostSampler {
  int mixer = -1, rec = -1;
  int voice_id_slot0 = -1;         // the pool's voices were registered last slot first, so that the mixer's list holds them in slot order: slot k has id voice_id_slot0 - k
  int n_voices = 0;
  bool has_envelope = false, transient = false;
  uint64_t start_time = 0;         // the mixer does not call the sampler before this frame: messages due earlier are held until it (sampler_drain_message)
  bool alive = true;               // until pg_graph_remove_sampler / the removal of its mixer / `stopped` has been seen
  int transpose = 0, finetune = 0; // the base pitch as of the last event STAGED (events are staged in time order): what the next pitch factor is made of
  PgEnvParams env = {};            // has_envelope: the pool's AhdsrParameters as of the last event STAGED — the sustain level an ADCY divides by, the zero times
  // a granular-mode sampler (pg_graph_add_granular_sampler): its note layer is PgGSampler `rec` of pg_graph::d_gsamp (PgSamplerRec `rec` is inert),
  // slot k renders through PgGrainVoice record grain0 + k; with_mod: every slot has a modulation matrix
  bool granular = false, with_mod = false;
  int grain0 = -1;
  // a sampler on the main mixer (pg_graph_add_sampler_to_main / _granular_sampler_to_main): mixer 0, and the ONE source unit that holds its whole pool
  int unit = -1;
};
// A sample buffer on the device (pg_graph_add_sample_buffer): AudioFileBuffer behind an Arc (src/source/file/buffer.rs). The host holds one
// reference until pg_graph_release_sample_buffer, every voice made from it one until its memory is released (graph_voice_release).
struct SampleBuffer {
  void* d_pcm = nullptr;           // interleaved PCM, n_frames * channels floats; null once the last reference is gone
  size_t n_frames = 0;
  uint32_t channels = 0, rate = 0;
  bool has_loop = false;           // AudioFileBuffer::loop_range(), source frames
  uint64_t loop_start = 0, loop_end = 0;
  float* d_mono = nullptr;         // the granular mono buffer at the graph's rate (pg_k_sample.hip); == d_pcm for a mono buffer at that rate
  int64_t mono_frames = -1;        // -1: not made yet
  int use_count = 0;               // voices holding a reference
  bool held = true;                // the host's reference
  float upload_ms = 0.0f, sched_ms = 0.0f, interp_ms = 0.0f;   // pg_debug_sample_buffer_times: taken only while sample_buffer_timing()
  float waveform_ms = 0.0f;        // pg_debug_sample_buffer_waveform_time: the kernels of the buffer's last overview (pg_k_waveform.hip), likewise
};
struct HostMixer {
  int unit_slot = -1;              // sub-mixer unit; for the main mixer: the bus unit
  std::vector<int> voices;         // voice ids in playing order (sorted by start time, insert-before-equal)
  std::vector<int> fx;             // effect ids in chain order
  std::vector<Event> events;       // sorted by sample_time (stable: insert after equal, event.rs:31-38)
  std::vector<PgCmd> messages;     // StopSource messages: applied at the start of the next write
  std::vector<Event> bus_events;   // main mixer only, defer_bus mode: effect events waiting for pg_graph_process_bus_device
  int parent = 0;                  // Player::add_mixer(parent): 0 = the main mixer
  int depth = 1;                   // main mixer 0, its sub-mixers 1, their sub-mixers 2 ...
  std::vector<int> children;       // nested sub-mixers, in the order they were added
  bool removed = false;            // Player::remove_mixer: gone from its parent (with everything under it)
  bool remove_pending = false;     // MixerMessage::RemoveAllPendingEvents waiting for the next write (it needs that write's position)
  uint64_t remove_event_seq = 0;   // ... it covers the events queued before it (Event::seq below this) and the sources added before it
  size_t remove_voice_limit = 0;   //     (voice ids below this): messages are processed in order (mixed.rs:294-313), what arrives later stays
};
// Launch level: the units of one depth of the mixer tree. A mixer reads its sub-mixers' output rows, so the levels are launched
// deepest first, in stream order; the sub-mixers of the main mixer and its sources form the last level (summed by the mix kernels).
struct Level { int off = 0, cnt = 0, n_staged = 0, n_staged_wide = 0, n_staged_adapt = 0, n_static_defer = 0; };

// Playback status events (pg_k_status.hip). The launch tables of pg_playback_status_kernel — its jobs and the record slots they fill — are
// mapped host memory in two halves, like the meter's; a chunk of the main mixer reserves what its launches need before the first one is issued,
// so a chunk's records never straddle a half. A half is reused once the event recorded behind its last launch has passed and its records
// have been compacted into the ring.
struct PstatLaunch { size_t job0 = 0, n_jobs = 0; bool closes = false; };   // one launch; `closes`: the last one of its chunk
struct PstatState {
  bool on = false;
  pgs::StatusRing ring;
  std::vector<pgs::StatusRec> gather;      // the chunk being compacted (capacity kept)
  uint64_t lost = 0;                       // records the device could not place (added to the ring's dropped count)
  PgStatVoice* d_recs = nullptr; size_t n_recs = 0, cap_recs = 0;
  int32_t* d_of_voice = nullptr;           // PgEnvTable::stat_of_voice: one entry per entry of the envelope table
  std::vector<int> voices;                 // ids of the voices that report, in the order they were enabled
  PgStatJob* h_jobs = nullptr; PgStatJob* d_jobs = nullptr;
  pg_status_event* h_slots = nullptr; pg_status_event* d_slots = nullptr;
  size_t half_jobs = 0, half_slots = 0, nj = 0, ns = 0;   // entries per half / used in the current half
  int turn = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool in_flight[2] = {false, false};
  std::vector<PstatLaunch> pending;        // launches whose records have not been compacted yet, oldest first (capacity kept)
  size_t pending_head = 0;
  // the chunk being issued: the voices that report, in traversal order, and what the chunk's launches may still take of the current half
  struct Walk { int voice; int level; uint32_t rank; int top; int unit; };
  std::vector<Walk> walk;
  size_t chunk_jobs_left = 0, chunk_slots_left = 0;
  bool chunk_min_slots = false;            // the chunk's launches would not fit a half with room for everything the exact kernel may log: every job
                                           // takes the slots of one source write, what finds none is counted as dropped
};

struct pg_graph {
  int device = 0;
  uint32_t sample_rate = 48000, channels = 2;
  size_t max_frames = 4096;
  hipStream_t stream = nullptr;
  bool failed = false;  // sticky: GuardedSource semantics
  int fast = 1;
  bool wide = false;  // some sub-mixer chain holds Filter / Eq5 / Distortion: use the wide fast-kernel variant
  uint64_t call_end = 0;   // end position of the write call being rendered (the sharded handle sets it for the whole write, across its segments)
  bool any_outer = false;  // some voice sits behind a ResampledSource: the four-per-CU fast kernel does not carry that code (sticky, like `wide`)
  uint32_t fast_kind_mask = 0;  // effect kinds held by the units the fast kernels render: sizes their LDS arena (pg_fast_scratch_bytes)
  int timing_period = 0;   // time every n-th round with a hipEvent pair (0: never, the default); pg_graph_set_timing_period creates the pairs
  int staged_mode = 1;     // [Gain|Panning]* -> Reverb units: 1 = staged single launch (pg_stage_fused_kernel), 2 = one launch per stage, 0 = fused fast kernel
  int n_staged = 0;        // graph units eligible for the staged pipeline (levels 1 and 2)
  int n_staged_wide = 0;   // ... of level 2 (leading effects beyond Gain / Panning)
  int n_staged_adapt = 0;  // ... of level 3 (a voice behind a ResampledSource or a host-fed one)
  int n_static_defer = 0;  // graph units that always run on the generic kernel
  double* d_stage = nullptr;  // [stage_rows][PG_STAGE_BUF_DOUBLES]
  DeviceTable<int4> d_slot_info;  // per launch slot: {unit slot, first voice, last effect, voices}
  DeviceTable<int2> d_slot_fx;    // per launch slot: {first effect, second effect} (device indices, -1: none)
  DeviceTable<int4> d_slot_lead;  // per launch slot, staged units: the first three effects in front of the reverb (device indices, -1: none)
  DeviceTable<int2> d_child_rows; // nested sub-mixers: {output row, unit slot}, indexed by PgUnit::child_off
  DeviceTable<PgUnit> d_topo;     // topology fields of every unit, patched into d_units by pg_patch_units_kernel
  std::vector<Level> levels;    // deepest first
  uint64_t defer_phase = 0;     // one deferral hand-shake per level launch (two counters, alternating)
  int32_t* d_defer = nullptr;  // [2 counters][2 state counters][defer_rows slots]: compact list of the units the fast kernels deferred
  bool defer_dirty = false;    // a round with a generic launch left a count in its counter: the first round that skips the launch clears all four words
  size_t defer_rows = 0;
  size_t stage_rows = 0;
  bool defer_bus = false;
  size_t max_blocks = 1;        // blocks of max_frames one launch sequence may render (pg_graph_set_max_blocks_per_launch); sizes d_unit_out
  size_t unit_out_blocks = 0;   // per-unit output tables as allocated: max(max_blocks, pieces of a chunk)
  size_t bus_frames = 0;        // frames the staging of pg_graph_write holds (whole chunks: >= PG_MAX_FRAMES)
  size_t audible_slots = 0;     // words of d_audible: one per block of a launch sequence / piece of a chunk
  bool audible_valid = false;   // the last write rendered (its `audible` words are in d_audible)
  // the last deferred-bus write: its position, the words it left (one per piece, in order) and the offsets at which a main-mixer event
  // restarted its chunk grid — pg_graph_process_bus_device of the same position walks the same grid
  uint64_t defer_pos = UINT64_MAX;
  int defer_words = 0;
  std::vector<uint64_t> defer_cuts;
  // Graphs with a bus chain, super-block launches: the unit kernels of launch sequence s + 1 run on a stream of their own UNDER the bus chain of
  // sequence s (one workgroup per effect: the machine is all but idle while it walks the blocks). They need the sum of sequence s to have read
  // the per-unit rows (ev_rows_free, recorded behind the mix launch, in front of the bus launch); the sum of s + 1 needs them done (ev_units_done).
  hipStream_t unit_stream = nullptr;
  hipEvent_t ev_units_done = nullptr, ev_rows_free = nullptr;
  hipStream_t overlap_stream = nullptr;  // the write stream ev_rows_free was last recorded on
  bool rows_free_fresh = false;  // ev_rows_free was recorded behind everything the caller's stream holds that the next unit launch must follow.
                                 // INVARIANT: whatever the library enqueues on a write's stream that a unit kernel reads — topology uploads, command
                                 // lists (stage_commands), stream feeds, a change of stream — must clear this flag (all of them do: rebuild_topology,
                                 // the piece path, flush_stream_feeds, graph_quiesce); the flag persists across calls on purpose, so that a call's
                                 // unit kernels run under the bus chain of the call before. A caller's own work on that stream never feeds a unit kernel.
  uint64_t bus_group = 16;       // blocks per launch sequence of a small unit level in front of a bus chain (PHONIC_BUS_GROUP)
  bool overlap_bus = true;       // PHONIC_BUS_OVERLAP=0 (read at create): everything on the caller's stream
  hipEvent_t ev_scan_done = nullptr, ev_generic_done = nullptr;   // the generic kernel beside the fast kernels (launch_level)
  bool concurrent_generic = true;   // PHONIC_CONCURRENT_GENERIC=0 (read at create): the generic kernel behind the fast kernels, on one stream
  bool messages_due = false;    // StopSource messages wait for the first launch of the write call that has begun
  int32_t* d_error = nullptr;   // sticky consistency flags of the kernels (PG_DEVERR_*)
  unsigned long long* d_bus_progress = nullptr;  // progress words of the pipelined bus chain (pg_bus_pipeline)
  uint32_t bus_epoch = 0;       // launch number of the pipelined bus chain, carried by its progress words
  bool bus_pipeline = true;     // PHONIC_BUS_PIPELINE=0 (read at create): the bus chain behind a super-block stays one workgroup
  // host mirrors
  std::vector<HostMixer> mixers;        // [0] = main
  std::vector<HostVoice> voices;
  std::vector<int> stream_voices;       // ids of the host-fed voices (their feeds are flushed at the top of every write)
  std::vector<int> retired_voices;      // removed sources whose removal has not reached the device yet (the next topology upload carries it)
  std::vector<int> retired_ready;       // ... and those it has: their memory is released at the next graph_quiesce
  std::vector<std::unique_ptr<HostFx>> fx;
  std::vector<int> fx_mixer;            // effect id -> mixer id
  std::vector<int> source_unit_of_voice;  // main-mixer voices: unit slot
  uint64_t event_seq = 0;
  int main_active_voices = 0;           // feedback from the device (sync write only)
  int n_main_samplers = 0;              // living samplers on the main mixer: sources of it whether a note sounds or not (graph_is_empty)
  bool ever_had_main_voice = false;
  // device tables
  DeviceVec<PgUnit> d_units;
  DeviceVec<PgVoice> d_voices;
  DeviceVec<PgFx> d_fx;
  DeviceTable<int32_t> d_voice_index, d_fx_index, d_order;
  // Command lists of the launch rounds: a device ring fed from a pinned host ring of the same size by asynchronous copies, one region
  // per round. A region is reused only after PG_CMD_RING commands have gone through since the last point at which the host knew the
  // stream to be drained (then it waits once): rounds with parameter automation neither allocate nor block.
  PgCmd* d_cmd_ring = nullptr;
  PgCmd* h_cmd_ring = nullptr;
  PgCmd* d_cmd_overflow = nullptr;
  size_t cmd_head = 0, cmds_since_sync = 0;
  hipStream_t last_stream = nullptr;   // the stream of the last write: mutating calls drain it before they touch device tables
  // control path (pg_ctrl.h): messages from any thread, drained at the top of write like MixedSource::process_messages
  pgc::CtrlRing ctrl{PG_CTRL_RING};
  pgc::ChunkTable<int8_t> fx_kind_tab;     // effect id -> kind, -1 once removed (readable from any thread)
  pgc::ChunkTable<int8_t> voice_alive_tab; // voice id -> its VoiceKind: VOICE_DEAD once it takes no more messages (voice_kind)
  DeviceVec<PgSchedEntry> d_sched;       // [classes][2 banks]
  std::map<uint32_t, int> sched_class_of_ratio;
  uint64_t launch_counter = 0;
  std::vector<PgUnit> h_units;          // topology part only (kind, offsets); state fields are device-owned
  bool topo_dirty = true;
  std::vector<int32_t> order;           // launch order: sub-mixer units, then main-mixer source units by start time
  int n_graph_units = 0;                // units excluding bus
  // buffers
  float* d_unit_out = nullptr; size_t unit_out_rows = 0;
  float* d_partial = nullptr; size_t partial_rows = 0;
  float* d_bus = nullptr;               // [2*max_frames + 4]
  int* d_audible = nullptr;             // [audible_slots] audible_input of the bus chain, one word per block of a round / of a deferred-bus call
  hipEvent_t write_done_event = nullptr; // set by the sharded handle around a write: rides on the call's LAST mixer-sum launch as its stop event (write_done_attached says it did)
  bool write_done_attached = false;
  int* d_audible_out = nullptr;         // deferred-bus writes only (pg_sharded, direct delivery): the mixer sum leaves the call's words HERE instead of d_audible — the root's table, on the root's device
  int32_t* d_audible_tab = nullptr;     // [max_blocks][unit_out_rows] per-unit `audible` results, block by block (PgLaunch::audible_tab)
  bool status_pending = false;          // graph_enqueue_status ran, graph_collect_status has not
  float* h_pinned = nullptr;
  unsigned long long* h_feedback = nullptr;   // pinned, device-visible: (round << 32 | deferred units) written by the generic kernel
  unsigned long long* d_feedback = nullptr;   // its device address
  uint64_t last_change_round = 0;             // last round that may have left a unit out of steady state (topology, commands, mode switches)
  uint32_t stride = 0;
  unsigned long long* d_diag = nullptr;  // diagnostic builds
  // timing of the dominant kernel
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  std::vector<uint32_t> ev_blocks;  // max_frames blocks the timed launch rendered (super-block launches: several)
  size_t ev_used = 0;
  // ... and of the main mixer's bus chain (one workgroup per effect: a latency chain — for graphs like BASELINE configs 2 and 4 it is the
  // launch that dominates by GPU time, pg_graph_bus_kernel_stats)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_bus_pool;
  std::vector<uint32_t> ev_bus_blocks;
  size_t ev_bus_used = 0;
  // ... and of the generic kernel's launches, with the counters behind pg_graph_dynamic_stats
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_gen_pool;
  size_t ev_gen_used = 0;
  uint64_t stat_unit_blocks = 0, stat_generic_launches = 0;
  // volume envelopes (pg_graph_set_voice_envelope): side table indexed by the voices' device index, allocated with the first envelope; one word
  // per voice in mapped host memory that the exact kernel sets when an enveloped voice ends (polled at the top of a write: no wait)
  PgEnvTable* d_env_tab = nullptr; // header + entries (PgLaunch::env)
  PgEnv* d_env = nullptr;          // its entries
  MappedWords env_done;            // one word per entry
  std::vector<int> env_voices;     // ids of the voices whose envelope is alive
  // level metering (pg_graph_set_metering, pg_k_meter.hip)
  bool metering = false;           // owner thread's view; meter_on is what pg_graph_mixer_audio_level reads from any thread
  std::atomic<int> meter_on{0};
  uint64_t meter_interval = 0;     // AudioLevelState::update_interval in frames
  bool meter_fragile = false;      // some sub-mixer has neither effects nor sub-mixers: whether it records depends on its sources (rebuild_topology)
  PgMeterState* d_meter_state = nullptr; size_t meter_cap = 0;        // per mixer id
  int32_t* d_meter_seen = nullptr; size_t meter_seen_cap = 0;         // per voice (device index)
  std::atomic<PgMeterPub*> meter_pub[PG_METER_PUB_CHUNKS] = {};       // pinned, published levels by mixer id
  PgMeterPub* meter_pub_dev[PG_METER_PUB_CHUNKS] = {};                // ... their device addresses
  pgc::ChunkTable<int8_t> mixer_alive_tab;                            // mixer id -> 1 until it is removed (readable from any thread)
  MeterRing meter_ring;
  std::vector<PgMeterJob> meter_jobs;    // the launch being put together (capacity kept across writes)
  std::vector<PgMeterSpan> meter_spans;
  std::vector<int> row_of_mixer;         // sub-mixer id -> its row of the per-unit output table (rebuild_topology)
  // granular voices (pg_graph_add_granular_voice): records in device memory (grown by doubling, the graph quiescent), reached by the kernels
  // through the envelope table's header; the window tables, built with the first granular voice; one `ended` word per record in mapped host
  // memory (polled at the top of a write); the records pg_grain_kernel still renders, uploaded when the set changes
  PgGrainVoice* d_gran = nullptr;
  size_t gran_n = 0;                     // records in use (room for gran_ended.cap)
  int32_t* d_grain_of_voice = nullptr;   // one entry per entry of d_env
  float* d_grain_lut = nullptr;
  MappedWords gran_ended;                // one word per record
  std::vector<int> gran_voices;          // ids of the living granular voices
  DeviceTable<int32_t> d_gran_live;      // their records
  std::vector<int32_t> gran_live;        // ... as the next upload puts them together (capacity kept across writes)
  bool gran_live_dirty = false;
  // samplers (pg_graph_add_sampler): the note layer's records in device memory (header + records, grown by doubling with the graph quiescent),
  // reached by the exact kernel through the envelope table's header; speed_from_note's table; one `stopped` word per record in mapped host
  // memory (polled at the top of a write)
  std::vector<HostSampler> samplers;     // by sampler id (ids are never reused)
  pgc::ChunkTable<int8_t> sampler_alive_tab;   // sampler id -> SAMPLER_TAB_* while it takes messages, 0 from then on (readable from any thread)
  pgc::ChunkTable<uint64_t> sampler_frames_tab; // sampler id -> frames of its sample buffer: what a loop range is checked against (appended first)
  PgSamplerTab* d_samp = nullptr;
  size_t samp_cap = 0;                   // records d_samp has room for
  double* d_speed_tab = nullptr;
  MappedWords samp_stopped;              // one word per record
  std::atomic<int64_t> next_note_id{1};  // unique_note_id (generator.rs:32), per graph
  // granular-mode samplers (pg_graph_add_granular_sampler): their note layer's records, indexed like d_samp's (a file sampler's entry is unused);
  // the records of the living ones and of their slots' grain pools, uploaded when the set changes — what pg_gsampler_kernel and the
  // pg_grain_kernel launches of their spans work on
  PgGSampler* d_gsamp = nullptr;
  size_t gsamp_cap = 0;
  size_t n_gsamplers = 0;                // granular samplers ever added (the lists below are reserved for all of them)
  DeviceTable<int32_t> d_gsamp_live, d_gsamp_grains;
  std::vector<int32_t> gsamp_live, gsamp_grains;   // ... as the next upload puts them together (capacity kept across writes)
  bool gsamp_dirty = false;
  PstatState pstat;                      // playback status events (pg_graph_enable_status)
  std::vector<SampleBuffer> sample_buffers;   // by buffer id (ids are never reused)
  uint64_t write_count = 0;        // writes that rendered frames so far, and the suffix maxima of their end positions (write number, end): the
  std::vector<std::pair<uint64_t, uint64_t>> write_end_max;   // largest end of the writes since a voice was added = first entry behind its number
};

// ---- the chunk grid, stated once (pg_dev.h: PG_MAX_FRAMES) ---------------------------------------------------------
// A chunk of chunk_n frames rendered as pieces of at most mf frames (the graph's max_frames): n_full full pieces, then a shorter last one
struct ChunkPieces {
  uint64_t chunk_n, mf;
  uint64_t n_pieces() const { return (chunk_n + mf - 1) / mf; }
  uint64_t n_full() const { return chunk_n / mf; }
  uint64_t piece_len(uint64_t p) const { return std::min<uint64_t>(mf, chunk_n - p * mf); }
};
static inline uint64_t pieces_per_chunk(uint64_t mf) { return ChunkPieces{PG_MAX_FRAMES, mf}.n_pieces(); }
// `audible` words of a span of `frames` frames that starts on the chunk grid and holds no event: one per piece — whole chunks, then the pieces
// of the last, shorter chunk
static inline uint64_t span_audible_words(uint64_t frames, uint64_t mf) { return (frames / PG_MAX_FRAMES) * pieces_per_chunk(mf) + ChunkPieces{frames % PG_MAX_FRAMES, mf}.n_pieces(); }
// Words of an `audible` table (pg_graph::audible_slots, the sharded handle's flag_stride): one per block of a launch sequence / piece of a chunk
static inline size_t audible_table_words(size_t mf) { return std::max<size_t>(PG_AUDIBLE_SLOTS, (size_t)pieces_per_chunk(mf)); }
// Per-unit output tables and meter spans are sized for the blocks of a launch sequence or the pieces of a chunk, whichever is more
static inline size_t graph_table_blocks(const pg_graph* g) { return std::max<size_t>(g->max_blocks, (size_t)pieces_per_chunk(g->max_frames)); }

// ---- graph internals used by the sharded handle and the sampler voices (pg_host.hip) ---------------------------
int graph_quiesce(pg_graph* g);
static inline int graph_fail(pg_graph* g, int code) { g->failed = true; return code; }
void graph_begin_write(pg_graph* g, uint64_t pos);
void drain_control_messages(pg_graph* g);
static inline VoiceKind voice_kind(pg_graph* g, int voice_id) {   // any thread
  return voice_id >= 0 && (size_t)voice_id < g->voice_alive_tab.size() ? (VoiceKind)g->voice_alive_tab.get((size_t)voice_id) : VOICE_DEAD;
}
// One timed message for a voice into the control ring. `need`: VOICE_GRANULAR / VOICE_GRANULAR_MOD for the calls only such a voice takes.
int voice_message(pg_graph* g, int voice_id, VoiceKind need, int type, uint64_t sample_time, float value = 0.0f, int param = 0, double dvalue = 0.0, float value2 = 0.0f);
// The fields every new voice starts with: fader neutral, exponential smoothers at `volume` / `panning`, active, start time and persistence of `opt`
void voice_init_neutral(const pg_graph* g, PgVoice& v, const pg_voice_options* opt, float volume, float panning);
// MixerMessage::AddSource for a voice whose record is d_voices[dev_index]: fills in what every HostVoice holds and returns the new id (< 0: -PG_ERR_*)
// source_unit >= 0: a voice of the main mixer that shares that source unit (a main-mixer sampler's pool: graph_new_sampler_unit); else a unit of its own
int graph_register_voice(pg_graph* g, int mixer_id, int dev_index, const pg_voice_options* opt, HostVoice hv, VoiceKind kind, int source_unit = -1);
int graph_new_sampler_unit(pg_graph* g, int sampler_index);   // a UNIT_SOURCE of the main mixer for the whole pool of that sampler (< 0: the device table could not take it)
void genout_init(const pg_graph* g, PgGenOut& o, float volume, float panning);   // AmplifiedSource::new(.., volume) / PannedSource::new(.., panning) at the graph's rate, on a main-mixer sampler
// Debug read-backs: waits for the graph's stream and the last write's, then copies `bytes` from device memory (PG_OK / PG_ERR_DEVICE)
int graph_read_back(pg_graph* g, void* dst, const void* d_src, size_t bytes);
bool graph_is_empty(const pg_graph* g);
uint64_t graph_frames_to_main_event(const pg_graph* g, uint64_t now);   // frames from `now` to the next main-mixer event behind it (UINT64_MAX: none); events due at `now` are not ahead
int graph_enqueue_status(pg_graph* g, hipStream_t stream);
void graph_collect_status(pg_graph* g);
void graph_call_cuts(const pg_graph* g, uint64_t now, uint64_t chunk_n, std::vector<uint64_t>& cuts);
uint64_t call_budget_bound(std::vector<uint64_t>& cuts, uint64_t now, uint64_t chunk_n);
size_t graph_write_impl(pg_graph* g, float* d_out, size_t n_samples, uint64_t pos, hipStream_t stream, bool begin = true, size_t cap_frames = 0);
int process_bus_impl(pg_graph* g, float* d_bus, size_t n_samples, uint64_t pos_in_frames, hipStream_t s, int* bus_audible);
// level metering (pg_k_meter.hip)
int graph_meter_reserve(pg_graph* g);    // mutating calls, graph quiescent: may allocate
void graph_meter_release(pg_graph* g);
int graph_meter_launch(pg_graph* g, hipStream_t stream);   // g->meter_jobs / g->meter_spans -> one pg_meter_kernel launch
int graph_meter_main(pg_graph* g, const float* d_ptr, uint64_t frames, uint64_t time, bool end_of_record, hipStream_t stream);
// playback status events (pg_k_status.hip)
void graph_pstat_release(pg_graph* g);
// One chunk of the main mixer rendered as pieces, one launch per level and piece. piece_cmds[p] = (unit slot, commands addressed to it) of piece p,
// sorted by unit. begin: the voices that report, in traversal order, and room in the launch tables for all of the chunk's launches.
// launch: pg_playback_status_kernel behind the launch of level `li` that rendered frames [t0, t0 + n) (`first`: the chunk's first piece).
int graph_pstat_begin_chunk(pg_graph* g, const std::vector<std::vector<std::pair<int, int>>>& piece_cmds, hipStream_t stream);
int graph_pstat_launch(pg_graph* g, size_t li, uint64_t t0, uint32_t n, bool first, uint64_t chunk_end, uint32_t round, const std::vector<std::pair<int, int>>& unit_cmds, hipStream_t stream);
void graph_pstat_end_chunk(pg_graph* g);
void graph_pstat_collect(pg_graph* g, bool wait);   // completed chunks -> the ring (wait: for every launch issued so far)
bool voice_has_rendered(const pg_graph* g, const HostVoice& hv);
// sampler voices (pg_sampler.hip)
int pg_ahdsr_params_check(const pg_ahdsr_params* p);   // the reference's parameter errors (PG_OK / PG_ERR_PARAMETER): no graph, no device
int graph_env_reserve(pg_graph* g, size_t n);          // mutating calls, graph quiescent: may allocate
int graph_env_head_refresh(pg_graph* g);               // ... the table's header again, behind a change of a table it names
void graph_sampler_release(pg_graph* g);
void graph_sampler_poll(pg_graph* g);                  // top of a write: voices whose `ended` word is set leave the exact kernel / pg_grain_kernel; stopped samplers leave their mixer
void push_event(pg_graph* g, int mixer, uint64_t sample_time, const PgCmd& cmd, uint64_t stamp = UINT64_MAX);   // (pg_host.hip) one event into a mixer's sorted list; stamp: Event::stamp, default = sample_time
bool sampler_drain_message(pg_graph* g, const pgc::CtrlMsg& m);   // drain_control_messages: a sampler's message -> an event of its mixer (false: not a sampler message)
void sampler_stage_command(pg_graph* g, PgCmd& c);     // an event leaves its mixer's list for a launch (in time order): a base-pitch command gets its pitch factor, an envelope command the field its setter writes
void samplers_of_removed_mixers(pg_graph* g);          // pg_graph_remove_mixer: their ids are dead from here on
int graph_gran_upload_live(pg_graph* g, hipStream_t stream);
int launch_grains(pg_graph* g, uint64_t t0, uint32_t n, uint64_t chunk_t0, const PgCmd* d_cmds, int n_cmds, hipStream_t stream);
// granular-mode samplers (pg_sampler.hip). The living ones' source-write grid inside the chunk [now, now + chunk_n): the positions behind `now` at
// which the mixer chain of any of them cuts (events of its mixer and of that mixer's ancestors, its start time), sorted. Called before the
// chunk's events leave their mixers' lists.
bool graph_has_gsamplers(const pg_graph* g);
void graph_gsampler_cuts(const pg_graph* g, uint64_t now, uint64_t chunk_n, std::vector<uint64_t>& cuts);
int graph_gsampler_upload_live(pg_graph* g, hipStream_t stream);
// pg_gsampler_kernel at boundary `t` = frame `frame` of the piece whose command list is d_cmds (closing: t is the chunk's end) ...
int launch_gsampler_boundary(pg_graph* g, uint64_t t, uint32_t frame, const PgCmd* d_cmds, int n_cmds, uint64_t chunk_t0, bool chunk_first, bool closing, hipStream_t stream);
// ... and pg_grain_kernel over the span [t0, t0 + n) of the living samplers' slots
int launch_gsampler_grains(pg_graph* g, uint64_t t0, uint32_t n, uint64_t chunk_t0, hipStream_t stream);
// sample buffers (pg_sampler.hip; the conversion: pg_k_sample.hip)
int sample_buffer_desc_check(const float* pcm, size_t n_frames, const pg_sample_buffer_desc* desc);   // PG_OK / PG_ERR_PARAMETER: no graph, no device
SampleBuffer* sample_buffer_find(pg_graph* g, int buffer_id);      // the buffer while the host holds it, else null (PG_ERR_NOT_FOUND is set)
void sample_buffer_unref(pg_graph* g, int sbuf);                   // a voice's reference goes: the last one frees the device memory
bool sample_buffer_timing();                                       // PHONIC_DEBUG_HOOKS=1: the upload and the conversion's passes are timed with hipEvents
int sample_buffer_convert(pg_graph* g, SampleBuffer& b);           // makes b.d_mono if it is not there yet; the graph is quiescent
void graph_voice_release(pg_graph* g, HostVoice& hv);              // what a voice owns goes back (graph quiescent): its memory, its buffer reference
void graph_sample_buffers_release(pg_graph* g);                    // pg_graph_destroy: whatever the host still holds
// pg_graph_add_voice / _from_buffer: `pcm` (copied to the device, owned by the voice) or, with pcm null, sample buffer `sbuf`
int graph_add_file_voice(pg_graph* g, int mixer_id, const float* pcm, int sbuf, size_t n_frames, uint32_t src_channels, uint32_t src_rate, const pg_voice_options* opt);
