// Per-mixer peak / RMS level metering: MeteredSource / AudioLevelState (src/source/metered.rs:75-143) for every mixer of a graph
// (PlayerConfig::metering_interval, src/player.rs:162-217, :346-348, :784-786; src/source/mixed/submixer.rs:24). Records shared by the host
// side (pg_k_meter.hip, pg_host.hip, pg_sharded.hip) and pg_meter_kernel. Nothing here is part of the ABI.
#pragma once
#include <stdint.h>

// Published level of one mixer in pinned host memory: the kernel writes seq odd, fence, values, fence, seq even; a reader retries until it
// has seen the same even word on both sides of its copy (pg_graph_mixer_audio_level: no HIP call, no wait).
struct PgMeterPub {
  uint32_t seq;
  uint32_t pad[3];
  float peak[2];
  float rms[2];
};
// AudioLevelState of one mixer (device memory, indexed by mixer id)
struct PgMeterState {
  double sum_square[2];
  float peak_hold[2];
  uint64_t collected_frames;
  uint64_t clock_start;   // SampleTimeClock::start_time
  uint32_t seq;           // the sequence word last written to the mixer's PgMeterPub
  uint32_t pad;
};
static_assert(sizeof(PgMeterPub) == 32 && sizeof(PgMeterState) == 48, "tables are indexed by mixer id");

enum { PG_METER_END_OF_RECORD = 1,   // the record (one write call of the metered mixer) ends behind this span: count, check the interval, publish
       PG_METER_ZEROS = 2 };         // no samples behind the span: n_frames frames of silence (the rest of a host write that ran dry)
// n_frames frames of interleaved stereo f32 at `job.base + off`; `time`: pos_in_frames of the record the span belongs to
struct PgMeterSpan {
  uint64_t off;
  uint64_t time;
  uint32_t n_frames;
  uint32_t flags;
};
enum { PG_METER_JOB_WRITTEN = 1 };   // the host knows the mixer's write returned samples (effects, sub-mixers, pending events, the main mixer)
// One workgroup: the mixer `slot` walks spans [span_first, +span_count) in time order. Without PG_METER_JOB_WRITTEN the kernel decides from
// the sources of unit `unit` whether the mixer had any in its list when the record's call began (MixedSource::write returns 0 and records
// nothing otherwise, src/source/mixed.rs:664-670).
struct PgMeterJob {
  const float* base;
  PgMeterPub* pub;
  int32_t slot, unit;
  int32_t span_first, span_count;
  int32_t flags, pad;
};
