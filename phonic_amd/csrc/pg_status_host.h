// Host part of the playback status events (pg_graph_poll_status, include/phonic_gpu.h): the bounded ring the records wait in, the compaction
// of the fixed slots pg_playback_status_kernel fills, the order of the records and the merge of several graphs' rings (pg_sharded_poll_status).
// Plain C++: no HIP, no device types — tests/host/status_host.cpp builds it alone, with the sanitizers.
//
// The reference sends every PlaybackStatusEvent with try_send on a bounded channel and drops what finds the channel full
// (src/source/file/common.rs:197-205, :212-219): here a record that finds `capacity` unpolled records in the ring is dropped — the newest
// goes, what waits stays — and counted.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/phonic_gpu.h"

namespace pgs {

// A record on its way to the host's ring: the event, where its voice stands in the reference's traversal of the write that emitted it
// (a mixer's sub-mixers first, then its sources in playing order, src/source/mixed.rs:505-620) and the sub-mixer of the main mixer the voice
// sits under (0: a source of the main mixer itself) — what a merge over several graphs orders by.
struct StatusRec {
  pg_status_event ev;
  uint32_t rank;
  int32_t top;
};

struct StatusRing {
  std::vector<StatusRec> buf;
  size_t head = 0, count = 0;
  uint64_t dropped = 0;
  void reset(size_t capacity) { buf.assign(capacity, StatusRec()); head = 0; count = 0; dropped = 0; }
  size_t capacity() const { return buf.size(); }
  bool push(const StatusRec& r) {  // try_send: a full ring drops the record
    if (count == buf.size()) { dropped += 1; return false; }
    buf[(head + count) % buf.size()] = r;
    count += 1;
    return true;
  }
  const StatusRec* front() const { return count ? &buf[head] : nullptr; }
  void pop() { if (count) { head = (head + 1) % buf.size(); count -= 1; } }
  size_t poll(pg_status_event* out, size_t max_events) {
    size_t n = 0;
    for (; n < max_events && count; ++n) { out[n] = buf[head].ev; pop(); }
    return n;
  }
};

// The jobs of one launch of the status kernel as the host sees them (any struct with slot0, n_slots, count, lost, rank, top: PgStatJob, pg_dev.h).
// Has the kernel run? It stores a job's records first and its count last: a count still at -1 means the launch has not passed.
template <class Job>
bool status_jobs_done(const Job* jobs, size_t n_jobs) {
  for (size_t j = 0; j < n_jobs; ++j) if (*(const volatile int32_t*)&jobs[j].count < 0) return false;
  return true;
}
// Slot compaction: the records of the launch's jobs, job by job, behind what `out` holds; a job's `lost` goes to `lost`.
template <class Job>
void status_gather(const Job* jobs, size_t n_jobs, const pg_status_event* slots, std::vector<StatusRec>& out, uint64_t& lost) {
  for (size_t j = 0; j < n_jobs; ++j) {
    const Job& job = jobs[j];
    const int32_t n = std::min<int32_t>(job.count, job.n_slots);
    for (int32_t i = 0; i < n; ++i) {
      StatusRec r;
      r.ev = slots[(size_t)job.slot0 + (size_t)i];
      r.rank = job.rank; r.top = job.top;
      out.push_back(r);
    }
    if (job.lost > 0) lost += (uint64_t)job.lost;
  }
}
// The order of the records of one chunk of the main mixer: by sample_time, then by the voice's place in the traversal, then as one source write
// emitted them (the gather keeps that order within a job and the jobs of one voice in launch order: the sort is stable).
inline void status_sort(std::vector<StatusRec>& recs) {
  std::stable_sort(recs.begin(), recs.end(), [](const StatusRec& a, const StatusRec& b) {
    return a.ev.sample_time != b.ev.sample_time ? a.ev.sample_time < b.ev.sample_time : a.rank < b.rank;
  });
}
inline void status_flush(std::vector<StatusRec>& recs, StatusRing& ring) {
  for (const StatusRec& r : recs) (void)ring.push(r);
  recs.clear();
}

// Merge of several graphs' rings (the shards of one main mixer) into the same order: the ring whose front record has the smallest
// (sample_time, key(ring, record)) goes first; `key` puts the record's voice into the one mixer's traversal, `remap` turns the record
// into what the caller hands out (a shard's voice id into the handle's). Equal keys: the lower ring.
template <class Key, class Remap>
size_t status_merge(StatusRing* const* rings, size_t n_rings, Key key, Remap remap, pg_status_event* out, size_t max_events) {
  size_t n = 0;
  while (n < max_events) {
    size_t best = n_rings;
    uint64_t best_time = 0;
    decltype(key((size_t)0, StatusRec())) best_key{};
    for (size_t r = 0; r < n_rings; ++r) {
      const StatusRec* f = rings[r]->front();
      if (!f) continue;
      const auto k = key(r, *f);
      if (best == n_rings || f->ev.sample_time < best_time || (f->ev.sample_time == best_time && k < best_key)) { best = r; best_time = f->ev.sample_time; best_key = k; }
    }
    if (best == n_rings) break;
    out[n++] = remap(best, *rings[best]->front());
    rings[best]->pop();
  }
  return n;
}

// SampleTimeClock::duration_to_sample_time (src/utils/time.rs:28-35): (secs * rate as f64) as u64, the cast saturating
inline uint64_t status_emit_rate_frames(double seconds, uint32_t sample_rate) {
  const double f = seconds * (double)sample_rate;
  return !(f > 0.0) ? 0ull : (f >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)f);
}

}  // namespace pgs
