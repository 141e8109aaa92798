// The host part of the playback status events (phonic_amd/csrc/pg_status_host.h) on its own, under AddressSanitizer + UndefinedBehaviorSanitizer:
// the bounded ring with its drop count, the compaction of the kernel's fixed slots, the order of a chunk's records, the merge of several graphs'
// rings, and polls that take less than what waits. No HIP, no device: the jobs and slots the kernel would fill are filled here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <vector>

#include "../../phonic_amd/csrc/pg_status_host.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Job { int32_t rec, slot0, n_slots, count, lost; uint32_t rank; int32_t top; };   // the fields of PgStatJob the host reads

static pg_status_event event(int kind, int voice, uint64_t time, uint64_t frame = 0, int exhausted = 0) {
  pg_status_event e;
  std::memset(&e, 0, sizeof e);
  e.kind = kind; e.voice_id = voice; e.sample_time = time; e.frame_pos = frame; e.position_seconds = (double)frame / 48000.0; e.exhausted = exhausted;
  return e;
}
static pgs::StatusRec rec(int voice, uint64_t time, uint32_t rank, int top = 0, int kind = PG_STATUS_POSITION) {
  pgs::StatusRec r;
  r.ev = event(kind, voice, time); r.rank = rank; r.top = top;
  return r;
}

int main() {
  static_assert(sizeof(pg_status_event) == 40, "the ABI's record");
  // ---- the ring: full, drops (the newest goes, what waits stays), polls smaller than what is pending, wrap-around ----
  {
    pgs::StatusRing ring;
    ring.reset(4);
    for (int i = 0; i < 7; ++i) (void)ring.push(rec(i, (uint64_t)i, 0));
    CHECK(ring.count == 4 && ring.dropped == 3);
    pg_status_event out[8];
    CHECK(ring.poll(out, 3) == 3 && out[0].voice_id == 0 && out[1].voice_id == 1 && out[2].voice_id == 2);
    CHECK(ring.count == 1 && ring.dropped == 3);
    for (int i = 7; i < 12; ++i) (void)ring.push(rec(i, (uint64_t)i, 0));   // three fit (the ring wraps), two are dropped
    CHECK(ring.count == 4 && ring.dropped == 5);
    CHECK(ring.poll(out, 8) == 4 && out[0].voice_id == 3 && out[1].voice_id == 7 && out[2].voice_id == 8 && out[3].voice_id == 9);
    CHECK(ring.poll(out, 8) == 0 && ring.poll(out, 0) == 0);
    (void)ring.push(rec(42, 1, 0));
    CHECK(ring.poll(out, 1) == 1 && out[0].voice_id == 42 && ring.count == 0);
  }
  // ---- slot compaction and the order of a chunk's records ----
  {
    std::vector<pg_status_event> slots(32);
    std::vector<Job> jobs;
    // launch 1 (piece 0): voice 10 (rank 2) sends Position + Stopped at time 0; voice 11 (rank 0) a Position at time 0; voice 12 (rank 1) nothing
    jobs.push_back({0, 0, 3, 2, 0, 2, 0});
    slots[0] = event(PG_STATUS_POSITION, 10, 0, 100); slots[1] = event(PG_STATUS_STOPPED, 10, 0, 0, 1);
    jobs.push_back({1, 3, 3, 1, 0, 0, 0});
    slots[3] = event(PG_STATUS_POSITION, 11, 0, 5);
    jobs.push_back({2, 6, 3, 0, 0, 1, 0});
    // launch 2 (piece 1): voice 12 ends a write that began at time 0 (it sorts in front of launch 1's rank 2); voice 11 one that began at 1024;
    // a job whose count exceeds its slots (the kernel counted what found none in `lost`)
    std::vector<Job> jobs2;
    jobs2.push_back({2, 9, 3, 1, 0, 1, 0});
    slots[9] = event(PG_STATUS_POSITION, 12, 0, 7);
    jobs2.push_back({1, 12, 3, 1, 0, 0, 0});
    slots[12] = event(PG_STATUS_POSITION, 11, 1024, 9);
    jobs2.push_back({3, 15, 2, 5, 3, 3, 0});
    slots[15] = event(PG_STATUS_POSITION, 13, 512, 1); slots[16] = event(PG_STATUS_POSITION, 13, 600, 2);
    CHECK(pgs::status_jobs_done(jobs.data(), jobs.size()));
    jobs2[1].count = -1;
    CHECK(!pgs::status_jobs_done(jobs2.data(), jobs2.size()));   // the launch has not passed: nothing of its chunk is taken
    jobs2[1].count = 1;
    std::vector<pgs::StatusRec> gather;
    uint64_t lost = 0;
    pgs::status_gather(jobs.data(), jobs.size(), slots.data(), gather, lost);
    pgs::status_gather(jobs2.data(), jobs2.size(), slots.data(), gather, lost);
    CHECK(gather.size() == 7 && lost == 3);
    pgs::status_sort(gather);
    const int want_voice[7] = {11, 12, 10, 10, 13, 13, 11};
    const uint64_t want_time[7] = {0, 0, 0, 0, 512, 600, 1024};
    for (int i = 0; i < 7; ++i) CHECK(gather[(size_t)i].ev.voice_id == want_voice[i] && gather[(size_t)i].ev.sample_time == want_time[i]);
    CHECK(gather[2].ev.kind == PG_STATUS_POSITION && gather[3].ev.kind == PG_STATUS_STOPPED && gather[3].ev.exhausted == 1);   // emission order inside one source write
    pgs::StatusRing ring;
    ring.reset(5);
    pgs::status_flush(gather, ring);
    ring.dropped += lost;
    CHECK(gather.empty() && ring.count == 5 && ring.dropped == 2 + 3);
  }
  // ---- the merge of three shards: sub-mixers in the order they were added whatever shard holds them, then the main mixer's sources ----
  {
    pgs::StatusRing a, b, c;
    a.reset(16); b.reset(16); c.reset(16);
    // global sub-mixers 1 (shard 0, local 1), 2 (shard 1, local 1), 3 (shard 0, local 2); main sources: global voice 20 on shard 1 (start 0),
    // 21 on shard 0 (start 0, added later: in front), 22 on shard 2 (start 100)
    (void)a.push(rec(0, 0, 0, 1)); (void)a.push(rec(1, 0, 1, 2)); (void)a.push(rec(2, 0, 5, 0)); (void)a.push(rec(0, 4096, 0, 1));
    (void)b.push(rec(0, 0, 0, 1)); (void)b.push(rec(1, 0, 3, 0)); (void)b.push(rec(1, 4096, 3, 0));
    (void)c.push(rec(0, 100, 0, 0)); (void)c.push(rec(0, 4096, 0, 0));
    const int mixer_global[3][3] = {{0, 1, 3}, {0, 2, 0}, {0, 0, 0}};
    const int voice_global[3][3] = {{10, 11, 21}, {12, 20, 0}, {22, 0, 0}};
    const uint64_t start_of[23] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 100};
    auto key = [&](size_t shard, const pgs::StatusRec& r) {
      if (r.top > 0) return std::make_tuple((uint64_t)mixer_global[shard][r.top], (uint64_t)r.rank, (uint64_t)0);
      const int gv = voice_global[shard][r.ev.voice_id];
      return std::make_tuple(UINT64_MAX, start_of[gv], (uint64_t)(1000 - gv));
    };
    auto remap = [&](size_t shard, const pgs::StatusRec& r) { pg_status_event e = r.ev; e.voice_id = voice_global[shard][r.ev.voice_id]; return e; };
    pgs::StatusRing* rings[3] = {&a, &b, &c};
    pg_status_event out[16];
    size_t n = pgs::status_merge(rings, 3, key, remap, out, 4);   // a poll that takes less than what waits ...
    CHECK(n == 4);
    n += pgs::status_merge(rings, 3, key, remap, out + 4, 12);     // ... and the next one goes on where it stopped
    CHECK(n == 9);
    const int want_voice[9] = {10, 12, 11, 21, 20, 22, 10, 20, 22};
    const uint64_t want_time[9] = {0, 0, 0, 0, 0, 100, 4096, 4096, 4096};
    for (int i = 0; i < 9; ++i) CHECK(out[i].voice_id == want_voice[i] && out[i].sample_time == want_time[i]);
    CHECK(a.count == 0 && b.count == 0 && c.count == 0);
  }
  // ---- the emit rate's conversion (time.rs:28-35) ----
  CHECK(pgs::status_emit_rate_frames(0.05, 48000) == 2400 && pgs::status_emit_rate_frames(1e-9, 48000) == 0 && pgs::status_emit_rate_frames(1e30, 48000) == UINT64_MAX);
  std::printf("ok\n");
  return 0;
}
