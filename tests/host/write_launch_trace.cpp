// A transcript of what the write path enqueues (graph_write_impl, process_bus_impl, the sharded walk: phonic_amd/csrc/pg_host.hip, pg_sharded.hip)
// against the stub HIP runtime with its observer installed (hip_stub.cpp, hip_stub_observer.h): one line per kernel launch, asynchronous copy / fill,
// event record, stream wait, stream synchronisation and stream query, in the order the host issues them, for a list of small scripted scenarios.
// Launches that take a PgLaunch are decoded field by field, the other kernels argument by argument; pointers appear as a<allocation>+<byte offset>,
// streams and events as their creation ordinals. A kernel the program does not know ends it with an error. The program plays the few words the host
// reads back from the device: the generic kernel's feedback (round << 32 | units deferred, scripted per scenario; pg_k_generic.hip) and the status
// kernel's count of live main-mixer sources. After every call: its return value, the error message if the call set one, pg_graph_deferred_units and, for
// deferred-bus graphs, pg_graph_next_main_event. The output is compared byte for byte with tests/golden/write_launch_trace.txt
// (tests/test_host_write_launches.py).
#include <cxxabi.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "hip_stub_observer.h"
#include "../../include/phonic_gpu.h"
#include "../../phonic_amd/csrc/pg_dev.h"
#include "../../phonic_amd/csrc/pg_meter.h"

// ---- what the scenarios script -----------------------------------------------------------------------------------------------------------
static std::deque<int> g_feedback;      // units the next generic launches report as deferred (empty: 0, steady)
static std::deque<int> g_query_busy;    // answers of the next hipStreamQuery calls (empty: idle)
static int g_live_sources = 1;          // what pg_status_kernel reports
static std::vector<unsigned char> g_last_cmds;   // the command list printed last (a list equal to it is printed as "=")
static bool g_tracing = false;          // inside a traced call (graph construction and the read-backs between the calls are not the write path)

// ---- names -------------------------------------------------------------------------------------------------------------------------------
static std::string P(const void* p) {
  if (!p) return "null";
  size_t off = 0;
  const int a = hip_stub_locate(p, &off);
  if (a < 0) return "host";
  char buf[48];
  snprintf(buf, sizeof buf, "a%d+%zu", a, off);
  return buf;
}
static std::string S(hipStream_t s) { const int o = hip_stub_stream_ordinal(s); return s ? (o < 0 ? "s?" : "s" + std::to_string(o)) : "s-"; }
static std::string E(hipEvent_t e) { const int o = hip_stub_event_ordinal(e); return e ? (o < 0 ? "e?" : "e" + std::to_string(o)) : "-"; }
static std::string kernel_name(const char* mangled) {
  int status = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string n = (status == 0 && d) ? d : mangled;
  free(d);
  const size_t paren = n.find('(');
  if (paren != std::string::npos) n.resize(paren);
  const size_t sp = n.rfind(' ');   // ("void name" of a template instance)
  return sp == std::string::npos ? n : n.substr(sp + 1);
}

// ---- decoders ------------------------------------------------------------------------------------------------------------------------------
// type, unit, frame; then target, param, value bits and value64 where they are not 0
static void print_cmd(const PgCmd& c) {
  uint32_t vb;
  memcpy(&vb, &c.value, 4);
  printf(" [%d u%d f%u", c.type, c.unit, c.frame);
  if (c.target) printf(" t%d", c.target);
  if (c.param) printf(" p%d", c.param);
  if (vb) printf(" v%08x", vb);
  if (c.value64) printf(" q%llx", (unsigned long long)c.value64);
  putchar(']');
}
static void print_cmds(const PgCmd* c, int n) {
  if (n <= 0 || !c) return;
  const size_t bytes = (size_t)n * sizeof(PgCmd);
  if (g_last_cmds.size() == bytes && memcmp(g_last_cmds.data(), c, bytes) == 0) { printf(" ="); return; }
  g_last_cmds.assign((const unsigned char*)c, (const unsigned char*)c + bytes);
  if (n <= 600) { for (int i = 0; i < n; ++i) print_cmd(c[i]); return; }
  for (int i = 0; i < 3; ++i) print_cmd(c[i]);   // (a list of tens of thousands: its ends)
  printf(" ...");
  for (int i = n - 3; i < n; ++i) print_cmd(c[i]);
}
// (the groups "bus", "staged", "defer" and "bp" are left out while every field of the group is null / 0)
static void print_launch(const PgLaunch& L) {
  printf(" m%d w%d nu%d ub%d uo=%s nf%u pos%llu nc%d pc%d rb=%s out=%s at=%s as%llu", L.mode, L.wide, L.n_units, L.unit_base, P(L.unit_order).c_str(), L.n_frames,
         (unsigned long long)L.pos, L.n_chunks, L.pad_chunks, P(L.rows_base).c_str(), P(L.unit_out).c_str(), P(L.audible_tab).c_str(), (unsigned long long)L.audible_stride);
  if (L.bus || L.bus_audible) printf(" bus=%s,%s", P(L.bus).c_str(), P(L.bus_audible).c_str());
  printf(" r%u sch%d sb%d go%u gs%u ce%llu", L.round, L.sched ? 1 : 0, L.sched_bank, L.grid_off, L.grid_span, (unsigned long long)L.call_end);
  if (L.staged_on || L.stage_buf) printf(" staged=%d,%s", L.staged_on, P(L.stage_buf).c_str());
  if (L.defer_count || L.defer_list || L.defer_reset || L.defer_state || L.defer_state_reset)
    printf(" defer=%s,%s,%s,%s,%s", P(L.defer_count).c_str(), P(L.defer_list).c_str(), P(L.defer_reset).c_str(), P(L.defer_state).c_str(), P(L.defer_state_reset).c_str());
  if (L.bus_progress) printf(" bp=%s", P(L.bus_progress).c_str());
  printf(" cmds=%s n%d", P(L.cmds).c_str(), L.n_cmds);
}
// The kernels that take plain arguments or one plain struct: a field code per argument — p pointer, i int32, u uint32, q uint64 — in declaration
// order; a struct's fields follow its natural alignment.
struct Plain { const char* name; const char* args[12]; };
static const Plain PLAIN[] = {
  {"pg_mix_kernel", {"p", "u", "i", "i", "p", "i", "p", "q", "p", "q"}},
  {"pg_mix_kernel_1", {"p", "u", "i", "i", "p", "i"}},
  {"pg_mix_kernel_2", {"p", "u", "i", "p", "i", "p", "i", "p"}},
  {"pg_shard_sum_kernel", {"p", "p", "p", "i", "q", "i", "p", "i", "i", "p", "i"}},
  {"pg_patch_units_kernel", {"p", "p", "i"}},
  {"pg_status_kernel", {"p", "p", "i", "p"}},
  {"pg_store_u64_kernel", {"p", "q"}},
  {"pg_words_to_float_kernel", {"p", "p", "i", "i"}},
  {"pg_float_to_words_kernel", {"p", "p", "i"}},
  {"pg_meter_kernel", {"pppppppq"}},                 // PgMeterLaunch
  {"pg_playback_status_kernel", {"ppppui"}},         // PgStatLaunch
  {"pg_grain_kernel", {"puupppiuppquuq"}},           // PgGrainLaunch
};
static void print_plain(const Plain& k, void** args) {
  for (int a = 0; a < 12 && k.args[a]; ++a) {
    const unsigned char* base = (const unsigned char*)args[a];
    size_t off = 0;
    putchar(' ');
    for (const char* f = k.args[a]; *f; ++f) {
      const size_t sz = (*f == 'p' || *f == 'q') ? 8 : 4;
      off = (off + sz - 1) / sz * sz;
      if (f != k.args[a]) putchar(',');
      if (*f == 'p') { void* p; memcpy(&p, base + off, 8); printf("%s", P(p).c_str()); }
      else if (*f == 'q') { uint64_t v; memcpy(&v, base + off, 8); printf("%llu", (unsigned long long)v); }
      else if (*f == 'u') { uint32_t v; memcpy(&v, base + off, 4); printf("%u", v); }
      else { int32_t v; memcpy(&v, base + off, 4); printf("%d", v); }
      off += sz;
    }
  }
}
// pg_meter_kernel: the jobs of the launch (one per workgroup) and the spans each walks, read from the tables the launch names
static void print_meter_tables(void** args, unsigned n_jobs) {
  const PgMeterJob* jobs; const PgMeterSpan* spans;
  memcpy(&jobs, (const char*)args[0], 8);
  memcpy(&spans, (const char*)args[0] + 8, 8);
  int last_first = -1, last_count = -1;
  for (unsigned j = 0; j < n_jobs; ++j) {
    const PgMeterJob& J = jobs[j];
    printf("\n  job base=%s pub=%s slot%d unit%d spans%d+%d fl%d", P(J.base).c_str(), P(J.pub).c_str(), J.slot, J.unit, J.span_first, J.span_count, J.flags);
    if (J.span_first == last_first && J.span_count == last_count) continue;   // (the sub-mixers of the main mixer share one run of spans)
    last_first = J.span_first; last_count = J.span_count;
    for (int i = 0; i < J.span_count; ++i) { const PgMeterSpan& s = spans[J.span_first + i]; printf(" (%llu t%llu n%u f%u)", (unsigned long long)s.off, (unsigned long long)s.time, s.n_frames, s.flags); }
  }
}

static int observe(const StubCall* c) {
  if (!g_tracing) return 0;
  switch (c->kind) {
    case STUB_MEMCPY_ASYNC: printf("copy %s <- %s %zu %s\n", P(c->dst).c_str(), P(c->src).c_str(), c->bytes, S(c->stream).c_str()); return 0;
    case STUB_MEMCPY_PEER_ASYNC: printf("peercopy %s dev%d <- %s dev%d %zu %s\n", P(c->dst).c_str(), c->dst_device, P(c->src).c_str(), c->src_device, c->bytes, S(c->stream).c_str()); return 0;
    case STUB_MEMSET_ASYNC: printf("fill %s %d %zu %s\n", P(c->dst).c_str(), c->value, c->bytes, S(c->stream).c_str()); return 0;
    case STUB_EVENT_RECORD: printf("record %s %s\n", E(c->ev0).c_str(), S(c->stream).c_str()); return 0;
    case STUB_STREAM_WAIT_EVENT: printf("wait %s for %s\n", S(c->stream).c_str(), E(c->ev0).c_str()); return 0;
    case STUB_STREAM_SYNCHRONIZE: printf("sync %s\n", S(c->stream).c_str()); return 0;
    case STUB_STREAM_QUERY: {
      int busy = 0;
      if (!g_query_busy.empty()) { busy = g_query_busy.front(); g_query_busy.pop_front(); }
      printf("query %s -> %s\n", S(c->stream).c_str(), busy ? "busy" : "idle");
      return busy;
    }
    case STUB_LAUNCH: break;
  }
  const std::string name = kernel_name(c->name);
  printf("K %s g%u", name.c_str(), c->grid.x);
  if (c->grid.y != 1) printf(",%u", c->grid.y);
  printf(" b%u lds%zu %s", c->block.x, c->lds, S(c->stream).c_str());
  if (c->ev0 || c->ev1) printf(" ev=%s,%s", E(c->ev0).c_str(), E(c->ev1).c_str());
  static const char* const UNIT_KERNELS[] = {"pg_unit_kernel", "pg_unit_kernel_fast", "pg_unit_kernel_fast_wide", "pg_unit_kernel_fast_mid", "pg_stage1_kernel", "pg_stage2_kernel", "pg_stage3_kernel",
                                             "pg_stage_fused_kernel", "pg_stage_fused_wide_kernel", "pg_stage_fused_adapt_kernel", "pg_defer_scan_kernel"};
  for (const char* u : UNIT_KERNELS) {
    if (name != u) continue;
    PgLaunch L;
    memcpy((void*)&L, c->args[0], sizeof L);
    print_launch(L);
    if (name == "pg_defer_scan_kernel") {
      PgCmdPack pack;
      memcpy((void*)&pack, c->args[1], sizeof pack);
      printf(" pack%d", pack.n);
      if (pack.n > 0) {   // block 0 leaves the pack where L.cmds points, for the kernels of the round
        print_cmds(pack.c, pack.n);
        memcpy(const_cast<PgCmd*>(L.cmds), pack.c, (size_t)pack.n * sizeof(PgCmd));
      } else print_cmds(L.cmds, L.n_cmds);
    } else print_cmds(L.cmds, L.n_cmds);
    if (name == "pg_unit_kernel" && L.mode == 2 && L.host_feedback) {   // the generic kernel's report (pg_k_generic.hip)
      int n = 0;
      if (!g_feedback.empty()) { n = g_feedback.front(); g_feedback.pop_front(); }
      L.host_feedback[0] = L.host_feedback[3] = ((unsigned long long)L.round << 32) | (unsigned)n;
      printf(" fb%d", n);
    }
    putchar('\n');
    return 0;
  }
  for (const Plain& k : PLAIN) {
    if (name != k.name) continue;
    print_plain(k, c->args);
    if (name == "pg_meter_kernel") print_meter_tables(c->args, c->grid.x);
    if (name == "pg_status_kernel") { int* status; memcpy(&status, c->args[3], 8); *status = g_live_sources; printf(" live%d", g_live_sources); }
    putchar('\n');
    return 0;
  }
  putchar('\n');
  fflush(stdout);
  fprintf(stderr, "write_launch_trace: no decoder for kernel %s\n", name.c_str());
  exit(3);
}

// ---- the graphs ----------------------------------------------------------------------------------------------------------------------------
static std::vector<float> g_pcm;
static float* g_dev = nullptr;      // the caller's device buffer (room for the longest call)
static float* g_host = nullptr;
static const size_t MAX_CALL = 40000;

// Every scenario starts the stub's ordinals again: the caller's device buffer is allocation 0
static void begin_scenario() {
  if (g_dev) (void)hipFree(g_dev);
  hip_stub_set_observer(observe);
  (void)hipMalloc((void**)&g_dev, 2 * 2 * MAX_CALL * sizeof(float));
  g_feedback.clear(); g_query_busy.clear(); g_live_sources = 1; g_last_cmds.clear();
}
static uint32_t fourcc(int kind, int index) {
  pg_param_desc d;
  memset(&d, 0, sizeof d);
  return pg_effect_kind_param(kind, index, &d) == 0 ? d.fourcc : 0;
}
struct Tr {
  pg_graph* g = nullptr;
  bool defer = false;
  uint64_t pos = 0;
  void create(const char* title, size_t mf, int mb, uint32_t rate = 48000) {
    printf("== %s (max_frames %zu, max_blocks %d)\n", title, mf, mb);
    begin_scenario();
    g = pg_graph_create(rate, 2, mf, 0);
    if (!g || pg_graph_set_max_blocks_per_launch(g, mb) != 0) { fprintf(stderr, "create failed: %s\n", pg_last_error_message()); exit(2); }
    defer = false; pos = 0;
  }
  void destroy() { pg_graph_destroy(g); g = nullptr; }
  int mixer(int parent = 0) { return must(pg_graph_add_mixer_to(g, parent)); }
  int fx(int m, int kind) { return must(pg_graph_add_effect(g, m, kind, nullptr)); }
  int voice(int m, size_t n = 4096) { return must(pg_graph_add_voice(g, m, g_pcm.data(), n, 1, 48000, nullptr)); }
  static int must(int id) { if (id < 0) { fprintf(stderr, "graph construction failed: %s\n", pg_last_error_message()); exit(2); } return id; }
  void param(int e, int kind, int index, float v, uint64_t t) { must(-pg_graph_schedule_param(g, e, fourcc(kind, index), v, 1, t)); }
  std::string error_before;   // the thread's error message as the traced call began: a message is printed only when the call set one
  void begin_call() { error_before = pg_last_error_message(); g_tracing = true; }
  void after(const char* what, long long rc, bool failed) {
    g_tracing = false;
    printf("< %s -> %lld", what, rc);
    if (failed && error_before != pg_last_error_message()) printf(" | %s", pg_last_error_message());
    printf(" | deferred %d", pg_graph_deferred_units(g));
    if (defer) printf(" next %lld", (long long)pg_graph_next_main_event(g, pos));
    putchar('\n');
  }
  size_t write(size_t frames, void* stream = nullptr) {
    printf("> write_device %zu at %llu %s\n", frames, (unsigned long long)pos, S((hipStream_t)stream).c_str());
    begin_call();
    const size_t w = pg_graph_write_device(g, g_dev, 2 * frames, pos, stream);
    pos += w / 2;
    after("write_device", (long long)w, w != 2 * frames);
    return w;
  }
  size_t write_host(size_t frames) {
    printf("> write %zu at %llu\n", frames, (unsigned long long)pos);
    begin_call();
    const size_t w = pg_graph_write(g, g_host, 2 * frames, pos);
    pos += w / 2;
    after("write", (long long)w, w != 2 * frames);
    return w;
  }
  int bus(size_t frames, uint64_t at, void* stream = nullptr) {
    printf("> process_bus_device %zu at %llu %s\n", frames, (unsigned long long)at, S((hipStream_t)stream).c_str());
    begin_call();
    const int rc = pg_graph_process_bus_device(g, g_dev, 2 * frames, at, stream);
    after("process_bus_device", rc, rc != 0);
    return rc;
  }
};

static hipStream_t new_stream() { hipStream_t s = nullptr; (void)hipStreamCreateWithFlags(&s, hipStreamNonBlocking); return s; }

// Two sub-mixers with a Gain each (fast kernels), no bus chain: every call length, on the graph's stream and on callers' streams
static void shapes(size_t mf, int mb) {
  Tr t;
  t.create("shapes", mf, mb);
  for (int i = 0; i < 2; ++i) { const int m = t.mixer(); t.fx(m, PG_FX_GAIN); t.voice(m); }
  if (mf == 1024) for (size_t n : {(size_t)1024, (size_t)1, (size_t)7, (size_t)1024, (size_t)4096, (size_t)4097, (size_t)5000, (size_t)32768, (size_t)40000}) t.write(n);
  else for (size_t n : {(size_t)1024, mf, (size_t)7, (size_t)4097}) t.write(n);
  if (mf == 1024 && mb > 1) {
    hipStream_t a = new_stream(), b = new_stream();
    t.write(1024, a); t.write(2048, a); t.write(1024, b); t.write(1024);
    (void)hipStreamDestroy(a); (void)hipStreamDestroy(b);
  }
  t.destroy();
}

// Sub-mixers that end in a Reverb (the staged kernels): steady, a parameter command and three rounds of units still moving, a volume and a panning
// command for one voice at one frame (twice the volume: the one-slot rule), steady again
static void staged(const char* title, int timing_period, bool concurrent_generic, bool brief) {
  if (!concurrent_generic) setenv("PHONIC_CONCURRENT_GENERIC", "0", 1);
  Tr t;
  t.create(title, 1024, 4);
  unsetenv("PHONIC_CONCURRENT_GENERIC");
  pg_graph_set_timing_period(t.g, timing_period);
  int rev = -1, v0 = -1;
  for (int i = 0; i < 3; ++i) { const int m = t.mixer(); t.fx(m, PG_FX_GAIN); rev = t.fx(m, PG_FX_REVERB); v0 = t.voice(m); }
  for (int i = 0; i < (brief ? 2 : 3); ++i) t.write(1024);
  t.param(rev, PG_FX_REVERB, 0, 0.25f, t.pos + 100);
  g_feedback = {2, 1, 1};
  for (int i = 0; i < (brief ? 3 : 5); ++i) t.write(1024);
  if (brief) { t.destroy(); return; }
  Tr::must(-pg_graph_set_voice_volume(t.g, v0, 0.5f, t.pos + 10));
  Tr::must(-pg_graph_set_voice_panning(t.g, v0, -0.5f, t.pos + 10));
  Tr::must(-pg_graph_set_voice_volume(t.g, v0, 0.7f, t.pos + 10));
  for (int i = 0; i < 3; ++i) t.write(1024);
  t.write(4096);
  t.destroy();
}

// A bus chain (Gain -> Delay) behind two small sub-mixers: the overlap pipeline, the pipelined bus, a bus event at a chunk's head
static void bus_chain(const char* title, const char* off_switch) {
  if (off_switch) setenv(off_switch, "0", 1);
  Tr t;
  t.create(title, 1024, 32);
  if (off_switch) unsetenv(off_switch);
  for (int i = 0; i < 2; ++i) { const int m = t.mixer(); t.fx(m, PG_FX_GAIN); t.voice(m); }
  t.fx(0, PG_FX_GAIN);
  const int dly = t.fx(0, PG_FX_DELAY);
  t.write(1024); t.write(1024);
  g_query_busy = {1};
  t.write(off_switch ? 8192 : 32768);
  if (!off_switch) { g_query_busy = {0}; t.write(8192); g_query_busy = {1}; t.write(4096); t.write(1024); }
  t.param(dly, PG_FX_DELAY, 2, 0.3f, t.pos);   // at the head of a chunk of four pieces: the commands ride on a launch of the first block alone
  t.write(8192);
  t.destroy();
}

// Nested mixers P <- C: n distinct events of P inside one chunk of the main mixer (the call budget of PG_MAX_CALLS calls): a chunk of 4096 frames
// in four pieces of 1024, one of 1024 frames in four pieces of 256
static void nested(size_t mf, int n_events, size_t call_frames, uint64_t spacing) {
  Tr t;
  char title[64];
  snprintf(title, sizeof title, "nested, %d events", n_events);
  t.create(title, mf, 1);
  const int p = t.mixer(), c = t.mixer(p);
  const int gain = t.fx(p, PG_FX_GAIN);
  t.fx(c, PG_FX_GAIN);
  t.voice(p); t.voice(c);
  for (int i = 0; i < n_events; ++i) t.param(gain, PG_FX_GAIN, 0, 0.5f + 0.001f * (float)i, 5 + spacing * (uint64_t)i);
  t.write(call_frames);
  t.destroy();
}

// The bus chain deferred to pg_graph_process_bus_device: main-mixer voice events, bus events and budget cuts inside the call, a call that runs
// out of `audible` words, a bus call at a position the write did not record
static void deferred_bus(size_t mf) {
  Tr t;
  t.create("deferred bus", mf, 8);
  pg_graph_set_defer_bus(t.g, 1);
  t.defer = true;
  const int m = t.mixer(), p = t.mixer(), c = t.mixer(p);
  t.fx(m, PG_FX_GAIN); t.voice(m);
  const int pg = t.fx(p, PG_FX_GAIN);
  t.fx(c, PG_FX_GAIN); t.voice(c);
  const int mv = t.voice(0);
  const int bg = t.fx(0, PG_FX_GAIN);
  t.fx(0, PG_FX_DELAY);
  uint64_t at = t.pos;
  t.write(1024); t.bus(1024, at);
  Tr::must(-pg_graph_set_voice_volume(t.g, mv, 0.5f, t.pos + 5000));
  t.param(bg, PG_FX_GAIN, 0, 0.4f, t.pos + 6000);
  for (int i = 0; i < 65; ++i) t.param(pg, PG_FX_GAIN, 0, 0.5f + 0.001f * (float)i, t.pos + 23 + 29 * (uint64_t)i);   // the budget ends the first chunk early
  at = t.pos;
  t.write(8192); t.bus(8192, at);
  t.bus(1024, at + 5);   // (not the position of the last write: no recorded cuts)
  t.destroy();
}
// ... one level, steady: super-block sequences leave a word per block, a main-mixer voice event and a bus event cut the call, and a call longer
// than the graph has `audible` words returns short
static void deferred_bus_flat(size_t mf) {
  Tr t;
  t.create("deferred bus, one level", mf, 32);
  pg_graph_set_defer_bus(t.g, 1);
  t.defer = true;
  const int m = t.mixer();
  t.fx(m, PG_FX_GAIN); t.voice(m);
  const int mv = t.voice(0);
  const int bg = t.fx(0, PG_FX_GAIN);
  t.fx(0, PG_FX_DELAY);
  uint64_t at = t.pos;
  t.write(mf); t.bus(mf, at);
  at = t.pos;
  t.write(mf); t.bus(mf, at);
  Tr::must(-pg_graph_set_voice_volume(t.g, mv, 0.5f, t.pos + 3000));
  t.param(bg, PG_FX_GAIN, 0, 0.4f, t.pos + 5000);
  at = t.pos;
  t.write(9000); t.bus(9000, at);
  at = t.pos;
  const size_t w = t.write(mf * 70);   // more blocks than the call has `audible` words
  t.bus(w / 2, at);
  t.destroy();
}

// Metering: a sub-mixer with sources only (the meter looks at them chunk by chunk), one with an effect, a nested one whose parent cuts the chunk
static void metering() {
  Tr t;
  t.create("metering", 1024, 32);
  const int s = t.mixer(), e = t.mixer(), p = t.mixer(), c = t.mixer(p);
  t.voice(s);
  t.fx(e, PG_FX_GAIN); t.voice(e);
  const int pg = t.fx(p, PG_FX_GAIN);
  t.voice(p); t.fx(c, PG_FX_GAIN); t.voice(c);
  Tr::must(-pg_graph_set_metering(t.g, 0.01));
  t.write(1024);
  t.param(pg, PG_FX_GAIN, 0, 0.3f, t.pos + 700);
  t.param(pg, PG_FX_GAIN, 0, 0.4f, t.pos + 2100);
  t.write(4096);
  t.destroy();
}
static void metering_flat() {   // one level, steady: the sources-only sub-mixer bounds a launch sequence to one chunk
  Tr t;
  t.create("metering, one level", 1024, 32);
  const int s = t.mixer(), e = t.mixer();
  t.voice(s);
  t.fx(e, PG_FX_GAIN); t.voice(e);
  Tr::must(-pg_graph_set_metering(t.g, 0.01));
  t.write(1024); t.write(1024);
  Tr::must(-pg_graph_schedule_param(t.g, 0, fourcc(PG_FX_GAIN, 0), 0.5f, 1, t.pos + 6144));   // an event of a sub-mixer ahead: a sequence ends in front of it
  t.write(8192);
  t.write_host(5000);
  t.destroy();
}

// A voice that reports its playback status (piece by piece whatever max_blocks is), a living granular voice (the commands travel by copy), a
// host-fed voice with feeds between the calls
static void voices() {
  Tr t;
  t.create("status voice", 1024, 32);
  int m = t.mixer();
  t.fx(m, PG_FX_GAIN);
  int v = t.voice(m);
  Tr::must(-pg_graph_enable_status(t.g, 64));
  Tr::must(-pg_graph_set_voice_status(t.g, v, 0.01, 1));
  t.write(1024); t.write(1024); t.write(8192);
  t.destroy();

  t.create("granular voice", 1024, 32);
  m = t.mixer();
  t.fx(m, PG_FX_GAIN);
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  v = Tr::must(pg_graph_add_granular_voice(t.g, m, g_pcm.data(), 4096, &gp, nullptr));
  const int fv = t.voice(m);
  t.write(1024); t.write(1024);
  Tr::must(-pg_graph_set_voice_volume(t.g, fv, 0.5f, t.pos + 10));
  t.write(1024); t.write(1024); t.write(4096);
  t.destroy();

  t.create("host-fed voice", 1024, 32);
  m = t.mixer();
  t.fx(m, PG_FX_GAIN);
  v = Tr::must(pg_graph_add_stream_voice(t.g, m, 2, 48000, 1024, nullptr));
  Tr::must(-pg_graph_feed_voice(t.g, v, g_pcm.data(), 300));
  t.write(256);
  Tr::must(-pg_graph_feed_voice(t.g, v, g_pcm.data(), 500));   // (wraps the ring: two copies)
  t.write(256); t.write(256);
  Tr::must(-pg_graph_end_stream_voice(t.g, v));
  t.write(1024);
  t.destroy();
}

// pg_graph_write into a host buffer, longer than the staging (max_blocks 8 x 1024 frames = 8192): a main-mixer event just before, at and just
// after the staging cap. Behind a bus chain the first launch sequence of a pass is one chunk, so the second one is bounded by what the staging
// still holds (super_block_count), and the pass ends where the next chunk would not fit (the look-ahead of graph_write_impl).
static void host_writes() {
  Tr t;
  t.create("host write", 1024, 8);
  const int m = t.mixer();
  t.fx(m, PG_FX_GAIN); t.voice(m);
  const int mv = t.voice(0);
  t.fx(0, PG_FX_GAIN);
  t.write_host(1024); t.write_host(1024);
  t.write_host(14000);   // (no event: the second sequence of the first pass could take eight blocks, the staging has room for four)
  for (uint64_t at : {(uint64_t)8191, (uint64_t)8192, (uint64_t)8193}) {
    Tr::must(-pg_graph_set_voice_volume(t.g, mv, 0.5f, t.pos + at));
    t.write_host(14000);
  }
  t.destroy();
  // a graph that becomes empty in the middle of a call: the first pass fills the staging (4096 frames), the status word behind it says that no
  // source is left, the second pass finds nothing to do: silence for the rest, and the meter's record of it
  t.create("host write, empty mid-call", 1024, 1);
  t.voice(0);
  Tr::must(-pg_graph_set_metering(t.g, 0.01));
  t.write_host(1024);
  g_live_sources = 0;
  t.write_host(10000);
  t.write_host(1024);
  t.destroy();
}

// More commands in one round than the command ring holds, and rounds that take the ring round once
static void command_ring() {
  Tr t;
  t.create("command ring", 1024, 1);
  const int m = t.mixer();
  const int gain = t.fx(m, PG_FX_GAIN);
  t.voice(m);
  t.write(1024);
  for (int round = 0; round < 3; ++round) {   // 3 x 30000 commands: the third list does not fit behind the second
    for (int i = 0; i < 30000; ++i) t.param(gain, PG_FX_GAIN, 0, 0.5f, t.pos + 5);
    t.write(1024);
  }
  for (int half = 0; half < 2; ++half) {      // 80000 at one frame, queued across two calls (the control ring holds 65536)
    for (int i = 0; i < 40000; ++i) t.param(gain, PG_FX_GAIN, 0, 0.25f, t.pos + 2048);
    t.write(half == 0 ? 1024 : 2048);
  }
  t.destroy();
}

// The host-side error injector: the call returns 0, the graph is failed, later calls launch nothing
static void injected_failure() {
  Tr t;
  t.create("injected failure", 1024, 1);
  const int m = t.mixer();
  t.fx(m, PG_FX_GAIN); t.voice(m);
  t.write(1024);
  pg_debug_fail_launch_round(2);
  t.write(4096);
  t.write(1024);
  t.destroy();
}

// ---- sharded handles (one thread: PHONIC_SHARD_THREADS=0) --------------------------------------------------------------------------------------
static void sharded(int n_shards, bool direct) {
  static const int DEVICES[3] = {0, 1, 2};
  printf("== sharded, %d shard(s), %s\n", n_shards, direct ? "direct delivery" : "peer copies");
  begin_scenario();
  setenv("PHONIC_SHARD_DIRECT", direct ? "1" : "0", 1);
  pg_sharded_graph* s = pg_sharded_create(48000, 2, 1024, DEVICES, n_shards);
  unsetenv("PHONIC_SHARD_DIRECT");
  if (!s) { fprintf(stderr, "create failed: %s\n", pg_last_error_message()); exit(2); }
  // two top-level sub-mixers (three shards: the third has nothing to render) and P <- C under the second; a Gain on the one main mixer
  const int m1 = Tr::must(pg_sharded_add_mixer(s)), m2 = Tr::must(pg_sharded_add_mixer(s));
  const int c = Tr::must(pg_sharded_add_mixer_to(s, m2));
  Tr::must(pg_sharded_add_effect(s, m1, PG_FX_GAIN, nullptr));
  const int pg = Tr::must(pg_sharded_add_effect(s, m2, PG_FX_GAIN, nullptr));
  Tr::must(pg_sharded_add_effect(s, c, PG_FX_GAIN, nullptr));
  const int bg = Tr::must(pg_sharded_add_effect(s, 0, PG_FX_GAIN, nullptr));
  Tr::must(pg_sharded_add_voice(s, m1, g_pcm.data(), 4096, 1, 48000, nullptr));
  Tr::must(pg_sharded_add_voice(s, c, g_pcm.data(), 4096, 1, 48000, nullptr));
  printf("shards of the mixers: %d %d %d\n", pg_sharded_shard_of_mixer(s, m1), pg_sharded_shard_of_mixer(s, m2), pg_sharded_shard_of_mixer(s, c));
  uint64_t pos = 0;
  auto write = [&](size_t frames, bool host) {
    printf("> sharded %s %zu at %llu\n", host ? "write" : "write_device", frames, (unsigned long long)pos);
    g_tracing = true;
    const size_t w = host ? pg_sharded_write(s, g_host, 2 * frames, pos) : pg_sharded_write_device(s, g_dev, 2 * frames, pos);
    g_tracing = false;
    pos += w / 2;
    printf("< -> %zu", w);
    if (w != 2 * frames) printf(" | %s", pg_last_error_message());
    putchar('\n');
  };
  write(1024, false);
  // a main-mixer voice that lands on the last shard takes an event: every shard's grid is cut there; a bus event on the root
  if (n_shards < 3) {
    // (main-mixer voices go to the least loaded shard, the root first on a tie: the second one lands on the last shard)
    Tr::must(pg_sharded_add_voice(s, 0, g_pcm.data(), 4096, 1, 48000, nullptr));
    const int mv = Tr::must(pg_sharded_add_voice(s, 0, g_pcm.data(), 4096, 1, 48000, nullptr));
    printf("shard count %d, the event's voice is voice %d\n", pg_sharded_shard_count(s), mv);
    Tr::must(-pg_sharded_set_voice_volume(s, mv, 0.5f, pos + 1500));
    Tr::must(-pg_sharded_schedule_param(s, bg, fourcc(PG_FX_GAIN, 0), 0.4f, 1, pos + 3000));
    write(5000, false);
    if (n_shards == 1) write(2048, true);
  } else {
    // the call budget: 65 events of P (on a shard that is not the root) inside one chunk
    for (int i = 0; i < 65; ++i) Tr::must(-pg_sharded_schedule_param(s, pg, fourcc(PG_FX_GAIN, 0), 0.5f + 0.001f * (float)i, 1, pos + 23 + 29 * (uint64_t)i));
    write(4096, false);
  }
  pg_sharded_destroy(s);
}

int main() {
  setenv("PHONIC_DEBUG_HOOKS", "1", 1);   // (read once, at the first pg_debug_fail_launch_round)
  setenv("PHONIC_SHARD_THREADS", "0", 1);
  g_pcm.resize(8192);
  for (size_t i = 0; i < g_pcm.size(); ++i) g_pcm[i] = 0.25f * (float)((int)(i % 97) - 48) / 48.0f;
  g_host = (float*)malloc(2 * MAX_CALL * sizeof(float));
  shapes(1024, 32);
  shapes(256, 1);
  shapes(1000, 32);
  staged("staged, timing period 1", 1, true, false);
  staged("staged, timing period 4", 4, true, true);
  staged("staged, generic kernel behind the fast kernels", 1, false, true);
  bus_chain("bus chain", nullptr);
  bus_chain("bus chain, PHONIC_BUS_OVERLAP=0", "PHONIC_BUS_OVERLAP");
  bus_chain("bus chain, PHONIC_BUS_PIPELINE=0", "PHONIC_BUS_PIPELINE");
  nested(256, 63, 1024, 7);
  nested(1024, 64, 4096, 29);
  nested(1024, 65, 4096, 29);
  nested(256, 130, 1024, 7);
  deferred_bus(1024);
  deferred_bus_flat(1024);
  metering();
  metering_flat();
  voices();
  host_writes();
  command_ring();
  injected_failure();
  sharded(1, false);
  sharded(2, true);
  sharded(3, false);
  (void)hipFree(g_dev);
  free(g_host);
  fflush(stdout);
  return 0;
}
