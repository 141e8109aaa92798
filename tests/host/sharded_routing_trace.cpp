// A transcript of the sharded handle's routing (pg_sharded_* of include/phonic_gpu.h) against the stub HIP runtime (hip_stub.cpp): every entry
// point, on handles of 1, 2 and 3 shards, through a scripted part and a seeded random part, one line per call — entry point, the arguments that
// matter, the return value and, when the call failed, pg_last_error_message(). After every add_mixer* the new mixer's shard is printed, after
// every add_*voice* the use counts of all sample buffers: placement and load accounting are part of the transcript. The output is compared byte
// for byte with tests/golden/sharded_routing_trace.txt (tests/test_host_sharded_routing.py), whatever PHONIC_SHARD_THREADS says.
// Null handles: the calls listed with `golden` below are part of the transcript ("null <entry point> ..." lines); for every other entry point the
// program itself asserts the rule of the header — the return value is the entry point's way of saying PG_ERR_PARAMETER and, where that way sets a
// message, the message names the null handle — and its last line counts them. usage: sharded_routing_trace [record]   (record: transcript only)
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/phonic_gpu.h"

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  int below(int n) { return n <= 0 ? 0 : (int)(next() % (uint64_t)n); }
  float unit() { return (float)(next() >> 40) / (float)(1 << 24); }
};

static const char* A(const char* fmt, ...) {
  static char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}
static void emit(const char* name, const char* args, long long rc, bool failed) {
  printf("%s(%s) -> %lld", name, args, rc);
  if (failed) printf(" | %s", pg_last_error_message());
  putchar('\n');
}
// the three ways an entry point answers: a status (0 or PG_ERR_*), an id or count (negative: -PG_ERR_*), a value that sets no error
static int st(const char* name, const char* args, int rc) { emit(name, args, rc, rc != 0); return rc; }
static long long id(const char* name, const char* args, long long rc) { emit(name, args, rc, rc < 0); return rc; }
static long long quiet(const char* name, const char* args, long long rc) { emit(name, args, rc, false); return rc; }

static const float NaN = NAN;
static uint32_t fx_param(int kind) {
  pg_param_desc d;
  memset(&d, 0, sizeof d);
  return pg_effect_kind_param(kind, 0, &d) == 0 ? d.fourcc : 0;
}
static uint32_t grain_param(int i) {
  pg_param_desc d;
  memset(&d, 0, sizeof d);
  return pg_granular_param(i, &d) == 0 ? d.fourcc : 0;
}

struct Tr {
  pg_sharded_graph* s = nullptr;
  int n_buffers = 0;
  std::vector<float> pcm = std::vector<float>(4096), out = std::vector<float>(2 * 4096);
  pg_grain_state grain;   // (24 KB: not on the stack)
  Tr() { for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = 0.25f * (float)((int)(i % 97) - 48) / 48.0f; }

  void uses() {
    printf("  use_count:");
    for (int b = 0; b < n_buffers; ++b) {
      pg_sample_buffer_info info;
      if (pg_sharded_sample_buffer_info(s, b, &info) == PG_OK) printf(" %d", (int)info.use_count); else printf(" x");
    }
    putchar('\n');
  }
  int shard_of_mixer(int m) { return (int)id("shard_of_mixer", A("%d", m), pg_sharded_shard_of_mixer(s, m)); }
  int add_mixer() { const int m = (int)id("add_mixer", "", pg_sharded_add_mixer(s)); shard_of_mixer(m); return m; }
  int add_mixer_to(int parent) { const int m = (int)id("add_mixer_to", A("%d", parent), pg_sharded_add_mixer_to(s, parent)); shard_of_mixer(m); return m; }
  int add_effect(int m, int kind) { return (int)id("add_effect", A("%d, kind %d", m, kind), pg_sharded_add_effect(s, m, kind, nullptr)); }
  int add_voice(int m, size_t n, uint32_t ch, uint32_t rate, const pg_voice_options* o) {
    const int v = (int)id("add_voice", A("%d, %zu frames, %u ch, %u Hz", m, n, ch, rate), pg_sharded_add_voice(s, m, pcm.data(), n, ch, rate, o));
    uses();
    return v;
  }
  int add_stream_voice(int m, uint32_t ch, uint32_t rate, size_t cap) {
    const int v = (int)id("add_stream_voice", A("%d, %u ch, %u Hz, %zu", m, ch, rate, cap), pg_sharded_add_stream_voice(s, m, ch, rate, cap, nullptr));
    uses();
    return v;
  }
  int add_granular_voice(int m, size_t n, const pg_granular_params* p) {
    const int v = (int)id("add_granular_voice", A("%d, %zu frames, size %g", m, n, p ? (double)p->size : -1.0), pg_sharded_add_granular_voice(s, m, pcm.data(), n, p, nullptr));
    uses();
    return v;
  }
  int feed_voice(int v, size_t n) { return st("feed_voice", A("%d, %zu", v, n), pg_sharded_feed_voice(s, v, pcm.data(), n)); }
  int end_stream_voice(int v) { return st("end_stream_voice", A("%d", v), pg_sharded_end_stream_voice(s, v)); }
  long long stream_voice_consumed(int v) { return id("stream_voice_consumed", A("%d", v), pg_sharded_stream_voice_consumed(s, v)); }
  int remove_mixer(int m) { return st("remove_mixer", A("%d", m), pg_sharded_remove_mixer(s, m)); }
  int remove_effect(int e) { return st("remove_effect", A("%d", e), pg_sharded_remove_effect(s, e)); }
  int move_effect(int e, int m, int mv, int off) { return st("move_effect", A("%d, %d, %d, %d", e, m, mv, off), pg_sharded_move_effect(s, e, m, mv, off)); }
  int schedule_param(int e, uint32_t fcc, float v, int norm, uint64_t t) {
    return st("schedule_param", A("%d, 0x%08x, %g, %d, %llu", e, fcc, (double)v, norm, (unsigned long long)t), pg_sharded_schedule_param(s, e, fcc, v, norm, t));
  }
  int schedule_reset(int e, uint64_t t) { return st("schedule_reset", A("%d, %llu", e, (unsigned long long)t), pg_sharded_schedule_reset(s, e, t)); }
  int set_voice_volume(int v, float x, uint64_t t) { return st("set_voice_volume", A("%d, %g, %llu", v, (double)x, (unsigned long long)t), pg_sharded_set_voice_volume(s, v, x, t)); }
  int set_voice_panning(int v, float x, uint64_t t) { return st("set_voice_panning", A("%d, %g, %llu", v, (double)x, (unsigned long long)t), pg_sharded_set_voice_panning(s, v, x, t)); }
  int set_voice_speed(int v, double x, float g, uint64_t t) { return st("set_voice_speed", A("%d, %g, %g, %llu", v, x, (double)g, (unsigned long long)t), pg_sharded_set_voice_speed(s, v, x, g, t)); }
  int seek_voice(int v, double x, uint64_t t) { return st("seek_voice", A("%d, %g, %llu", v, x, (unsigned long long)t), pg_sharded_seek_voice(s, v, x, t)); }
  int stop_voice(int v, uint64_t t) { return st("stop_voice", A("%d, %llu", v, (unsigned long long)t), pg_sharded_stop_voice(s, v, t)); }
  int stop_all_voices() { return st("stop_all_voices", "", pg_sharded_stop_all_voices(s)); }
  int remove_voice(int v) { return st("remove_voice", A("%d", v), pg_sharded_remove_voice(s, v)); }
  int is_voice_playing(int v) { return (int)quiet("is_voice_playing", A("%d", v), pg_sharded_is_voice_playing(s, v)); }
  int set_voice_envelope(int v, const pg_ahdsr_params* p) { return st("set_voice_envelope", A("%d, attack %g", v, p ? (double)p->attack_s : -1.0), pg_sharded_set_voice_envelope(s, v, p)); }
  int release_voice(int v, uint64_t t) { return st("release_voice", A("%d, %llu", v, (unsigned long long)t), pg_sharded_release_voice(s, v, t)); }
  int voice_envelope_stage(int v) { return (int)quiet("voice_envelope_stage", A("%d", v), pg_sharded_voice_envelope_stage(s, v)); }
  int voice_grain_state(int v) { return st("voice_grain_state", A("%d", v), pg_sharded_voice_grain_state(s, v, &grain)); }
  int set_voice_granular_parameter(int v, uint32_t fcc, float x, int norm, uint64_t t) {
    return st("set_voice_granular_parameter", A("%d, 0x%08x, %g, %d, %llu", v, fcc, (double)x, norm, (unsigned long long)t), pg_sharded_set_voice_granular_parameter(s, v, fcc, x, norm, t));
  }
  int set_voice_grain_loop_range(int v, int has, float a, float b, uint64_t t) {
    return st("set_voice_grain_loop_range", A("%d, %d, %g, %g, %llu", v, has, (double)a, (double)b, (unsigned long long)t), pg_sharded_set_voice_grain_loop_range(s, v, has, a, b, t));
  }
  int voice_granular_params(int v) {
    pg_granular_params p;
    memset(&p, 0, sizeof p);
    const int rc = pg_sharded_voice_granular_params(s, v, &p);
    return st("voice_granular_params", A("%d", v), rc);
  }
  int add_sample_buffer(const float* data, size_t n, const pg_sample_buffer_desc* d) {
    const int b = (int)id("add_sample_buffer", A("%s, %zu frames, %u ch, %u Hz", data ? "pcm" : "null", n, d ? d->channels : 0u, d ? d->rate : 0u), pg_sharded_add_sample_buffer(s, data, n, d));
    if (b >= 0) n_buffers = b + 1;
    return b;
  }
  int release_sample_buffer(int b) { return st("release_sample_buffer", A("%d", b), pg_sharded_release_sample_buffer(s, b)); }
  int add_voice_from_buffer(int m, int b, const pg_voice_options* o) {
    const int v = (int)id("add_voice_from_buffer", A("%d, %d", m, b), pg_sharded_add_voice_from_buffer(s, m, b, o));
    uses();
    return v;
  }
  int add_granular_voice_from_buffer(int m, int b, const pg_granular_params* p) {
    const int v = (int)id("add_granular_voice_from_buffer", A("%d, %d, size %g", m, b, p ? (double)p->size : -1.0), pg_sharded_add_granular_voice_from_buffer(s, m, b, p, nullptr));
    uses();
    return v;
  }
  int prepare_granular_buffer(int b) { return st("prepare_granular_buffer", A("%d", b), pg_sharded_prepare_granular_buffer(s, b)); }
  int sample_buffer_info(int b, bool with_out = true) {
    pg_sample_buffer_info info;
    memset(&info, 0, sizeof info);
    const int rc = pg_sharded_sample_buffer_info(s, b, with_out ? &info : nullptr);
    printf("sample_buffer_info(%d%s) -> %d", b, with_out ? "" : ", null", rc);
    if (rc) printf(" | %s", pg_last_error_message());
    else printf(" frames %llu ch %u rate %u loop %u %llu..%llu uses %d granular %lld", (unsigned long long)info.n_frames, info.channels, info.rate, info.has_loop_range,
                (unsigned long long)info.loop_start, (unsigned long long)info.loop_end, (int)info.use_count, (long long)info.granular_frames);
    putchar('\n');
    return rc;
  }
  long long read_granular_buffer(int b, int shard, size_t cap, bool with_out = true) {
    return id("read_granular_buffer", A("%d, shard %d, %s, %zu", b, shard, with_out ? "out" : "null", cap), pg_sharded_read_granular_buffer(s, b, shard, with_out ? out.data() : nullptr, cap));
  }
  int set_voice_modulation_matrix(int v, const pg_modulation_params* p) {
    return st("set_voice_modulation_matrix", A("%d, velocity %g", v, p ? (double)p->velocity : -1.0), pg_sharded_set_voice_modulation_matrix(s, v, p));
  }
  int set_voice_modulation(int v, int src, int dst, float amount, int bipolar, uint64_t t) {
    return st("set_voice_modulation", A("%d, %d, %d, %g, %d, %llu", v, src, dst, (double)amount, bipolar, (unsigned long long)t), pg_sharded_set_voice_modulation(s, v, src, dst, amount, bipolar, t));
  }
  int clear_voice_modulation(int v, int src, int dst, uint64_t t) {
    return st("clear_voice_modulation", A("%d, %d, %d, %llu", v, src, dst, (unsigned long long)t), pg_sharded_clear_voice_modulation(s, v, src, dst, t));
  }
  int set_voice_lfo_rate(int v, int lfo, float hz, uint64_t t) { return st("set_voice_lfo_rate", A("%d, %d, %g, %llu", v, lfo, (double)hz, (unsigned long long)t), pg_sharded_set_voice_lfo_rate(s, v, lfo, hz, t)); }
  int set_voice_lfo_waveform(int v, int lfo, int w, uint64_t t) { return st("set_voice_lfo_waveform", A("%d, %d, %d, %llu", v, lfo, w, (unsigned long long)t), pg_sharded_set_voice_lfo_waveform(s, v, lfo, w, t)); }
  int voice_modulation_state(int v) {
    pg_modulation_state ms;
    memset(&ms, 0, sizeof ms);
    const int rc = pg_sharded_voice_modulation_state(s, v, &ms);
    return st("voice_modulation_state", A("%d", v), rc);
  }
  int set_metering(double interval) { return st("set_metering", A("%g", interval), pg_sharded_set_metering(s, interval)); }
  int mixer_audio_level(int m, bool with_out = true) {
    pg_audio_level l;
    memset(&l, 0, sizeof l);
    const int rc = pg_sharded_mixer_audio_level(s, m, with_out ? &l : nullptr);
    return st("mixer_audio_level", A("%d%s", m, with_out ? "" : ", null"), rc);
  }
  int enable_status(size_t cap) { return st("enable_status", A("%zu", cap), pg_sharded_enable_status(s, cap)); }
  int set_voice_status(int v, double emit_s, int stopped) { return st("set_voice_status", A("%d, %g, %d", v, emit_s, stopped), pg_sharded_set_voice_status(s, v, emit_s, stopped)); }
  int poll_status(size_t max_events, bool with_out = true) {
    std::vector<pg_status_event> ev(max_events ? max_events : 1);
    const int n = (int)quiet("poll_status", A("%s, %zu", with_out ? "out" : "null", max_events), pg_sharded_poll_status(s, with_out ? ev.data() : nullptr, max_events));
    for (int i = 0; i < n; ++i) printf("  event kind %d voice %d time %llu frame %llu exhausted %d\n", ev[i].kind, ev[i].voice_id, (unsigned long long)ev[i].sample_time, (unsigned long long)ev[i].frame_pos, ev[i].exhausted);
    return n;
  }
  long long status_dropped() { return quiet("status_dropped", "", (long long)pg_sharded_status_dropped(s)); }
  size_t write(size_t frames, uint64_t pos) { return (size_t)quiet("write", A("%zu frames at %llu", frames, (unsigned long long)pos), (long long)pg_sharded_write(s, out.data(), 2 * frames, pos)); }
};

static pg_sample_buffer_desc desc(uint32_t ch, uint32_t rate, bool loop, uint64_t a = 0, uint64_t b = 0) {
  pg_sample_buffer_desc d;
  memset(&d, 0, sizeof d);
  d.channels = ch; d.rate = rate; d.has_loop_range = loop ? 1 : 0; d.loop_start = a; d.loop_end = b;
  return d;
}

// every argument error that is checked in front of the handle, on a null handle (which makes the order visible) and on handle `t.s`
static void argument_errors(Tr& t) {
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  gp.size = NaN;
  pg_ahdsr_params ap;
  pg_ahdsr_params_default(&ap);
  ap.attack_s = -1.0f;
  pg_modulation_params mp;
  pg_modulation_params_default(&mp);
  mp.velocity = 2.0f;
  pg_sample_buffer_desc bad = desc(3, 48000, false);
  t.add_granular_voice(0, 100, &gp);
  t.add_granular_voice(0, 100, nullptr);
  t.add_granular_voice_from_buffer(0, 0, &gp);
  t.add_granular_voice_from_buffer(-1, -1, nullptr);
  t.set_voice_envelope(0, &ap);
  t.set_voice_envelope(-1, nullptr);
  t.set_voice_modulation_matrix(0, &mp);
  t.set_voice_modulation_matrix(-1, nullptr);
  t.add_sample_buffer(t.pcm.data(), 100, &bad);
  t.add_sample_buffer(nullptr, 100, &bad);
  t.add_sample_buffer(t.pcm.data(), 0, nullptr);
  t.set_metering((double)NaN);
  t.set_metering(INFINITY);
  t.set_voice_status(0, (double)NaN, 1);
  t.set_voice_status(-1, (double)NaN, 1);
  t.set_voice_modulation(0, 9, 0, 0.5f, 0, 0);
  t.set_voice_modulation(0, 0, 9, 0.5f, 0, 0);
  t.set_voice_modulation(-1, 0, 0, 1.5f, 0, 0);
  t.clear_voice_modulation(0, -1, 0, 0);
  t.set_voice_lfo_rate(0, 2, 1.0f, 0);
  t.set_voice_lfo_rate(-1, 0, NaN, 0);
  t.set_voice_lfo_waveform(0, 0, 7, 0);
  t.set_voice_lfo_waveform(-1, -1, 0, 0);
  t.set_voice_granular_parameter(0, 0x12345678u, 0.5f, 0, 0);
  t.set_voice_granular_parameter(-1, grain_param(2), NaN, 0, 0);
  t.set_voice_grain_loop_range(0, 1, -0.5f, 0.5f, 0);
  t.set_voice_grain_loop_range(-1, 1, 0.2f, 1.5f, 0);
  t.enable_status(0);
  t.mixer_audio_level(0, false);
  t.sample_buffer_info(0, false);
  t.read_granular_buffer(0, -1, 16, false);
}

// every call that takes an id, on the id `x` of each kind (negative, one past the end, removed)
static void bad_ids(Tr& t, int voice, int fx, int mixer, int buffer, uint64_t pos) {
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  pg_ahdsr_params ap;
  pg_ahdsr_params_default(&ap);
  pg_modulation_params mp;
  pg_modulation_params_default(&mp);
  t.add_mixer_to(mixer); t.add_effect(mixer, 0); t.add_voice(mixer, 100, 1, 48000, nullptr); t.add_stream_voice(mixer, 2, 48000, 1024); t.add_granular_voice(mixer, 100, &gp);
  t.add_voice_from_buffer(mixer, 1, nullptr); t.add_granular_voice_from_buffer(mixer, 1, &gp); t.add_voice_from_buffer(0, buffer, nullptr); t.add_granular_voice_from_buffer(0, buffer, &gp);
  t.add_voice_from_buffer(mixer, buffer, nullptr);
  t.shard_of_mixer(mixer); t.remove_mixer(mixer); t.mixer_audio_level(mixer); t.move_effect(0, mixer, PG_MOVE_END, 0); t.move_effect(fx, 0, PG_MOVE_START, 0); t.move_effect(fx, mixer, PG_MOVE_START, 0);
  t.remove_effect(fx); t.schedule_param(fx, fx_param(0), 0.5f, 1, pos); t.schedule_reset(fx, pos);
  t.feed_voice(voice, 16); t.end_stream_voice(voice); t.stream_voice_consumed(voice);
  t.set_voice_volume(voice, 0.5f, pos); t.set_voice_panning(voice, 0.5f, pos); t.set_voice_speed(voice, 1.5, 0.0f, pos); t.seek_voice(voice, 0.001, pos); t.stop_voice(voice, pos);
  t.remove_voice(voice); t.is_voice_playing(voice); t.set_voice_envelope(voice, &ap); t.release_voice(voice, pos); t.voice_envelope_stage(voice); t.voice_grain_state(voice);
  t.set_voice_granular_parameter(voice, grain_param(2), 0.5f, 1, pos); t.set_voice_grain_loop_range(voice, 1, 0.1f, 0.9f, pos); t.voice_granular_params(voice);
  t.set_voice_modulation_matrix(voice, &mp); t.set_voice_modulation(voice, 0, 0, 0.5f, 1, pos); t.clear_voice_modulation(voice, 0, 0, pos); t.set_voice_lfo_rate(voice, 0, 2.0f, pos);
  t.set_voice_lfo_waveform(voice, 1, 3, pos); t.voice_modulation_state(voice); t.set_voice_status(voice, 0.01, 1);
  t.release_sample_buffer(buffer); t.prepare_granular_buffer(buffer); t.sample_buffer_info(buffer); t.read_granular_buffer(buffer, -1, 16);
}

static void scripted(Tr& t, int n_shards) {
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  pg_ahdsr_params ap;
  pg_ahdsr_params_default(&ap);
  pg_modulation_params mp;
  pg_modulation_params_default(&mp);
  mp.routes[0][0].amount = 0.5f;
  pg_voice_options late;
  pg_voice_options_default(&late);
  late.start_time = 100000;
  uint64_t pos = 0;
  argument_errors(t);
  quiet("shard_count", "", pg_sharded_shard_count(t.s));
  quiet("reduce_mode", "", pg_sharded_reduce_mode(t.s));
  // metering off, then on; status twice
  t.mixer_audio_level(0); t.mixer_audio_level(1); t.mixer_audio_level(99);
  t.set_metering(0.01);
  t.mixer_audio_level(0); t.mixer_audio_level(1);
  t.poll_status(8); t.status_dropped();
  t.enable_status(64); t.enable_status(64);
  // nested sub-mixers: top-level ones spread over the shards, nested ones live with their parents
  const int m1 = t.add_mixer(), m2 = t.add_mixer(), m3 = t.add_mixer_to(0), m4 = t.add_mixer();
  const int n1 = t.add_mixer_to(m1), n2 = t.add_mixer_to(m2), nn = t.add_mixer_to(n2);
  t.mixer_audio_level(m2); t.mixer_audio_level(nn);
  // effects on mixer 0 (the root's bus chain, no load) and on sub-mixers
  const int e0 = t.add_effect(0, 0), e1 = t.add_effect(m1, 1), e2 = t.add_effect(m2, 2), e3 = t.add_effect(nn, 5), e4 = t.add_effect(0, 4), e5 = t.add_effect(m1, 0);
  t.add_effect(m1, 99);
  // sample buffers: stereo with a loop at another rate, mono at the graph's rate
  const pg_sample_buffer_desc ds = desc(2, 44100, true, 100, 1900), dm = desc(1, 48000, false);
  const int bs = t.add_sample_buffer(t.pcm.data(), 2001, &ds), bm = t.add_sample_buffer(t.pcm.data(), 777, &dm), bx = t.add_sample_buffer(t.pcm.data(), 300, &dm);
  t.sample_buffer_info(bs); t.sample_buffer_info(bm);
  t.prepare_granular_buffer(bm);   // (reached no shard yet: converted on the root)
  t.sample_buffer_info(bm);
  // every kind of voice, on mixer 0 and on sub-mixers
  const int vf0 = t.add_voice(0, 500, 1, 48000, nullptr), vf1 = t.add_voice(m1, 900, 2, 44100, nullptr), vf2 = t.add_voice(nn, 300, 1, 22050, &late), vf3 = t.add_voice(0, 64, 2, 48000, nullptr);
  const int vs0 = t.add_stream_voice(0, 2, 48000, 2048), vs1 = t.add_stream_voice(m3, 1, 44100, 1024);
  const int vg0 = t.add_granular_voice(0, 1000, &gp), vg1 = t.add_granular_voice(n1, 400, &gp);
  const int vb0 = t.add_voice_from_buffer(0, bs, nullptr), vb1 = t.add_voice_from_buffer(m2, bs, &late), vb2 = t.add_voice_from_buffer(m4, bm, nullptr), vb3 = t.add_voice_from_buffer(0, bs, nullptr);
  const int vgb0 = t.add_granular_voice_from_buffer(0, bs, &gp), vgb1 = t.add_granular_voice_from_buffer(m1, bm, &gp), vgb2 = t.add_granular_voice_from_buffer(m3, bs, &gp);
  t.add_voice(0, 0, 1, 48000, nullptr); t.add_voice(0, 100, 3, 48000, nullptr); t.add_stream_voice(0, 5, 48000, 1024);
  t.sample_buffer_info(bs); t.sample_buffer_info(bm); t.sample_buffer_info(bx);
  t.prepare_granular_buffer(bs); t.sample_buffer_info(bs);
  for (int sh = -2; sh <= n_shards; ++sh) t.read_granular_buffer(bs, sh, 8);
  t.read_granular_buffer(bx, -1, 0, false);
  // set-up calls that only work before the first render
  t.set_voice_envelope(vf0, &ap); t.set_voice_envelope(vg1, &ap); t.set_voice_envelope(vs0, &ap);
  t.set_voice_modulation_matrix(vg0, &mp); t.set_voice_modulation_matrix(vgb1, &mp); t.set_voice_modulation_matrix(vf0, &mp);
  t.set_voice_status(vf0, 0.001, 1); t.set_voice_status(vb1, -1.0, 1); t.set_voice_status(vgb0, 0.002, 0); t.set_voice_status(vs0, 0.001, 1); t.set_voice_status(vf1, 0.001, 1);
  // ids of the wrong kind
  t.voice_grain_state(vf0); t.voice_granular_params(vs0); t.voice_modulation_state(vb0); t.set_voice_granular_parameter(vf1, grain_param(2), 0.5f, 1, 0);
  t.set_voice_grain_loop_range(vs1, 1, 0.1f, 0.9f, 0); t.set_voice_modulation(vf0, 0, 0, 0.5f, 0, 0); t.set_voice_modulation(vg1, 0, 0, 0.5f, 0, 0);
  t.set_voice_lfo_rate(vb2, 0, 2.0f, 0); t.set_voice_lfo_waveform(vs0, 0, 1, 0); t.clear_voice_modulation(vf3, 0, 0, 0);
  t.seek_voice(vs0, 0.01, 0); t.seek_voice(vg0, 0.01, 0); t.feed_voice(vf0, 16); t.end_stream_voice(vg0); t.stream_voice_consumed(vb0); t.set_voice_speed(vs1, 2.0, 0.0f, 0);
  t.move_effect(e1, m2, PG_MOVE_START, 0); t.move_effect(e3, m1, PG_MOVE_END, 0); t.move_effect(e0, m1, PG_MOVE_END, 0); t.move_effect(e2, 0, PG_MOVE_START, 0);
  t.move_effect(e5, m1, PG_MOVE_START, 0); t.move_effect(e4, 0, PG_MOVE_DIRECTION, -1); t.move_effect(e3, n2, PG_MOVE_END, 0); t.move_effect(e1, m1, 7, 0);
  // the working calls on ids of the right kind
  t.feed_voice(vs0, 600); t.feed_voice(vs1, 2000); t.feed_voice(vs1, 100); t.stream_voice_consumed(vs0);
  t.schedule_param(e0, fx_param(0), 0.5f, 1, 32); t.schedule_param(e2, fx_param(2), 0.25f, 1, 100); t.schedule_param(e2, 0x01020304u, 0.25f, 1, 100); t.schedule_reset(e3, 40);
  t.set_voice_volume(vf0, 0.5f, 10); t.set_voice_panning(vf1, -0.5f, 70); t.set_voice_speed(vf1, 1.5, 12.0f, 90); t.seek_voice(vb0, 0.002, 50); t.set_voice_speed(vf0, -1.0, 0.0f, 0);
  t.set_voice_modulation(vg0, 1, 2, 0.25f, 1, 20); t.clear_voice_modulation(vg0, 0, 0, 30); t.set_voice_lfo_rate(vgb1, 1, 50.0f, 0); t.set_voice_lfo_waveform(vg0, 0, 6, 60);
  t.set_voice_granular_parameter(vg0, grain_param(2), 0.75f, 1, 16); t.set_voice_granular_parameter(vgb2, grain_param(0), 5.0f, 0, 16); t.set_voice_grain_loop_range(vg1, 1, 0.25f, 0.75f, 48);
  t.set_voice_grain_loop_range(vgb0, 0, 0.0f, 0.0f, 0);
  t.voice_envelope_stage(vf0); t.voice_envelope_stage(vf1); t.voice_grain_state(vg0); t.voice_granular_params(vgb2); t.voice_modulation_state(vg0); t.voice_modulation_state(vg1);
  for (int v : {vf0, vf2, vs0, vg0, vb1, vgb2}) t.is_voice_playing(v);
  // short writes: "already rendered" is reached
  pos += t.write(64, pos) / 2;
  t.poll_status(64); t.status_dropped();
  t.mixer_audio_level(0); t.mixer_audio_level(m1); t.mixer_audio_level(nn);
  t.set_voice_envelope(vf0, &ap); t.set_voice_envelope(vf2, &ap); t.set_voice_modulation_matrix(vg1, &mp); t.set_voice_status(vf1, 0.001, 1); t.set_voice_status(vf2, 0.001, 1);
  t.enable_status(16);
  pos += t.write(333, pos) / 2;
  t.poll_status(3); t.poll_status(0, false); t.poll_status(4, false); t.poll_status(64);
  t.stream_voice_consumed(vs0); t.stream_voice_consumed(vs1); t.end_stream_voice(vs1); t.feed_voice(vs1, 10);
  t.release_voice(vf0, pos + 10); t.release_voice(vg1, pos); t.release_voice(vf1, pos + 5); t.stop_voice(vb0, pos + 20); t.stop_voice(vf3, 0);
  pos += t.write(64, pos) / 2;
  for (int v : {vf0, vf1, vf3, vb0, vg1}) { t.is_voice_playing(v); t.voice_envelope_stage(v); }
  // buffers released while in use, and twice; voices and mixers leave
  t.release_sample_buffer(bs); t.sample_buffer_info(bs); t.release_sample_buffer(bs); t.add_voice_from_buffer(0, bs, nullptr); t.prepare_granular_buffer(bs); t.read_granular_buffer(bs, -1, 8);
  t.release_sample_buffer(bx); t.release_sample_buffer(bx);
  t.set_voice_volume(vb3, 0.25f, pos); t.voice_granular_params(vgb0);
  t.remove_voice(vb3); t.remove_voice(vb3); t.remove_voice(vg0); t.remove_effect(e1); t.remove_effect(e1); t.remove_effect(e4);
  pos += t.write(64, pos) / 2;
  t.remove_mixer(0); t.remove_mixer(n2); t.remove_mixer(n2); t.remove_mixer(m4); t.remove_mixer(m4);
  const int m5 = t.add_mixer(), m6 = t.add_mixer();   // (the shard that lost m4 has room again)
  t.sample_buffer_info(bm);
  t.add_mixer_to(n2); t.add_mixer_to(nn); t.add_effect(m4, 0); t.add_voice(n2, 100, 1, 48000, nullptr); t.add_voice_from_buffer(m4, bm, nullptr);
  t.add_granular_voice_from_buffer(m5, bm, &gp); t.add_voice(m6, 200, 1, 48000, nullptr);
  // removed ids (voice, effect, mixer, buffer), negative ones, one past the end
  bad_ids(t, vb3, e1, m4, bx, pos);
  bad_ids(t, -1, -1, -1, -1, pos);
  bad_ids(t, 1000, 1000, 1000, 1000, pos);
  t.move_effect(e3, nn, PG_MOVE_START, 0); t.schedule_param(e3, fx_param(5), 0.5f, 1, pos); t.mixer_audio_level(nn); t.mixer_audio_level(m4);
  pos += t.write(333, pos) / 2;
  t.set_metering(-1.0); t.mixer_audio_level(0); t.mixer_audio_level(m1); t.mixer_audio_level(-1);
  t.stop_all_voices();
  pos += t.write(64, pos) / 2;
  for (int v : {vf1, vs0, vgb0, vgb2}) t.is_voice_playing(v);
  t.poll_status(64); t.status_dropped();
}

static void random_part(Tr& t, uint64_t seed, int steps) {
  Rng r(seed);
  std::vector<int> mixers(1, 0), fx, voices, buffers;   // (removed ids stay listed: calls on them must fail the same way)
  pg_granular_params gp;
  pg_granular_params_default(&gp);
  pg_ahdsr_params ap;
  pg_ahdsr_params_default(&ap);
  pg_modulation_params mp;
  pg_modulation_params_default(&mp);
  uint64_t pos = 100000;
  auto any = [&](std::vector<int>& ids) { const int k = r.below((int)ids.size() + 2); return k < (int)ids.size() ? ids[(size_t)k] : (k == (int)ids.size() ? -1 : (int)ids.size() + 50); };
  for (int step = 0; step < steps; ++step) {
    const uint64_t when = pos + (uint64_t)r.below(400);
    switch (r.below(30)) {
      case 0: case 1: if (mixers.size() < 14) { const int m = r.below(2) ? t.add_mixer_to(r.below(2) ? 0 : any(mixers)) : t.add_mixer(); if (m > 0) mixers.push_back(m); } break;
      case 2: if (r.below(2)) t.remove_mixer(any(mixers)); break;
      case 3: case 4: if (fx.size() < 24) { const int e = t.add_effect(any(mixers), r.below(10)); if (e >= 0) fx.push_back(e); } break;
      case 5: t.remove_effect(any(fx)); break;
      case 6: t.move_effect(any(fx), any(mixers), r.below(3), r.below(5) - 2); break;
      case 7: case 8: if (voices.size() < 60) {
        pg_voice_options o;
        pg_voice_options_default(&o);
        o.start_time = r.below(2) ? 0 : when;
        const int v = t.add_voice(any(mixers), (size_t)(16 + r.below(1500)), 1 + (uint32_t)r.below(2), r.below(2) ? 48000u : 44100u, &o);
        if (v >= 0) voices.push_back(v);
      } break;
      case 9: if (voices.size() < 60) { const int v = t.add_stream_voice(any(mixers), 1 + (uint32_t)r.below(2), 48000, 1024); if (v >= 0) voices.push_back(v); } break;
      case 10: if (voices.size() < 60) { gp.size = 1.0f + (float)r.below(300); const int v = t.add_granular_voice(any(mixers), (size_t)(16 + r.below(1500)), &gp); if (v >= 0) voices.push_back(v); } break;
      case 11: if (buffers.size() < 6) {
        const uint32_t ch = 1 + (uint32_t)r.below(2);
        const pg_sample_buffer_desc d = desc(ch, r.below(2) ? 48000u : 32000u, r.below(2) != 0, 10, 200);
        const int b = t.add_sample_buffer(t.pcm.data(), (size_t)(300 + r.below(1200)), &d);
        if (b >= 0) buffers.push_back(b);
      } break;
      case 12: if (voices.size() < 60) { const int v = t.add_voice_from_buffer(any(mixers), any(buffers), nullptr); if (v >= 0) voices.push_back(v); } break;
      case 13: if (voices.size() < 60) { gp.size = 1.0f + (float)r.below(300); const int v = t.add_granular_voice_from_buffer(any(mixers), any(buffers), &gp); if (v >= 0) voices.push_back(v); } break;
      case 14: switch (r.below(4)) {
        case 0: if (r.below(3) == 0) t.release_sample_buffer(any(buffers)); break;
        case 1: t.prepare_granular_buffer(any(buffers)); break;
        case 2: t.sample_buffer_info(any(buffers)); break;
        default: t.read_granular_buffer(any(buffers), r.below(5) - 1, 4); break;
      } break;
      case 15: { const int v = any(voices); if (r.below(2)) t.feed_voice(v, (size_t)r.below(600)); else if (r.below(4) == 0) t.end_stream_voice(v); else t.stream_voice_consumed(v); } break;
      case 16: if (r.below(2)) t.schedule_param(any(fx), fx_param(r.below(10)), r.unit(), 1, when); else t.schedule_reset(any(fx), when); break;
      case 17: if (r.below(2)) t.set_voice_volume(any(voices), r.unit(), when); else t.set_voice_panning(any(voices), 2.0f * r.unit() - 1.0f, when); break;
      case 18: if (r.below(2)) t.set_voice_speed(any(voices), 0.5 + (double)r.below(4), r.below(2) ? 12.0f : 0.0f, when); else t.seek_voice(any(voices), 0.001 * r.below(10), when); break;
      case 19: { const int v = any(voices); if (r.below(3)) t.stop_voice(v, when); else t.remove_voice(v); t.is_voice_playing(v); } break;
      case 20: { const int v = any(voices); if (r.below(2)) t.set_voice_envelope(v, &ap); else t.release_voice(v, when); t.voice_envelope_stage(v); } break;
      case 21: { const int v = any(voices); mp.velocity = 0.25f * (float)r.below(5); if (r.below(2)) t.set_voice_modulation_matrix(v, &mp); else t.voice_modulation_state(v); } break;
      case 22: { const int v = any(voices);
        switch (r.below(4)) {
          case 0: t.set_voice_modulation(v, r.below(5), r.below(8), 0.25f * (float)(r.below(10) - 5), r.below(2), when); break;
          case 1: t.clear_voice_modulation(v, r.below(5), r.below(8), when); break;
          case 2: t.set_voice_lfo_rate(v, r.below(3), 0.5f * (float)r.below(50), when); break;
          default: t.set_voice_lfo_waveform(v, r.below(3), r.below(8), when); break;
        } } break;
      case 23: { const int v = any(voices);
        switch (r.below(4)) {
          case 0: t.set_voice_granular_parameter(v, r.below(8) ? grain_param(r.below(10)) : 0x41424344u, 0.125f * (float)r.below(9), r.below(2), when); break;
          case 1: t.set_voice_grain_loop_range(v, r.below(2), 0.125f * (float)r.below(10), 0.125f * (float)r.below(10), when); break;
          case 2: t.voice_granular_params(v); break;
          default: t.voice_grain_state(v); break;
        } } break;
      case 24: if (r.below(2)) t.set_voice_status(any(voices), r.below(3) ? 0.001 * r.below(20) : -1.0, r.below(2)); else t.mixer_audio_level(any(mixers)); break;
      case 25: switch (r.below(8)) {
        case 0: t.set_metering(r.below(2) ? 0.005 * r.below(4) : -1.0); break;
        case 1: t.stop_all_voices(); break;
        case 2: t.enable_status(32); break;
        case 3: t.shard_of_mixer(any(mixers)); break;
        default: t.poll_status((size_t)r.below(16)); t.status_dropped(); break;
      } break;
      default: { const size_t n = r.below(3) ? 64 : 333; t.write(n, pos); pos += n; } break;
    }
  }
}

// ---- null handles -------------------------------------------------------------------------------------------------------------------
enum Way { STATUS, NEGATIVE, QUIET_MINUS_ONE, QUIET_ZERO, NOTHING };   // how the entry point says PG_ERR_PARAMETER
struct NullCall { const char* name; Way way; bool golden; long long (*call)(Tr&); };

static const NullCall NULL_CALLS[] = {
#define NC(name, way, golden, expr) {#name, way, golden, [](Tr& t) -> long long { (void)t; return (long long)(expr); }}
  NC(destroy, NOTHING, true, (pg_sharded_destroy(nullptr), 0)),
  NC(shard_count, NEGATIVE, false, pg_sharded_shard_count(nullptr)),
  NC(set_max_blocks_per_launch, STATUS, false, pg_sharded_set_max_blocks_per_launch(nullptr, 2)),
  NC(set_reduce, STATUS, false, pg_sharded_set_reduce(nullptr, PG_REDUCE_PEER_COPY)),
  NC(reduce_mode, NEGATIVE, false, pg_sharded_reduce_mode(nullptr)),
  NC(add_mixer, NEGATIVE, false, pg_sharded_add_mixer(nullptr)),
  NC(add_mixer_to, NEGATIVE, false, pg_sharded_add_mixer_to(nullptr, 0)),
  NC(add_effect, NEGATIVE, false, pg_sharded_add_effect(nullptr, 0, 0, nullptr)),
  NC(add_voice, NEGATIVE, false, pg_sharded_add_voice(nullptr, 0, t.pcm.data(), 100, 1, 48000, nullptr)),
  NC(add_stream_voice, NEGATIVE, false, pg_sharded_add_stream_voice(nullptr, 0, 2, 48000, 1024, nullptr)),
  NC(feed_voice, STATUS, false, pg_sharded_feed_voice(nullptr, 0, t.pcm.data(), 16)),
  NC(end_stream_voice, STATUS, false, pg_sharded_end_stream_voice(nullptr, 0)),
  NC(stream_voice_consumed, NEGATIVE, false, pg_sharded_stream_voice_consumed(nullptr, 0)),
  NC(shard_of_mixer, NEGATIVE, false, pg_sharded_shard_of_mixer(nullptr, 0)),
  NC(remove_mixer, STATUS, false, pg_sharded_remove_mixer(nullptr, 1)),
  NC(remove_effect, STATUS, false, pg_sharded_remove_effect(nullptr, 0)),
  NC(move_effect, STATUS, false, pg_sharded_move_effect(nullptr, 0, 0, PG_MOVE_START, 0)),
  NC(schedule_param, STATUS, false, pg_sharded_schedule_param(nullptr, 0, fx_param(0), 0.5f, 1, 0)),
  NC(schedule_reset, STATUS, false, pg_sharded_schedule_reset(nullptr, 0, 0)),
  NC(set_voice_volume, STATUS, false, pg_sharded_set_voice_volume(nullptr, 0, 0.5f, 0)),
  NC(set_voice_panning, STATUS, false, pg_sharded_set_voice_panning(nullptr, 0, 0.5f, 0)),
  NC(set_voice_speed, STATUS, false, pg_sharded_set_voice_speed(nullptr, 0, 1.5, 0.0f, 0)),
  NC(seek_voice, STATUS, false, pg_sharded_seek_voice(nullptr, 0, 0.01, 0)),
  NC(stop_voice, STATUS, false, pg_sharded_stop_voice(nullptr, 0, 0)),
  NC(stop_all_voices, STATUS, false, pg_sharded_stop_all_voices(nullptr)),
  NC(remove_voice, STATUS, false, pg_sharded_remove_voice(nullptr, 0)),
  NC(is_voice_playing, QUIET_ZERO, false, pg_sharded_is_voice_playing(nullptr, 0)),
  NC(set_voice_envelope, STATUS, true, [] { pg_ahdsr_params p; pg_ahdsr_params_default(&p); return pg_sharded_set_voice_envelope(nullptr, 0, &p); }()),
  NC(release_voice, STATUS, true, pg_sharded_release_voice(nullptr, 0, 0)),
  NC(voice_envelope_stage, QUIET_MINUS_ONE, true, pg_sharded_voice_envelope_stage(nullptr, 0)),
  NC(add_granular_voice, NEGATIVE, true, [&] { pg_granular_params p; pg_granular_params_default(&p); return pg_sharded_add_granular_voice(nullptr, 0, t.pcm.data(), 100, &p, nullptr); }()),
  NC(voice_grain_state, STATUS, true, pg_sharded_voice_grain_state(nullptr, 0, &t.grain)),
  NC(set_voice_granular_parameter, STATUS, true, pg_sharded_set_voice_granular_parameter(nullptr, 0, grain_param(2), 0.5f, 1, 0)),
  NC(set_voice_grain_loop_range, STATUS, true, pg_sharded_set_voice_grain_loop_range(nullptr, 0, 1, 0.25f, 0.75f, 0)),
  NC(voice_granular_params, STATUS, true, [] { pg_granular_params p; return pg_sharded_voice_granular_params(nullptr, 0, &p); }()),
  NC(add_sample_buffer, NEGATIVE, true, [&] { const pg_sample_buffer_desc d = desc(1, 48000, false); return pg_sharded_add_sample_buffer(nullptr, t.pcm.data(), 100, &d); }()),
  NC(release_sample_buffer, STATUS, true, pg_sharded_release_sample_buffer(nullptr, 0)),
  NC(add_voice_from_buffer, NEGATIVE, true, pg_sharded_add_voice_from_buffer(nullptr, 0, 0, nullptr)),
  NC(add_granular_voice_from_buffer, NEGATIVE, true, [] { pg_granular_params p; pg_granular_params_default(&p); return pg_sharded_add_granular_voice_from_buffer(nullptr, 0, 0, &p, nullptr); }()),
  NC(prepare_granular_buffer, STATUS, true, pg_sharded_prepare_granular_buffer(nullptr, 0)),
  NC(sample_buffer_info, STATUS, true, [] { pg_sample_buffer_info i; return pg_sharded_sample_buffer_info(nullptr, 0, &i); }()),
  NC(read_granular_buffer, NEGATIVE, true, pg_sharded_read_granular_buffer(nullptr, 0, -1, t.out.data(), 4)),
  NC(set_voice_modulation_matrix, STATUS, true, [] { pg_modulation_params p; pg_modulation_params_default(&p); return pg_sharded_set_voice_modulation_matrix(nullptr, 0, &p); }()),
  NC(set_voice_modulation, STATUS, true, pg_sharded_set_voice_modulation(nullptr, 0, 0, 0, 0.5f, 0, 0)),
  NC(clear_voice_modulation, STATUS, true, pg_sharded_clear_voice_modulation(nullptr, 0, 0, 0, 0)),
  NC(set_voice_lfo_rate, STATUS, true, pg_sharded_set_voice_lfo_rate(nullptr, 0, 0, 2.0f, 0)),
  NC(set_voice_lfo_waveform, STATUS, true, pg_sharded_set_voice_lfo_waveform(nullptr, 0, 0, 1, 0)),
  NC(voice_modulation_state, STATUS, true, [] { pg_modulation_state m; return pg_sharded_voice_modulation_state(nullptr, 0, &m); }()),
  NC(set_metering, STATUS, true, pg_sharded_set_metering(nullptr, 0.01)),
  NC(mixer_audio_level, STATUS, true, [] { pg_audio_level l; return pg_sharded_mixer_audio_level(nullptr, 0, &l); }()),
  NC(enable_status, STATUS, true, pg_sharded_enable_status(nullptr, 16)),
  NC(set_voice_status, STATUS, true, pg_sharded_set_voice_status(nullptr, 0, 0.01, 1)),
  NC(poll_status, QUIET_ZERO, true, [] { pg_status_event e[2]; return pg_sharded_poll_status(nullptr, e, 2); }()),
  NC(status_dropped, QUIET_ZERO, true, pg_sharded_status_dropped(nullptr)),
  NC(write, QUIET_ZERO, false, pg_sharded_write(nullptr, t.out.data(), 128, 0)),
  NC(write_device, QUIET_ZERO, false, pg_sharded_write_device(nullptr, t.out.data(), 128, 0)),
  NC(synchronize, STATUS, false, pg_sharded_synchronize(nullptr)),
  NC(device_errors, NEGATIVE, false, pg_sharded_device_errors(nullptr)),
#undef NC
};

static int null_handles(Tr& t, bool record) {
  int asserted = 0;
  for (const NullCall& c : NULL_CALLS) {
    if (record && !c.golden) continue;   // (the tree the transcript was recorded from dereferenced the handle in these)
    const long long rc = c.call(t);
    const bool says = c.way == STATUS || c.way == NEGATIVE;
    if (c.golden) { printf("null pg_sharded_%s -> %lld", c.name, rc); if (says) printf(" | %s", pg_last_error_message()); putchar('\n'); continue; }
    const long long want = c.way == STATUS ? PG_ERR_PARAMETER : c.way == NEGATIVE ? -PG_ERR_PARAMETER : c.way == QUIET_MINUS_ONE ? -1 : 0;
    if (rc != want || (says && !strstr(pg_last_error_message(), "null"))) {
      fprintf(stderr, "pg_sharded_%s on a null handle returned %lld (expected %lld), message \"%s\"\n", c.name, rc, want, pg_last_error_message());
      exit(1);
    }
    ++asserted;
  }
  return asserted;
}

int main(int argc, char** argv) {
  const bool record = argc > 1 && strcmp(argv[1], "record") == 0;
  Tr t;
  printf("== null handle\n");
  argument_errors(t);
  const int asserted = null_handles(t, record);
  static const int DEVICES[3] = {0, 1, 1};   // (a device may be listed more than once)
  for (int n = 1; n <= 3; ++n) {
    printf("== %d shard(s)\n", n);
    t.s = pg_sharded_create(48000, 2, 64, DEVICES, n);
    t.n_buffers = 0;
    if (!t.s) { fprintf(stderr, "create failed: %s\n", pg_last_error_message()); return 2; }
    scripted(t, n);
    printf("-- random\n");
    random_part(t, 77 + (uint64_t)n, 420);
    pg_sharded_destroy(t.s);
    t.s = nullptr;
  }
  fflush(stdout);
  if (!record) printf("null handle rule asserted for %d entry points\n", asserted);
  return 0;
}
