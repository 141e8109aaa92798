"""tests/status_model.py on cases worked out by hand from the reference's lines: one per rule of the playback status events."""
import status_model as sm

SR = 48000


def file_voice(sink, n_frames=6001, channels=2, emit=0.05, voice=7, file_rate=SR, **kw):
    s = sm.Sender(voice, SR, emit, True, channels, file_rate, sink)
    return sm.FileSource(s, n_frames, channels, file_rate, SR, **kw)


def test_emit_rate_is_a_truncating_cast():   # time.rs:28-35
    assert sm.duration_to_sample_time(0.05, 48000) == 2400
    assert sm.duration_to_sample_time(1.0 / 3.0, 44100) == 14700   # 14699.999... in f64 rounds to 14700.0 before the cast
    assert sm.duration_to_sample_time(1e-9, 48000) == 0 and sm.duration_to_sample_time(-1.0, 48000) == 0
    assert sm.duration_to_sample_time(1e30, 48000) == sm.U64_MAX


def test_position_after_the_write_when_the_clock_has_run_out():   # common.rs:171-208, preloaded.rs:454-462
    ev = []
    f = file_voice(ev)
    for t in range(0, 6144, 1024):
        f.write(1024, t)
    # elapsed(0) = 0, 1024, 2048 < 2400; elapsed(3072) >= 2400: playback_pos BEHIND that write = 4096 frames, the clock restarts at 3072;
    # elapsed(4096) = 1024, elapsed(5120) = 2048: nothing more; the write at 5120 finds 881 frames: end of file
    assert ev == [("position", 7, 3072, 4096, 4096 / 48000), ("stopped", 7, 5120, True)]


def test_the_call_grid_decides():
    ev = []
    f = file_voice(ev)
    for t in range(0, 6016, 128):
        f.write(128, t)
    assert ev == [("position", 7, 2432, 2560, 2560 / 48000), ("position", 7, 4864, 4992, 4992 / 48000), ("stopped", 7, 5888, True)]


def test_one_long_write_is_two_chunks():   # mixed.rs:679-712: chunks of 4096 frames
    ev = []
    m = sm.Mixer()
    m.add_source(file_voice(ev))
    m.write(8192, 0)
    assert ev == [("position", 7, 4096, 6001, 6001 / 48000), ("stopped", 7, 4096, True)]   # Position stands before Stopped (preloaded.rs:454-472)


def test_no_start_event_for_a_file_voice():   # playback_started is never set (preloaded.rs:405-416)
    ev = []
    f = file_voice(ev)
    f.write(1024, 0)
    assert ev == []
    ev2 = []
    g = file_voice(ev2, emit=1e-9)   # Some(0): elapsed >= 0 holds at every write — the ordinary test, not a start event
    g.write(1024, 0)
    assert ev2 == [("position", 7, 0, 1024, 1024 / 48000)]


def test_emit_none_and_stopped_off():
    ev = []
    s = sm.Sender(1, SR, None, False, 2, SR, ev)
    f = sm.FileSource(s, 101, 2, SR, SR)
    f.write(1024, 0)
    assert ev == [] and f.finished


def test_speed_changes_what_a_write_consumes():   # cubic.rs:60-111: three frames preloaded, then the f32 sub_pos recurrence
    ev = []
    f = file_voice(ev, n_frames=100000, speed=2.0, emit=1e-9)
    f.write(1024, 0)
    g = file_voice(ev, n_frames=100000, speed=0.5, emit=1e-9, voice=8)
    g.write(1024, 0)
    assert ev == [("position", 7, 0, 2051, 2051 / 48000), ("position", 8, 0, 514, 514 / 48000)]


def test_loop_with_repeat_then_end():   # preloaded.rs:273-325
    ev = []
    f = file_voice(ev, n_frames=1001, repeat=2, loop_range=(200, 700), emit=1e-9)
    f.write(1024, 0)    # 0 -> 700, back to 200 (repeat 2 -> 1), 200 + 324 = 524
    f.write(1024, 1024) # 524 -> 700 (176), -> 200 (repeat 1 -> 0), 500 to 700: 676 written, pos 700 >= end, no repeats left: end of file ...
    assert ev[0] == ("position", 7, 0, 524, 524 / 48000)
    assert ev[1:] == [("position", 7, 1024, 700, 700 / 48000), ("stopped", 7, 1024, True)]


def test_seek_moves_the_position():   # preloaded.rs:139-147
    ev = []
    f = file_voice(ev, emit=1e-9)
    f.write(100, 0)
    f.seek(0.0625)      # 3000 frames
    f.write(100, 100)
    assert ev == [("position", 7, 0, 100, 100 / 48000), ("position", 7, 100, 3100, 3100 / 48000)]


def test_stop_without_a_fade_out_at_the_stop_time():   # mixed.rs:584-603, preloaded.rs:196-208
    ev = []
    m = sm.Mixer()
    ps = m.add_source(file_voice(ev, fade_out_seconds=-1.0, emit=1e-9))
    ps.stop_time = 1500
    m.write(4096, 0)
    assert ev == [("position", 7, 0, 1500, 1500 / 48000), ("stopped", 7, 1500, False)]
    assert m.sources == []


def test_stop_with_the_default_fade_out():   # fader.rs:67-122: inertia 1 - exp(-1 / (48000 * 0.05 / 4.605)); |cur| < 1e-4 after 4798 frames
    ev = []
    m = sm.Mixer()
    ps = m.add_source(file_voice(ev, n_frames=100001, emit=None))
    ps.stop_time = 1000
    for t in range(0, 8192, 1024):
        m.write(1024, t)
    # the fade runs from frame 1000; the fader looks at its arrival when a write returns: the write that begins at 5120 ends 5144 frames into the fade
    assert ev == [("stopped", 7, 5120, False)]


def test_an_event_of_the_mixer_is_one_more_source_write():   # mixed.rs:679-712
    ev = []
    m = sm.Mixer()
    sub = m.add_mixer()
    sub.add_source(file_voice(ev, n_frames=100001, emit=0.03125))   # 1500 frames
    sub.add_event(1500, lambda: None)
    m.write(4096, 0)
    assert ev == [("position", 7, 1500, 4096, 4096 / 48000)]   # the write [0, 1500): elapsed 0; the write at 1500: elapsed 1500 >= 1500


def test_envelope_idle_kills_the_source():   # voice.rs:488-495 -> preloaded.rs:212-239
    ev = []
    s = sm.Sender(3, SR, None, True, 2, SR, ev)
    f = sm.FileSource(s, 100001, 2, SR, SR)
    state = {"left": 1500}

    def run(n):
        state["left"] -= n
        return state["left"] <= 0

    v = sm.SamplerVoice(s, source=f, envelope_run=run)
    m = sm.Mixer()
    m.add_source(v)
    m.write(1024, 0)
    m.write(1024, 1024)
    m.write(1024, 2048)
    assert ev == [("stopped", 3, 1024, False)]


class FakePool:
    def __init__(self, positions, dry_after):
        self.positions, self.calls, self.dry_after, self.stopped = positions, 0, dry_after, False

    def process(self, n):
        self.calls += 1

    def playback_position(self):
        return self.positions[min(self.calls - 1, len(self.positions) - 1)]

    def is_exhausted(self):
        return self.calls >= self.dry_after

    def stop(self):
        self.stopped = True


def test_granular_start_event_positions_and_two_stopped():   # voice.rs:449-467, :488-502
    ev = []
    s = sm.Sender(5, SR, 0.05, True, 1, SR, ev)
    v = sm.SamplerVoice(s, pool=FakePool([0.5, 0.25, 0.75, 0.125], dry_after=4), buffer_len=2048)
    for t in range(0, 4096, 1024):
        v.write(1024, t)
    assert ev == [("position", 5, 0, 1024, 1024 / 48000),      # the start event: unconditional, and it restarts the clock at 0
                  ("position", 5, 3072, 256, 256 / 48000),     # elapsed(1024), elapsed(2048) < 2400; (0.125 * 2048.0) as u64
                  ("stopped", 5, 3072, False), ("stopped", 5, 3072, sm.SECOND_STOPPED_OF_A_GRANULAR_VOICE)]
    assert sm.SECOND_STOPPED_OF_A_GRANULAR_VOICE is False


def test_sub_mixers_first_then_sources_in_list_order():   # mixed.rs:324-329, :505-620
    ev = []
    m = sm.Mixer()
    a = m.add_mixer()
    m.add_source(file_voice(ev, voice=1, emit=1e-9, n_frames=100001))
    m.add_source(file_voice(ev, voice=2, emit=1e-9, n_frames=100001))   # same start time: in FRONT of voice 1
    a.add_source(file_voice(ev, voice=3, emit=1e-9, n_frames=100001))
    b = a.add_mixer()
    b.add_source(file_voice(ev, voice=4, emit=1e-9, n_frames=100001))
    m.write(256, 0)
    assert [e[1] for e in ev] == [4, 3, 2, 1]


def test_removed_and_not_yet_started_sources_send_nothing():
    ev = []
    m = sm.Mixer()
    p1 = m.add_source(file_voice(ev, voice=1, emit=1e-9, n_frames=100001))
    m.add_source(file_voice(ev, voice=2, emit=1e-9, n_frames=100001), start_time=5000)
    m.write(1024, 0)
    m.remove_source(p1)   # MixerMessage::RemoveSource: dropped, no kill
    m.write(1024, 1024)
    assert ev == [("position", 1, 0, 1024, 1024 / 48000)]


def test_mono_file_is_asked_again_behind_a_short_write():   # mapped.rs:61-99
    ev = []
    s = sm.Sender(9, SR, 1e-9, True, 1, 44100, ev)
    f = sm.Mapped(sm.FileSource(s, 501, 1, 44100, 44100))
    assert f.write(1024, 0) == 501
    assert ev == [("position", 9, 0, 501, 501 / 44100), ("stopped", 9, 0, True)]
