"""Independent restatement of the reference's playback status events (PlaybackStatusEvent::Position / ::Stopped, src/source/status.rs):
what sends them — FileSourceImpl (src/source/file/common.rs:171-221), PreloadedFileSource (src/source/file/preloaded.rs:196-239, :270-332,
:396-475), SamplerVoice::process (src/generator/sampler/voice.rs:434-502) — and the grid of Source::write calls a MixedSource makes
(src/source/mixed.rs:558-624, :659-719). Integers, f32 and f64 only: every record is compared for equality.

Events are tuples: ("position", voice, sample_time, frame_pos, position_seconds) / ("stopped", voice, sample_time, exhausted)."""
import numpy as np

F32 = np.float32
U64_MAX = (1 << 64) - 1
MAX_MIX_FRAMES = 4096          # MixedSource::MAX_MIX_BUFFER_SAMPLES / 2 (mixed.rs:216)
SECOND_STOPPED_OF_A_GRANULAR_VOICE = False
# voice.rs:488-502 sends { exhausted: pool.is_exhausted() } AFTER SamplerVoice::reset -> GrainPool::reset (granular.rs:495-502), which sets
# trigger_new_grains = true; is_exhausted = !trigger_new_grains && no active grain (granular.rs:442-444): always false there.


def duration_to_sample_time(seconds, sample_rate):
    """SampleTimeClock::duration_to_sample_time (src/utils/time.rs:28-35): (secs * rate as f64) as u64, the cast saturating."""
    f = float(seconds) * float(sample_rate)
    if not f > 0.0:
        return 0
    return U64_MAX if f >= 18446744073709551615.0 else int(f)


class Sender:
    """FileSourceImpl's status part: playback_pos_emit_rate, playback_pos_sample_time_clock, the two send functions (common.rs:171-221)."""

    def __init__(self, voice, out_rate, emit_seconds, report_stopped, channels, rate, sink):
        self.voice, self.channels, self.rate, self.sink = voice, channels, rate, sink
        self.emit_rate = None if emit_seconds is None or not emit_seconds > 0 else duration_to_sample_time(emit_seconds, out_rate)
        self.report_stopped = report_stopped
        self.clock_start = 0   # SampleTimeClock::new: start_time 0 (time.rs:19-26)

    def position(self, time, is_start_event, sample_pos):
        if self.emit_rate is None:
            return
        if is_start_event or max(time - self.clock_start, 0) >= self.emit_rate:   # elapsed: saturating_sub
            self.clock_start = time
            frame_pos = int(sample_pos) // self.channels
            self.sink.append(("position", self.voice, time, frame_pos, float(frame_pos) / float(self.rate)))

    def stopped(self, time, exhausted):
        if self.report_stopped:
            self.sink.append(("stopped", self.voice, time, bool(exhausted)))


class Cubic:
    """How many input frames CubicInterpolator::process consumes for how many output frames (src/utils/resampler/cubic.rs:36-114): the f32
    sub_pos recurrence; the samples themselves do not matter."""

    def __init__(self, ratio):
        self.ratio, self.sub_pos, self.initialized = F32(ratio), F32(0.0), False

    def reset(self):
        self.sub_pos, self.initialized = F32(0.0), False

    def process(self, num_in, num_out):
        one = F32(1.0)
        if abs(F32(self.ratio - one)) < F32(0.000001):
            m = min(num_in, num_out)
            return m, m
        consumed = produced = 0
        if not self.initialized and num_in >= 3:
            self.initialized = True
            consumed = 3
        if self.ratio < one:
            while produced < num_out:
                if self.sub_pos >= one:
                    if consumed >= num_in:
                        break
                    consumed += 1
                    self.sub_pos = F32(self.sub_pos - one)
                produced += 1
                self.sub_pos = F32(self.sub_pos + self.ratio)
        else:
            done = False
            while produced < num_out and not done:
                while self.sub_pos < self.ratio:
                    if consumed >= num_in:
                        done = True
                        break
                    consumed += 1
                    self.sub_pos = F32(self.sub_pos + one)
                if done:
                    break
                self.sub_pos = F32(self.sub_pos - self.ratio)
                produced += 1
        return consumed, produced


class FileSource:
    """PreloadedFileSource as far as its status events go: playback_pos, the loop, the end of the file, the fader's arrival, stop / kill / seek /
    set_speed (no glide). n_frames counts the buffer's frames (the extra zero frame included, as the device gets it)."""

    def __init__(self, sender, n_frames, channels, file_rate, out_rate, speed=1.0, repeat=0, loop_range=None, fade_out_seconds=0.05):
        self.s, self.n_samples, self.channels, self.file_rate, self.out_rate = sender, n_frames * channels, channels, file_rate, out_rate
        self.playback_pos, self.repeat, self.repeat_count = 0, repeat, repeat
        self.loop_range = loop_range
        self.eof = self.finished = False
        self.fade_out_seconds = fade_out_seconds
        self.fader_running, self.fader_finished, self.fader_cur, self.fader_tgt, self.fader_inertia = False, False, F32(1.0), F32(1.0), F32(1.0)
        self.cubic = Cubic(self._ratio(speed))

    def _ratio(self, speed):   # FileSourceImpl::new / update_speed: (out_rate as f64 / speed) as u32; ratio = (in / out as f64) as f32 (cubic.rs:164)
        return F32(float(self.file_rate) / float(int(float(self.out_rate) / speed)))

    def is_exhausted(self):
        return self.finished

    def stop(self):   # preloaded.rs:196-208 (the status of a stop without a fade-out carries the time of the write that processes the message)
        self._stop_pending = True

    def set_speed(self, speed):   # preloaded.rs:181-192, glide None
        if not self.finished:
            self.cubic.ratio = self._ratio(speed)

    def seek(self, seconds):   # preloaded.rs:139-147
        if not self.finished:
            self.playback_pos = min(int(seconds * float(self.file_rate) * float(self.channels)), self.n_samples)
            self.cubic.reset()

    def kill(self, time):   # preloaded.rs:232-239
        if not self.finished:
            self.s.stopped(time, self.eof)
            self.finished = True

    _stop_pending = False

    def _write_buffer(self, frames):   # preloaded.rs:270-332
        c = self.channels
        if self.repeat > 0 and self.loop_range is not None:
            lo, hi = self.loop_range[0] * c, self.loop_range[1] * c
        else:
            lo, hi = 0, self.n_samples
        written = 0
        while written < frames:
            remaining_in = max(hi - self.playback_pos, 0) // c
            consumed, produced = self.cubic.process(remaining_in, frames - written)
            self.playback_pos += consumed * c
            written += produced
            if self.playback_pos >= hi:
                if self.repeat_count > 0:
                    if self.repeat_count != U64_MAX:
                        self.repeat_count -= 1
                    self.playback_pos = lo
                else:
                    self.eof = True
            if self.eof and produced == 0:
                break
        return written

    def write(self, frames, time):   # preloaded.rs:396-475
        if self._stop_pending:   # process_messages -> stop()
            self._stop_pending = False
            if not self.finished:
                if self.fade_out_seconds is not None and self.fade_out_seconds > 0:
                    frm = self.fader_cur if self.fader_running else F32(1.0)   # VolumeFader::start_fade_out (fader.rs:67-91)
                    self.fader_running, self.fader_finished, self.fader_cur, self.fader_tgt = True, False, frm, F32(0.0)
                    samples_duration = F32(F32(self.out_rate) * F32(self.fade_out_seconds)) / F32(4.605)
                    self.fader_inertia = F32(F32(1.0) - F32(np.exp(np.float64(F32(F32(-1.0) / samples_duration)))))
                else:
                    self.s.stopped(time, self.eof)
                    self.finished = True
        if self.finished:
            return 0
        # playback_started is never true: no start event (docs/parity_findings.md)
        written = self._write_buffer(frames)
        if self.fader_running:   # VolumeFader::process (fader.rs:103-122)
            for _ in range(written):
                self.fader_cur = F32(self.fader_cur + F32(F32(self.fader_tgt - self.fader_cur) * self.fader_inertia))
            if abs(F32(self.fader_cur - self.fader_tgt)) < F32(0.0001):
                self.fader_running, self.fader_finished = False, True
        self.s.position(time, False, self.playback_pos)
        if self.eof or (self.fader_finished and self.fader_tgt == F32(0.0)):
            self.s.stopped(time, self.eof)
            self.finished = True
        return written


class Mapped:
    """ChannelMappedSource in front of a mono file (mapped.rs:61-99): it asks again for what a short write left open, until a write returns nothing."""

    def __init__(self, inner):
        self.inner = inner

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def write(self, frames, time):
        total = 0
        while total < frames:
            w = self.inner.write(frames - total, time + total)
            if w == 0:
                break
            total += w
        return total


class SamplerVoice:
    """SamplerVoice::process's status part (voice.rs:434-502): `envelope` = an object with run() -> stage after one frame (or None), `pool` = a grain
    pool model with process(n), playback_position() and is_exhausted() (or None: the file source plays)."""

    def __init__(self, sender, source=None, envelope_run=None, pool=None, buffer_len=0):
        self.s, self.source, self.envelope_run, self.pool, self.buffer_len = sender, source, envelope_run, pool, buffer_len
        self.started = pool is not None   # grain_pool_started (voice.rs:169)
        self.active = True
        self._stop_at_write = False

    def is_exhausted(self):
        return not self.active

    def stop(self):
        if self.pool is not None:
            self.pool.stop()
        else:
            self.source.stop()

    def write(self, frames, time):
        if not self.active:
            return 0
        if self.pool is not None:
            self.pool.process(frames)
            written = frames
            ph = F32(self.pool.playback_position())
            is_start, self.started = self.started, False
            self.s.position(time, is_start, int(F32(ph * F32(self.buffer_len))))
        else:
            written = self.source.write(frames, time)
        idle = False
        if self.envelope_run is not None:
            idle = self.envelope_run(written)
        if (self.source is not None and self.source.is_exhausted()) or (self.pool is not None and self.pool.is_exhausted()) or idle:
            if self.source is not None:
                self.source.kill(time)   # reset() -> PreloadedFileSource::reset -> kill
            else:
                self.s.stopped(time, False)   # the file source of a granular voice never played: exhausted = pos_eof = false
            if self.pool is not None:
                self.s.stopped(time, SECOND_STOPPED_OF_A_GRANULAR_VOICE)
            self.active = False
        return written


class Playing:
    def __init__(self, source, start_time, transient=True):
        self.source, self.start_time, self.stop_time, self.transient, self.active = source, start_time, None, transient, True


class Mixer:
    """MixedSource::write's walk (mixed.rs:659-719): events cut chunks of at most 4096 frames, sub-mixers are called first, then the sources —
    each gets Source::write calls cut at its start and stop time (process_sources, :558-624)."""

    def __init__(self):
        self.mixers, self.sources, self.events, self._seq = [], [], [], 0

    def add_mixer(self):
        m = Mixer()
        self.mixers.append(m)
        return m

    def add_source(self, source, start_time=0, transient=True):
        ps = Playing(source, start_time, transient)
        i = 0
        while i < len(self.sources) and self.sources[i].start_time < start_time:   # partition_point(|e| e.start_time < sample_time) (mixed.rs:324-329)
            i += 1
        self.sources.insert(i, ps)
        return ps

    def remove_source(self, ps):
        self.sources.remove(ps)

    def add_event(self, time, fn):
        i = len(self.events)
        while i > 0 and self.events[i - 1][0] > time:
            i -= 1
        self.events.insert(i, (time, fn))

    def write(self, frames, time):
        total = 0
        while total < frames:
            now = time + total
            while self.events and self.events[0][0] <= now:
                self.events.pop(0)[1]()
            until_next = self.events[0][0] - now if self.events else U64_MAX
            n = min(frames - total, MAX_MIX_FRAMES, until_next)
            if n > 0:
                for m in self.mixers:
                    m.write(n, now)
                self._process_sources(n, now)
                total += n
        self.sources = [p for p in self.sources if not (p.transient and not p.active)]
        return frames

    def _process_sources(self, frames, time):
        for ps in self.sources:
            written = 0
            if ps.start_time > time:
                until = ps.start_time - time
                if until >= frames:
                    break   # sorted by start time: nothing behind it starts in this chunk either
                written = until
            while written < frames:
                st = time + written
                until_stop = U64_MAX
                if ps.stop_time is not None:
                    until_stop = max(ps.stop_time - st, 0)
                if until_stop == 0:
                    ps.source.stop()
                    ps.stop_time = None
                    until_stop = U64_MAX
                w = ps.source.write(min(frames - written, until_stop), st)
                written += w
                if ps.transient and ps.source.is_exhausted():
                    ps.active = False
                    break
                if w == 0:
                    break
