"""Independent restatement of the reference Sampler's note layer for file playback (src/generator/sampler.rs:656-860, :974-1028, :1076-1120;
src/generator/sampler/voice.rs:122-310, :488-502): timed messages, next_free_voice_index, SamplerVoice::start / stop / reset, the base
parameters, stop / stopping / stopped. Written from the reference, not from the device code.

It composes what the repository already restates: tests/ahdsr_model.py (the envelope, frame by frame) and tests/status_model.py's FileSource
(playback position, end of file, the fader's arrival: when a source write exhausts the file source). Audio is NOT modelled: per note the model
says which slot it got, the frame it started at, the frame at which it was stolen or freed, the speed / volume / panning / stop events it
saw, the smoother values the slot handed down to it and — with an envelope — the gain of every frame; tests render each note from that.

The write grid: the owning sub-mixer is called once per chunk of the main mixer (min(remaining, 4096) frames from the start of a write,
src/source/mixed.rs:216, :679-712) and cuts its own chunk at every message's sample time (:902-918); the sampler's `write` runs once per such
chunk, messages first (process_playback_messages), with time.pos_in_frames = the chunk's first frame."""
import math

import numpy as np

import ahdsr_model as A
import status_model as S

F32 = np.float32
MAX_MIX_FRAMES = S.MAX_MIX_FRAMES
SPEED_UPDATE_CHUNK = 64            # FileSourceImpl::SPEED_UPDATE_CHUNK_SIZE (src/source/file/common.rs)
EPS100 = F32(F32(1.1920929e-07) * F32(100.0))   # ExponentialSmoothedValue::need_ramp (src/utils/smoothing.rs:198-206)


def speed_from_note(note):
    """utils.rs:67-78"""
    pitch = lambda n: 440.0 * math.pow(2.0, (float(n) - 69.0) / 12.0)
    return pitch(note) / pitch(60)


def pitch_factor(transpose, finetune):
    """voice.rs:146-147"""
    return math.pow(2.0, float(transpose) / 12.0 + float(finetune) / 1200.0)


class Smoother:
    """ExponentialSmoothedValue with the default inertia (smoothing.rs:139, :198-226) as AmplifiedSource / PannedSource run it: a write whose
    first step needs no ramp leaves the state alone (smoothing.rs:60-71, :98-101); otherwise one `next()` per sample / frame."""

    def __init__(self, value, sample_rate):
        self.current = self.target = F32(value)
        self.inertia, self.comp = F32(1.0 / 256.0), F32(F32(44100.0) / F32(sample_rate))

    def need_ramp(self):
        return abs(F32(F32(F32(self.target - self.current) * self.inertia) * self.comp)) > EPS100

    def set_target(self, t):
        self.target = F32(t)
        if not self.need_ramp():
            self.current = self.target

    def run(self, steps):
        for _ in range(steps):
            if not self.need_ramp():
                return
            self.current = F32(self.current + F32(F32(F32(self.target - self.current) * self.inertia) * self.comp))


class _NoStatus:
    def position(self, *a):
        pass

    def stopped(self, *a):
        pass


class GlidingFileSource(S.FileSource):
    """status_model.FileSource + set_speed with a glide (preloaded.rs:181-192, :418-446; common.rs:141-169): while current_speed != target_speed
    the write walks in chunks of SPEED_UPDATE_CHUNK frames and moves the resampler's ratio at each."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.current_speed = self.target_speed = float(kw.get("speed", 1.0))
        self.glide_rate, self.to_next_update = F32(0.0), 0

    def set_speed(self, speed, glide=None):
        if self.finished:
            return
        self.to_next_update = 0
        self.target_speed = float(speed)
        self.glide_rate = F32(glide) if glide is not None and glide > 0 else F32(0.0)
        if self.glide_rate == 0:
            self.current_speed = float(speed)
            self._update_speed()

    def _update_speed(self):
        diff = self.target_speed - self.current_speed
        if self.glide_rate > 0 and abs(diff) > 0.0001:
            semis = abs(12.0 * math.log2(self.target_speed / self.current_speed))
            duration_secs = F32(F32(semis) / self.glide_rate)
            if duration_secs > 0:
                duration_frames = F32(duration_secs * F32(self.out_rate))
                change = ((self.target_speed - self.current_speed) / float(duration_frames)) * float(SPEED_UPDATE_CHUNK)
                if abs(self.target_speed - self.current_speed) < abs(change):
                    self.current_speed = self.target_speed
                else:
                    self.current_speed += change
            else:
                self.current_speed = self.target_speed
        else:
            self.current_speed = self.target_speed
        self.cubic.ratio = self._ratio(self.current_speed)

    def _write_buffer(self, frames):
        if self.current_speed == self.target_speed:
            self.to_next_update = 0
            return super()._write_buffer(frames)
        total = 0
        while total < frames:
            if self.to_next_update == 0:
                if self.current_speed != self.target_speed:
                    self._update_speed()
                self.to_next_update = SPEED_UPDATE_CHUNK
            n = min(frames - total, self.to_next_update)
            w = super()._write_buffer(n)
            self.to_next_update -= w
            total += w
            if w < n:
                break
        return total


class Note:
    def __init__(self, note_id, slot, start, note, volume, panning, speed, inherited_volume, inherited_panning, volume_target, panning_target):
        self.note_id, self.slot, self.start, self.end = note_id, slot, start, None   # end: the frame it was stolen at, or behind the write that freed it
        self.stolen = False
        self.stolen_releasing = False                     # stolen while its envelope was in Release
        self.stole = None                                 # the id of the note this one took its slot from, None: the slot was free
        self.note, self.volume, self.panning = note, volume, panning
        self.inherited_volume, self.inherited_panning = inherited_volume, inherited_panning   # the smoothers' `current` as start() found them
        self.speed_events = [(start, speed, None)]        # (frame, effective speed, glide or None)
        self.volume_events = [(start, volume_target)]     # (frame, set_target value)
        self.panning_events = [(start, panning_target)]
        self.stop_frames = []                             # PreloadedFileSource::stop() calls (no envelope)
        self.release_frames = []                          # AhdsrEnvelope::note_off calls (with an envelope)
        self.gains = []                                   # with an envelope: one f32 per rendered frame from `start`


class Voice:
    """SamplerVoice (voice.rs:28-60): one slot of the pool."""

    def __init__(self, m):
        self.m = m
        self.note_id, self.note, self.note_volume, self.note_panning = None, 60, F32(1.0), F32(0.0)
        self.release_start_frame = None
        self.volume, self.panning = Smoother(1.0, m.sr), Smoother(0.0, m.sr)
        self.env = A.Envelope()
        self.file = None
        self.rec = None

    def is_active(self):
        return self.note_id is not None

    def reset(self):   # voice.rs:222-236
        if self.is_active():
            self.file = None   # PreloadedFileSource::reset: the next start finds a source as new
            self.note_id = None
        self.release_start_frame = None


class SamplerModel:
    def __init__(self, sample_rate, buffer_frames, channels, file_rate, voice_count=8, envelope=None, loop_range=None, transient=False, note_ids=None,
                 start_time=0, extra_cuts=()):
        """buffer_frames counts the frames the device gets (the decoder's extra zero frame included). envelope: keywords of ahdsr_model.Params
        or None. loop_range: the active loop range in source frames (Sampler::set_loop_range, or the buffer's embedded one) or None.
        note_ids: a one-element list shared by the samplers of one graph (unique_note_id).
        start_time: the sample time the owning mixer starts the sampler at (mixed.rs:565-576): no `write` reaches it before that frame, the first
        one begins exactly there when the frame lies inside a chunk, and the messages that came due earlier wait in its queue (mixed.rs:902-918)
        until the top of that write. extra_cuts: sample times of the owning mixer's OTHER events (a second sampler's messages, an ordinary
        voice's events): the mixer cuts its chunk there too (mixed.rs:679-712)."""
        self.sr, self.buffer_frames, self.channels, self.file_rate = sample_rate, buffer_frames, channels, file_rate
        self.env_params = A.Params(sample_rate, **envelope) if envelope is not None else None
        self.loop_range, self.transient = loop_range, transient
        self.voices = [Voice(self) for _ in range(voice_count)]
        self.transpose = self.finetune = 0
        self.base_volume, self.base_panning = F32(1.0), F32(0.0)
        self.stopping = self.stopped = False
        self.active_voices = 0
        self.queue, self._seq = [], 0
        self.note_ids = note_ids if note_ids is not None else [0]
        self.notes = {}
        self.pos = 0
        self.start_time, self.extra_cuts = int(start_time), sorted(set(int(t) for t in extra_cuts))

    # ---- the handle's calls: (sample_time, seq, fn) ----
    def _send(self, t, fn):
        self.queue.append((t, self._seq, fn))
        self._seq += 1

    def note_on(self, note, volume=1.0, panning=0.0, t=0):
        self.note_ids[0] += 1
        nid = self.note_ids[0]
        self._send(t, lambda now: self._trigger(lambda: self._note_on(nid, note, F32(volume), F32(panning), now)))
        return nid

    def note_off(self, note_id, t=0):
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, lambda v: self._stop_voice(v, now))))

    def all_notes_off(self, t=0):
        self._send(t, lambda now: self._trigger(lambda: [self._stop_voice(v, now) for v in self.voices]))

    def set_note_speed(self, note_id, speed, t=0, glide=None):
        def fn(v, now):
            eff = float(speed) * pitch_factor(self.transpose, self.finetune)
            v.file.set_speed(eff, glide)
            v.rec.speed_events.append((now, eff, glide))
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, lambda v: fn(v, now))))

    def set_note_volume(self, note_id, volume, t=0):
        def fn(v, now):
            v.note_volume = F32(volume)
            self._set_volume(v, now)
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, lambda v: fn(v, now))))

    def set_note_panning(self, note_id, panning, t=0):
        def fn(v, now):
            v.note_panning = F32(panning)
            self._set_panning(v, now)
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, lambda v: fn(v, now))))

    def set_parameter(self, name, raw, t=0):
        """name in transpose / finetune / volume / panning; raw: the resolved value."""
        def fn(now):
            if name in ("transpose", "finetune"):
                setattr(self, name, int(raw))
                for v in self.voices:
                    if v.is_active():   # set_base_pitch (voice.rs:258-268): no glide
                        eff = speed_from_note(v.note) * pitch_factor(self.transpose, self.finetune)
                        v.file.set_speed(eff, None)
                        v.rec.speed_events.append((now, eff, None))
            elif name == "volume":
                self.base_volume = F32(raw)
                for v in self.voices:
                    if v.is_active():
                        self._set_volume(v, now)
            else:
                self.base_panning = F32(raw)
                for v in self.voices:
                    if v.is_active():
                        self._set_panning(v, now)
        self._send(t, lambda now: self._trigger(lambda: fn(now)))

    def stop(self, t=0):
        def fn(now):   # sampler.rs:733-738: taken also while stopping
            self.stopping = self.transient
            for v in self.voices:
                self._stop_voice(v, now)
        self._send(t, fn)

    # ---- what the messages do ----
    def _trigger(self, fn):
        if not self.stopping:   # sampler.rs:663-664
            fn()

    def _with(self, note_id, fn):   # the FIRST slot whose note id matches (sampler.rs:776-822)
        for v in self.voices:
            if v.note_id == note_id:
                fn(v)
                return

    def _set_volume(self, v, now):
        t = F32(self.base_volume * v.note_volume)
        v.volume.set_target(t)
        v.rec.volume_events.append((now, t))

    def _set_panning(self, v, now):
        t = F32(min(max(F32(self.base_panning + v.note_panning), F32(-1.0)), F32(1.0)))
        v.panning.set_target(t)
        v.rec.panning_events.append((now, t))

    def _stop_voice(self, v, now):   # voice.rs:196-219
        if not v.is_active():
            return
        v.release_start_frame = now
        if self.env_params is not None:
            v.env.note_off(self.env_params)
            v.rec.release_frames.append(now)
        else:
            v.file.stop()
            v.rec.stop_frames.append(now)

    def next_free_voice_index(self):   # sampler.rs:826-860
        for i, v in enumerate(self.voices):
            if not v.is_active():
                return i
        candidate, earliest_release, oldest_id = 0, None, None
        for i, v in enumerate(self.voices):
            if self.env_params is not None and v.env.stage == A.RELEASE:
                if v.release_start_frame is not None and (earliest_release is None or v.release_start_frame < earliest_release):
                    earliest_release, oldest_id, candidate = v.release_start_frame, None, i
            elif earliest_release is None:
                if v.note_id is not None and (oldest_id is None or v.note_id < oldest_id):
                    oldest_id, candidate = v.note_id, i
        return candidate

    def _note_on(self, nid, note, volume, panning, now):   # trigger_note_on + SamplerVoice::start (voice.rs:122-193)
        i = self.next_free_voice_index()
        v = self.voices[i]
        victim = v.rec if v.is_active() else None
        if victim is not None:
            victim.end, victim.stolen = now, True
            victim.stolen_releasing = self.env_params is not None and v.env.stage == A.RELEASE
        v.reset()
        v.note, v.note_volume, v.note_panning = note, volume, panning
        eff = speed_from_note(note) * pitch_factor(self.transpose, self.finetune)
        repeat = S.U64_MAX if self.loop_range is not None else 0
        v.file = GlidingFileSource(_NoStatus(), self.buffer_frames, self.channels, self.file_rate, self.sr, speed=1.0, repeat=repeat, loop_range=self.loop_range, fade_out_seconds=0.05)
        v.file.set_speed(eff, None)
        inherited = (v.volume.current, v.panning.current)
        vt = F32(self.base_volume * volume)
        pt = F32(min(max(F32(self.base_panning + panning), F32(-1.0)), F32(1.0)))
        v.volume.set_target(vt)
        v.panning.set_target(pt)
        if self.env_params is not None:
            v.env.note_on(self.env_params, 1.0)
        v.note_id = nid
        v.rec = Note(nid, i, now, note, volume, panning, eff, inherited[0], inherited[1], vt, pt)
        v.rec.stole = victim.note_id if victim is not None else None
        self.notes[nid] = v.rec
        self.active_voices += 1

    # ---- Source::write of the sampler, once per chunk of its mixer ----
    def _write_chunk(self, frames, now):
        due = sorted([q for q in self.queue if q[0] <= now], key=lambda q: (q[0], q[1]))
        self.queue = [q for q in self.queue if q[0] > now]
        for _, _, fn in due:
            fn(now)
        if self.stopped or (self.active_voices == 0 and not self.stopping):
            return
        active = 0
        for v in self.voices:
            if not v.is_active():
                continue
            written = v.file.write(frames, now)
            stereo = 2 * written   # ChannelMappedSource: the sampler runs in stereo
            v.volume.run(stereo)      # apply_smoothed_gain: one step per sample while the smoother ramps
            v.panning.run(written)    # apply_smoothed_panning: one step per frame
            idle = False
            if self.env_params is not None:   # voice.rs:469-486
                e = v.env
                if e.stage in (A.SUSTAIN, A.IDLE):
                    v.rec.gains.extend([e.output] * written)
                else:
                    v.rec.gains.extend(e.run(self.env_params) for _ in range(written))
                idle = e.stage == A.IDLE
            if v.file.is_exhausted() or idle:   # voice.rs:488-502
                v.rec.end = now + frames
                v.reset()
            if v.is_active():
                active += 1
        self.active_voices = active
        if self.stopping and active == 0:
            self.stopped = True

    def write(self, frames, pos=None):
        """One write of the main mixer of `frames` frames at `pos` (default: behind the last one). Returns the state behind it (state())."""
        pos = self.pos if pos is None else pos
        total = 0
        while total < frames:
            main_chunk = min(frames - total, MAX_MIX_FRAMES)
            done = 0
            while done < main_chunk:
                now = pos + total + done
                later = [q[0] for q in self.queue if q[0] > now] + [t for t in self.extra_cuts if t > now]
                n = min(main_chunk - done, min(later) - now) if later else main_chunk - done
                if now + n <= self.start_time:        # process_sources skips a source that starts behind this chunk (mixed.rs:565-573)
                    pass
                elif now < self.start_time:           # ... and writes one that starts inside it from its start time on (:574-582)
                    self._write_chunk(now + n - self.start_time, self.start_time)
                else:
                    self._write_chunk(n, now)
                done += n
            total += main_chunk
        self.pos = pos + frames
        return self.state()

    def state(self):
        """What pg_graph_sampler_state reports: the sampler's fields and one dict per slot."""
        slots = []
        for v in self.voices:
            slots.append(dict(note_id=v.note_id if v.note_id is not None else 0, note=int(v.note), note_volume=F32(v.note_volume), note_panning=F32(v.note_panning),
                              envelope_stage=int(v.env.stage) if self.env_params is not None else -1, release_start_frame=v.release_start_frame))
        return dict(voice_count=len(self.voices), active_voices=sum(1 for v in self.voices if v.is_active()), stopping=self.stopping, stopped=self.stopped,
                    transpose=self.transpose, finetune=self.finetune, volume=F32(self.base_volume), panning=F32(self.base_panning), slots=slots)
