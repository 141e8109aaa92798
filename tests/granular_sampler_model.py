"""Independent restatement of the reference Sampler in granular mode (Sampler::with_granular_playback, src/generator/sampler.rs:598-637): the
note layer of src/generator/sampler.rs:656-860, :974-1028, :1076-1120 around granular voices (src/generator/sampler/voice.rs:122-310, :388-505)
whose pools are src/generator/sampler/granular.rs and whose matrices are src/modulation/matrix.rs. Written from the reference, not from the
device code.

It composes what the repository already restates: tests/sampler_model.py (speed_from_note, the pitch factor, the write grid),
tests/granular_params_model.py's ParamGrainPool (the pool behind its matrix, with the pool's own overlap mode; tests/granular_model.py and
tests/modulation_model.py under it) and tests/ahdsr_model.py (the envelope, frame by frame).

The model is driven per Sampler::write span. A slot stops being active at the END of the `write` in which its pool became exhausted or its
envelope went Idle (voice.rs:488-502), so where the spans end decides which slot a later note gets — and, because a pool that has run dry
keeps drawing from its generator until that end and GrainPool::reset does not reseed, every later note of the slot. The spans are the calls of
the owning mixer: one per chunk of the main mixer (min(remaining, 4096) frames from the start of a write), cut at the sampler's own messages
(they are events of its mixer) and at the `cuts` the caller names: the sample times of every OTHER event of the owning mixer and of its
ancestors (src/source/mixed.rs:679-712).

Orders that are this implementation's, documented in DESIGN.md: the grains of a frame are added in ascending slot order
(tests/granular_model.py), the voices in slot order (the reference's own: sampler.rs:989-1006).

Seeds: the reference seeds every generator from the OS. Here a sampler takes explicit Xoshiro256++ states per slot and generator (pool, LFO 1,
LFO 2), or derives them from the given ones by the rule include/phonic_gpu.h states (derive_state below)."""
import numpy as np

import ahdsr_model as A
import granular_model as gm
import granular_params_model as gpm
import modulation_model as mm
import sampler_model as sm

F32 = np.float32
M64 = (1 << 64) - 1
MAX_MIX_FRAMES = sm.MAX_MIX_FRAMES
TILE = 32   # pg_grain_kernel's tile: a statistic only (messages that land inside the first tile of the span they end)


def _splitmix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    x = z
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return z, x ^ (x >> 31)


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & M64


def derive_state(given, slot, generator):
    """The state of slot `slot`'s generator (0 pool, 1 LFO 1, 2 LFO 2) without an explicit table: `given` (all-zero or None: SplitMix64 of the
    fixed seed, four times) folded into one word, plus (3 slot + generator + 1) * 0xD1B54A32D192ED03, run through SplitMix64 four times; the low
    byte of the last word is 3 slot + generator, so no two generators of one sampler share a state."""
    base = gm.Xoshiro256pp(given).s
    index = 3 * int(slot) + int(generator) % 3
    z = ((base[0] ^ _rotl(base[1], 16) ^ _rotl(base[2], 32) ^ _rotl(base[3], 48)) + (index + 1) * 0xD1B54A32D192ED03) & M64
    out = []
    for _ in range(4):
        z, x = _splitmix(z)
        out.append(x)
    out[3] = (out[3] & ~0xFF & M64) | (index & 0xFF)
    if not any(out):
        out[0] = 1
    return tuple(out)


class Slot:
    """SamplerVoice in granular mode (voice.rs:28-60, :341-373): the per-note fields, the envelope, the pool behind its matrix."""

    def __init__(self, m, index, pool_state, lfo_states):
        self.m, self.index = m, index
        self.note_id, self.note, self.note_volume, self.note_panning = None, 60, F32(1.0), F32(0.0)
        self.release_start_frame = None
        self.env = A.Envelope()
        mod = m.modulation
        if mod is not None:   # create_matrix (state.rs:91-156), then the parameter and routing updates in front of the first note; no note yet
            matrix = mm.Matrix(m.sr, lfo_states)
            for l in range(2):
                matrix.set_lfo_rate(l, mod.get("rates", (1.0, 2.0))[l])
                matrix.set_lfo_waveform(l, mod.get("waveforms", (mm.SINE, mm.TRIANGLE))[l])
            for (s, t, amount, bipolar) in mod.get("routes", ()):
                matrix.set_modulation(s, t, amount, bipolar)
        else:
            matrix = None    # (ParamGrainPool then runs a matrix without routes: every sum is 0.0)
        self.pool = gpm.ParamGrainPool(m.sr, m.buf, m.p, matrix, pool_state)
        # GrainPool::new (granular.rs:384-429): ParamGrainPool's constructor is new() + start(); take the start() back
        pool = self.pool
        pool.trigger_new_grains, pool.trigger_phase = True, F32(0.0)
        pool.speed, pool.volume, pool.panning, pool.playhead, pool.playing_loop_range = 1.0, F32(1.0), F32(0.0), F32(0.0), False
        self.frees_exhausted = self.frees_idle = 0

    def is_active(self):
        return self.note_id is not None

    def pool_reset(self):   # GrainPool::reset (granular.rs:495-502) + Grain::deactivate (:1071-1074); the generator is not reseeded
        pool = self.pool
        pool.active[:] = False
        pool.samples_remaining[:] = 0
        pool.trigger_new_grains = True
        pool.primary = -1

    def reset(self):   # voice.rs:222-236
        if self.is_active():
            self.note_id = None
            self.pool_reset()
        self.release_start_frame = None

    def start(self, note_id, note, volume, panning):   # voice.rs:122-193
        m = self.m
        self.reset()
        self.note, self.note_volume, self.note_panning = int(note), F32(volume), F32(panning)
        pool = self.pool
        # GrainPool::start (granular.rs:474-489): the effective values, set directly
        pool.trigger_new_grains, pool.trigger_phase = True, F32(1.0)
        pool.speed = sm.speed_from_note(note) * sm.pitch_factor(m.transpose, m.finetune)
        pool.volume = F32(m.base_volume * F32(volume))
        pool.panning = F32(min(max(F32(m.base_panning + F32(panning)), F32(-1.0)), F32(1.0)))
        pool.playhead = F32(m.p.position)
        pool.playing_loop_range = False
        if m.env_params is not None:
            self.env.note_on(m.env_params, 1.0)
        if m.modulation is not None:
            pool.matrix.note_on(note, F32(volume))   # matrix.rs:394-408
        self.note_id = note_id

    def stop(self, now):   # voice.rs:196-219
        if not self.is_active():
            return
        self.release_start_frame = now
        if self.m.env_params is not None:
            self.env.note_off(self.m.env_params)
        else:
            self.pool.stop()   # (file_source.stop() starts a fade on a source that is never written: nothing follows from it)

    def process(self, frames):   # voice.rs:388-505; returns the voice's frames
        m = self.m
        out, _, _ = self.pool.process(frames)
        if m.env_params is not None:   # :469-486
            e = self.env
            if e.stage in (A.SUSTAIN, A.IDLE):
                out = (out * e.output).astype(F32)
            else:
                for f in range(frames):
                    g = e.run(m.env_params)
                    out[f, 0], out[f, 1] = F32(out[f, 0] * g), F32(out[f, 1] * g)
        exhausted = self.pool.is_exhausted()
        idle = m.env_params is not None and self.env.stage == A.IDLE
        if exhausted or idle:   # :488-502 (source.is_exhausted(): the file source is never written and never finished)
            self.frees_exhausted += int(exhausted)
            self.frees_idle += int(idle and not exhausted)
            self.reset()
        return out


class GranularSamplerModel:
    def __init__(self, sample_rate, buffer, params, voice_count=8, envelope=None, modulation=None, rng_states=None, transient=False, note_ids=None,
                 start_time=0, extra_cuts=()):
        """buffer: the granular mono buffer at the graph's rate. params: a granular_model.Params — the sampler's ONE parameter set (its loop_range
        is the pools' normalised one). envelope: keywords of ahdsr_model.Params or None. modulation: None (no matrix) or a dict with rates,
        waveforms, routes = [(source, target, amount, bipolar)] and rng_states = (LFO 1, LFO 2) base states. rng_states: None, or per slot
        (pool, LFO 1, LFO 2) states; params_rng_state: see derive_state. note_ids: a one-element list shared by the samplers of one graph.
        extra_cuts: sample times of the other events of the owning mixer chain (more can be given per write)."""
        self.sr = int(sample_rate)
        self.buf = np.ascontiguousarray(buffer, dtype=F32)
        self.p = params
        self.env_params = A.Params(sample_rate, **envelope) if envelope is not None else None
        self.modulation, self.transient = modulation, transient
        self.transpose = self.finetune = 0
        self.base_volume, self.base_panning = F32(1.0), F32(0.0)
        self.stopping = self.stopped = False
        self.active_voices = 0
        self.queue, self._seq = [], 0
        self.note_ids = note_ids if note_ids is not None else [0]
        self.pos = 0
        self.start_time, self.extra_cuts = int(start_time), sorted(set(int(t) for t in extra_cuts))
        base_pool = getattr(params, "rng_state", None)
        base_lfo = (modulation or {}).get("rng_states", (None, None))
        self.slots = []
        for k in range(voice_count):
            if rng_states is not None:
                pool_state, lfo_states = rng_states[k][0], (rng_states[k][1], rng_states[k][2])
            else:
                pool_state, lfo_states = derive_state(base_pool, k, 0), (derive_state(base_lfo[0], k, 1), derive_state(base_lfo[1], k, 2))
            self.slots.append(Slot(self, k, pool_state, lfo_states))
        # what a script did (the GPU tests qualify their random scripts by these, from the model alone)
        self.steals = 0
        self.first_tile_messages = 0
        self.allocations = []        # (frame, note id, slot, stolen note id or None)
        self.span_log = []           # (first frame, frames) of every Sampler::write
        self._span_start = None

    # ---- the handle's calls: (sample_time, seq, fn) ----
    def _send(self, t, fn):
        self.queue.append((int(t), self._seq, fn))
        self._seq += 1

    def note_on(self, note, volume=1.0, panning=0.0, t=0):
        self.note_ids[0] += 1
        nid = self.note_ids[0]
        self._send(t, lambda now: self._trigger(lambda: self._note_on(nid, note, F32(volume), F32(panning), now)))
        return nid

    def note_off(self, note_id, t=0):
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, lambda v: v.stop(now))))

    def all_notes_off(self, t=0):
        self._send(t, lambda now: self._trigger(lambda: [v.stop(now) for v in self.slots]))

    def set_note_speed(self, note_id, speed, t=0, glide=None):   # voice.rs:239-254: the pool gets the speed alone, no glide
        def fn(v):
            v.pool.set_speed(float(speed) * sm.pitch_factor(self.transpose, self.finetune))
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, fn)))

    def set_note_volume(self, note_id, volume, t=0):
        def fn(v):
            v.note_volume = F32(volume)
            v.pool.set_volume(F32(self.base_volume * v.note_volume))
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, fn)))

    def set_note_panning(self, note_id, panning, t=0):
        def fn(v):
            v.note_panning = F32(panning)
            v.pool.set_panning(self._pan(v))
        self._send(t, lambda now: self._trigger(lambda: self._with(note_id, fn)))

    def set_parameter(self, name, raw, t=0):
        """name in transpose / finetune / volume / panning; raw: the resolved value (sampler.rs:1076-1120): the stored base value, then every
        ACTIVE voice."""
        def fn():
            if name in ("transpose", "finetune"):
                setattr(self, name, int(raw))
                for v in self.slots:
                    if v.is_active():
                        v.pool.set_speed(sm.speed_from_note(v.note) * sm.pitch_factor(self.transpose, self.finetune))
            elif name == "volume":
                self.base_volume = F32(raw)
                for v in self.slots:
                    if v.is_active():
                        v.pool.set_volume(F32(self.base_volume * v.note_volume))
            else:
                self.base_panning = F32(raw)
                for v in self.slots:
                    if v.is_active():
                        v.pool.set_panning(self._pan(v))
        self._send(t, lambda now: self._trigger(fn))

    def set_granular_parameter(self, fourcc, value, t=0, normalized=False):
        """Sampler::set_granular_parameter (sampler.rs:299-360) on the sampler's one parameter set: every slot reads it from that frame on."""
        def fn():
            v = gpm.resolve(fourcc, value, normalized)
            if v is not None:
                setattr(self.p, gpm.FIELD[fourcc], int(v) if isinstance(v, int) else float(v))
        self._send(t, lambda now: self._trigger(fn))

    def stop(self, t=0):
        def fn(now):   # sampler.rs:733-738: taken also while stopping
            self.stopping = self.transient
            for v in self.slots:
                v.stop(now)
        self._send(t, fn)

    # ---- what the messages do ----
    def _pan(self, v):
        return F32(min(max(F32(self.base_panning + v.note_panning), F32(-1.0)), F32(1.0)))

    def _trigger(self, fn):
        if not self.stopping:   # sampler.rs:663-664
            fn()

    def _with(self, note_id, fn):   # the FIRST slot whose note id matches (sampler.rs:776-822)
        for v in self.slots:
            if v.note_id == note_id:
                fn(v)
                return

    def next_free_voice_index(self):   # sampler.rs:826-860
        for i, v in enumerate(self.slots):
            if not v.is_active():
                return i
        candidate, earliest_release, oldest_id = 0, None, None
        for i, v in enumerate(self.slots):
            if self.env_params is not None and v.env.stage == A.RELEASE:
                if v.release_start_frame is not None and (earliest_release is None or v.release_start_frame < earliest_release):
                    earliest_release, oldest_id, candidate = v.release_start_frame, None, i
            elif earliest_release is None:
                if v.note_id is not None and (oldest_id is None or v.note_id < oldest_id):
                    oldest_id, candidate = v.note_id, i
        return candidate

    def _note_on(self, nid, note, volume, panning, now):
        i = self.next_free_voice_index()
        v = self.slots[i]
        victim = v.note_id
        if victim is not None:
            self.steals += 1
        v.start(nid, note, volume, panning)
        self.allocations.append((now, nid, i, victim))
        self.active_voices += 1

    # ---- Source::write of the sampler, once per call of its mixer ----
    def _write_span(self, frames, now, out):
        """One Sampler::write of `frames` frames whose first frame is `now`; adds into out[frames, 2]."""
        due = sorted([q for q in self.queue if q[0] <= now], key=lambda q: (q[0], q[1]))
        self.queue = [q for q in self.queue if q[0] > now]
        if due and self._span_start is not None and 0 < now - self._span_start < TILE:
            self.first_tile_messages += len(due)
        self._span_start = now
        self.span_log.append((now, frames))
        for _, _, fn in due:
            fn(now)
        if self.stopped or (self.active_voices == 0 and not self.stopping):
            return
        active = 0
        for v in self.slots:
            if not v.is_active():
                continue
            voice = v.process(frames)
            out[:] = (out + voice).astype(F32)   # add_buffers, slot order
            if v.is_active():
                active += 1
        self.active_voices = active
        if self.stopping and active == 0:
            self.stopped = True

    def write(self, frames, pos=None, cuts=()):
        """One write of the main mixer of `frames` frames at `pos` (default: behind the last one). cuts: sample times at which the owning mixer
        chain cuts for other reasons than this sampler's messages. Returns the sampler's stereo frames [frames, 2] f32."""
        pos = self.pos if pos is None else pos
        cuts = sorted(set(self.extra_cuts) | set(int(t) for t in cuts))
        audio = np.zeros((frames, 2), dtype=F32)
        total = 0
        while total < frames:
            main_chunk = min(frames - total, MAX_MIX_FRAMES)
            done = 0
            while done < main_chunk:
                now = pos + total + done
                later = [q[0] for q in self.queue if q[0] > now] + [t for t in cuts if t > now]
                n = min(main_chunk - done, min(later) - now) if later else main_chunk - done
                a = total + done
                if now + n <= self.start_time:        # process_sources skips a source that starts behind this chunk (mixed.rs:565-573)
                    pass
                elif now < self.start_time:           # ... and writes one that starts inside it from its start time on (:574-582)
                    k = self.start_time - now
                    self._write_span(n - k, self.start_time, audio[a + k:a + n])
                else:
                    self._write_span(n, now, audio[a:a + n])
                done += n
            total += main_chunk
        self.pos = pos + frames
        return audio

    # ---- read-backs ----
    def state(self):
        """What pg_graph_sampler_state reports (tests/sampler_model.py's layout)."""
        slots = []
        for v in self.slots:
            slots.append(dict(note_id=v.note_id if v.note_id is not None else 0, note=int(v.note), note_volume=F32(v.note_volume), note_panning=F32(v.note_panning),
                              envelope_stage=int(v.env.stage) if self.env_params is not None else -1, release_start_frame=v.release_start_frame))
        return dict(voice_count=len(self.slots), active_voices=sum(1 for v in self.slots if v.is_active()), stopping=self.stopping, stopped=self.stopped,
                    transpose=self.transpose, finetune=self.finetune, volume=F32(self.base_volume), panning=F32(self.base_panning), slots=slots)

    def grain_state(self, slot):
        return self.slots[slot].pool.state()

    def modulation_state(self, slot):
        return self.slots[slot].pool.matrix.state()

    def params_state(self):
        return self.slots[0].pool.params_state()

    def frees(self):
        return sum(v.frees_exhausted for v in self.slots), sum(v.frees_idle for v in self.slots)
