"""The rig the sampler's GPU tests share (tests/test_gpu_sampler.py, tests/test_gpu_sampler_pools.py): one sampler on the GPU and its model
(tests/sampler_model.py) driven by the same calls, the writes with the slot table compared after every one, and the expected audio rendered
note by note through the CPU oracle. A plain module: no test lives here.

Expected audio: every note of the model is rendered as one ordinary voice of an OracleGraph that starts at the model's start frame with the
smoother values the slot handed down (the set-targets follow at its start), gets the model's speed, volume, panning and stop events, the
buffer's channels and rate and the pool's loop range (repeat forever: Sampler::set_loop_range / the file's embedded loop), is cut at the frame
the model says it was stolen or freed at, and is multiplied by the model's envelope gains in f32; the notes are then added in slot order in
f32 — the reference's own order (sampler.rs:989-1006)."""
import numpy as np

import oracle
import sampler_model as M
from phonic_amd import workloads
from phonic_amd.graph import Graph

SR = 48000
MF = 1024
SHORT = workloads.tone_buffer(1, SR, 6000 / SR)    # 6001 frames: ends by itself
LONG = workloads.tone_buffer(2, SR, 4.0)           # 192001 frames: outlasts 1.5 s at any speed used here
ENV = dict(attack_s=0.01, hold_s=0.05, decay_s=0.05, sustain_level=0.75, release_s=0.1)
UNKNOWN = 999999
U64_MAX = (1 << 64) - 1


def _frames(pcm, channels=2):
    return pcm.size // channels


def _db_to_linear(x):
    lib = oracle.lib()
    return np.float32(lib.po_db_to_linear(np.float32(x)))


def resolve(name, value, normalized):
    """The raw value a parameter update resolves to (sampler.rs:862-906; integer.rs:110-126, float.rs:137-141, scaling.rs:45-74), from the
    descriptors' constants: STRN -48..48, SFTN -100..100, SVOL 0.000001..15.848932 Decibel(-60, 24), SPAN -1..1."""
    f = np.float32
    if name in ("transpose", "finetune"):
        lo, hi = (-48, 48) if name == "transpose" else (-100, 100)
        if not normalized:
            return int(min(max(int(value), lo), hi))
        x = f(f(lo) + f(f(value) * f(hi - lo)))
        return int(np.floor(abs(x) + f(0.5)) * np.sign(x))   # f32::round: half away from zero
    lo, hi = (f(0.000001), f(15.848932)) if name == "volume" else (f(-1.0), f(1.0))
    if not normalized:
        return f(min(max(f(value), lo), hi))
    n = f(value)
    if name == "volume":
        db = f(f(-60.0) + f(n * f(f(24.0) - f(-60.0))))
        mn, mx = _db_to_linear(-60.0), _db_to_linear(24.0)
        n = f(f(_db_to_linear(db) - mn) / f(mx - mn))
    return f(lo + f(n * f(hi - lo)))


PARAM_ID = dict(transpose="STRN", finetune="SFTN", volume="SVOL", panning="SPAN")


class Rig:
    """One sampler on the GPU and its model, driven by the same calls. loop_range: the sampler's own (Sampler::set_loop_range); start_time: the
    sampler's; channels, rate, buffer_loop: the sample buffer's channel count, rate and embedded loop."""

    def __init__(self, g, mixer, pcm, note_ids, voice_count, envelope=None, transient=False, loop_range=None, start_time=0, channels=2, rate=SR, buffer_loop=None):
        self.g, self.pcm = g, pcm
        self.channels, self.rate = channels, rate
        self.loop = loop_range if loop_range is not None else buffer_loop   # the range the pool's voices play (voice.rs:313-328, preloaded.rs:89-104)
        self.buf = g.add_sample_buffer(pcm, channels, rate, loop_range=buffer_loop)
        self.s = g.add_sampler(mixer, self.buf, voice_count=voice_count, envelope=envelope, transient=transient, loop_range=loop_range, start_time=start_time)
        self.m = M.SamplerModel(SR, _frames(pcm, channels), channels, rate, voice_count=voice_count, envelope=envelope, transient=transient, note_ids=note_ids,
                                loop_range=self.loop, start_time=start_time)
        self.ids = []
        self.times = []    # the sample time of every message sent, in sending order

    def _id(self, k):
        return UNKNOWN if k is None else self.ids[k]

    def on(self, t, note, volume=1.0, panning=0.0):
        self.times.append(t)
        a, b = self.g.sampler_note_on(self.s, note, volume, panning, t), self.m.note_on(note, volume, panning, t)
        assert a == b, (a, b)
        self.ids.append(a)
        return len(self.ids) - 1

    def off(self, t, k):
        self.times.append(t)
        self.g.sampler_note_off(self.s, self._id(k), t)
        self.m.note_off(self._id(k), t)

    def all_off(self, t):
        self.times.append(t)
        self.g.sampler_all_notes_off(self.s, t)
        self.m.all_notes_off(t)

    def speed(self, t, k, speed, glide=None):
        self.times.append(t)
        self.g.sampler_set_note_speed(self.s, self._id(k), speed, t, glide)
        self.m.set_note_speed(self._id(k), speed, t, glide)

    def vol(self, t, k, v):
        self.times.append(t)
        self.g.sampler_set_note_volume(self.s, self._id(k), v, t)
        self.m.set_note_volume(self._id(k), v, t)

    def pan(self, t, k, p):
        self.times.append(t)
        self.g.sampler_set_note_panning(self.s, self._id(k), p, t)
        self.m.set_note_panning(self._id(k), p, t)

    def param(self, t, name, value, normalized=False):
        self.times.append(t)
        self.g.sampler_set_parameter(self.s, PARAM_ID[name], value, t, normalized)
        self.m.set_parameter(name, resolve(name, value, normalized), t)

    def stop(self, t):
        self.times.append(t)
        self.g.sampler_stop(self.s, t)
        self.m.stop(t)

    def check_state(self, where):
        got, exp = self.g.sampler_state(self.s), self.m.state()
        slots_g, slots_e = got.pop("slots"), exp.pop("slots")
        assert got == exp, (where, got, exp)
        for i, (a, b) in enumerate(zip(slots_g, slots_e)):
            assert a == b, (where, i, a, b)

    def expected(self, n_frames, origin=0):
        """expected_audio of this rig's model for frames [origin, origin + n_frames)."""
        return expected_audio(self.m, self.pcm, n_frames, channels=self.channels, rate=self.rate, loop_range=self.loop, origin=origin)


class ModelRig(Rig):
    """The same calls against the model alone: what a script does to the pool can be asserted without a GPU."""

    def __init__(self, frames, voice_count, envelope=None, **kw):
        self.m = M.SamplerModel(SR, frames, 2, SR, voice_count=voice_count, envelope=envelope, **kw)
        self.ids, self.times, self.g, self.s = [], [], _NoGraph(self.m), None


class _NoGraph:
    """Stands where ModelRig has no graph: note_on answers with the id the model is about to hand out, everything else does nothing."""

    def __init__(self, m):
        self._m = m

    def sampler_note_on(self, *a):
        return self._m.note_ids[0] + 1

    def __getattr__(self, name):
        return lambda *a, **kw: None


def _single(pcm, voice_count, envelope=None, transient=False, **kw):
    g = Graph(SR, 2, MF, 0)
    return g, Rig(g, g.add_mixer(), pcm, [0], voice_count, envelope, transient, **kw)


def _run(g, rigs, sizes, pos=0):
    """The writes, from frame `pos` on; after every one, every sampler's state against its model."""
    out = []
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        for r in rigs:
            r.m.write(n, pos)
            r.check_state((k, pos + n))
        pos += n
        out.append(buf)
    assert g.device_errors() == 0
    return np.concatenate(out)


def _note_audio(rec, pcm, n_frames, channels=2, rate=SR, loop_range=None, origin=0):
    """One note as an ordinary oracle voice (stereo frames x 2) over frames [origin, origin + n_frames), uncut and without its envelope. A mixer
    holds ONE stop time per source, so every stop() of the note is sent when the oracle's writes have reached its frame: the writes are cut
    there (how a source's audio is cut into writes changes none of its samples)."""
    o = oracle.OracleGraph(SR, 2, MF)
    mx = o.add_mixer()
    first = origin + ((rec.start - origin) // MF) * MF
    loop = {} if loop_range is None else dict(has_repeat=1, repeat=U64_MAX, has_loop_range=1, loop_start=int(loop_range[0]), loop_end=int(loop_range[1]))
    v = o.add_voice(mx, pcm, channels, rate, volume=float(rec.inherited_volume), panning=float(rec.inherited_panning), speed=rec.speed_events[0][1], start_time=rec.start, **loop)
    for t, x in rec.volume_events:
        o.set_voice_volume(v, float(x), t)
    for t, x in rec.panning_events:
        o.set_voice_panning(v, float(x), t)
    for t, sp, gl in rec.speed_events[1:]:
        o.set_voice_speed(v, sp, t, glide=gl)
    stop = origin + n_frames
    end = rec.end if rec.end is not None else stop
    last = min(origin + ((end - origin + MF - 1) // MF) * MF, stop)
    audio = np.zeros((n_frames, 2), np.float32)
    cuts = sorted(set(list(range(first, last, MF)) + [t for t in rec.stop_frames if first < t < last]) | {last})
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a in rec.stop_frames:
            o.stop_voice(v, a)
        buf = np.zeros(2 * (b - a), np.float32)
        o.write(buf, a)
        audio[a - origin:b - origin] = buf.reshape(-1, 2)
    return audio


def expected_audio(model, pcm, n_frames, channels=2, rate=SR, loop_range=None, origin=0):
    slots = [np.zeros((n_frames, 2), np.float32) for _ in model.voices]
    for rec in model.notes.values():
        a = _note_audio(rec, pcm, n_frames, channels, rate, loop_range, origin)
        start = rec.start - origin
        end = min(rec.end - origin if rec.end is not None else n_frames, n_frames)
        a[end:] = 0.0
        if model.env_params is not None:
            gains = np.zeros(n_frames, np.float32)
            k = min(len(rec.gains), n_frames - start)
            gains[start:start + k] = np.asarray(rec.gains[:k], np.float32)
            a = (a * gains[:, None]).astype(np.float32)
        slots[rec.slot] = (slots[rec.slot] + a).astype(np.float32)
    out = np.zeros((n_frames, 2), np.float32)
    for s in slots:   # the sampler's sum: its active voices in slot order (sampler.rs:989-1006)
        out = (out + s).astype(np.float32)
    return out.reshape(-1)


def _assert_equal(got, exp):
    assert np.abs(exp).max() > 1e-3
    assert np.array_equal(got, exp), (int(np.flatnonzero(got != exp)[0]) // 2, float(np.abs(got - exp).max()))


def pool_script(r, rng, n_frames, n_messages, p_on=0.7, first=1):
    """About n_messages messages on distinct frames from `first` on, sent in frame order: note-ons (the share p_on of them), and the rest in the
    proportions of test_gpu_sampler.py's _random_script: note-offs, the per-note setters on living, ended and unknown ids, base parameters,
    all-notes-off. `r`: a Rig or a ModelRig."""
    frames = sorted(int(x) for x in rng.choice(np.arange(first, n_frames - 1), size=n_messages, replace=False))
    for t in frames:
        u = rng.random()
        k = int(rng.integers(0, len(r.ids))) if r.ids and rng.random() < 0.9 else None
        w = 0.5 + 0.5 * (u - p_on) / (1.0 - p_on)    # the rest, scaled onto _random_script's 0.5..1
        if u < p_on or not r.ids:
            r.on(t, int(rng.integers(48, 73)), float(np.float32(rng.uniform(0.2, 1.0))), float(np.float32(rng.uniform(-1.0, 1.0))))
        elif w < 0.68:
            r.off(t, k)
        elif w < 0.74:
            r.vol(t, k, float(np.float32(rng.uniform(0.0, 1.2))))
        elif w < 0.80:
            r.pan(t, k, float(np.float32(rng.uniform(-1.0, 1.0))))
        elif w < 0.85:
            r.speed(t, k, float(rng.uniform(0.5, 2.0)), glide=float(rng.uniform(6.0, 48.0)) if rng.random() < 0.5 else None)
        elif w < 0.96:
            name = ("transpose", "finetune", "volume", "panning")[int(rng.integers(0, 4))]
            normalized = bool(rng.random() < 0.5)
            raw = dict(transpose=int(rng.integers(-12, 13)), finetune=int(rng.integers(-100, 101)), volume=float(np.float32(rng.uniform(0.1, 1.5))),
                       panning=float(np.float32(rng.uniform(-1.0, 1.0))))[name]
            r.param(t, name, float(np.float32(rng.uniform(0.3, 0.7))) if normalized else raw, normalized)
        else:
            r.all_off(t)


POOL_CASES = [(33, False, 1), (33, False, 2), (33, True, 1), (33, True, 2), (64, False, 1), (64, False, 2), (64, True, 1), (64, True, 2)]   # (voice_count, envelope, seed)
POOL_PIECES, POOL_MESSAGES = 16, 250


def pool_rng(voice_count, envelope, seed):
    return np.random.default_rng(7000 * seed + 10 * voice_count + int(envelope))


def assert_pool_script_conditions(m, envelope):
    """What a large-pool random script must contain (conditions on the script: the model alone decides them): a steal, with an envelope a steal of
    a releasing slot, and a note that starts in a slot at or above 32 by stealing."""
    notes = list(m.notes.values())
    assert any(rec.stolen for rec in notes)
    if envelope:
        assert any(rec.stolen and rec.stolen_releasing for rec in notes)
    assert any(rec.stole is not None and rec.slot >= 32 for rec in notes)
