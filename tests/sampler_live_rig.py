"""The rigs the tests of the samplers' messages-while-playing share (tests/test_gpu_granular_sampler_live.py, tests/test_gpu_sampler_live.py on
the device; tests/test_sampler_live_model.py for the script conditions both decide on the model alone): tests/granular_sampler_rig.py's and
tests/sampler_rig.py's rigs with the models of tests/sampler_live_model.py behind them and the new calls sent to graph and model alike. After
every write the existing bars hold and the envelope read-back equals the model's field by field, on every slot. A plain module: no test lives
here."""
import numpy as np

import granular_sampler_rig as R
import sampler_live_model as L
import sampler_rig as FR

SR = R.SR
SIZES = [300, 20, 4300, 1, 499]     # 5120 frames: a write across a chunk, one below a tile, one of 1 frame


class _LiveCalls:
    """The calls both kinds of sampler take."""

    def env(self, t, fourcc, value, normalized=False):
        self.times.append(t)
        self.g.sampler_set_envelope_parameter(self.s, fourcc, value, t, normalized)
        self.m.set_envelope_parameter(fourcc, value, t, normalized)

    def check_envelope(self, where, slots):
        if self.m.env_params is None:
            return
        exp = self.m.envelope_state()
        for k in slots:   # playing or free
            got = self.g.sampler_envelope_params(self.s, k)
            bad = [f for f in exp if not (got[f] == exp[f])]
            assert bad == [], (where, "envelope parameters of slot", k, bad, got, exp)


class GRig(_LiveCalls, R.Rig):
    """granular_sampler_rig.Rig with a LiveGranularSamplerModel."""

    def __init__(self, g, mixer, note_ids, voice_count, kw=R.SHORT, envelope=None, modulation=None, rng_states=None, transient=False, start_time=0, loop_range=None,
                 buf=R.BUF, buffer_id=None):
        super().__init__(g, mixer, note_ids, voice_count, kw=kw, envelope=envelope, modulation=modulation, rng_states=rng_states, transient=transient,
                         start_time=start_time, loop_range=loop_range, buf=buf, buffer_id=buffer_id)
        self.m = L.LiveGranularSamplerModel(SR, buf, R.model_params(kw, loop_range), voice_count=voice_count, envelope=envelope, modulation=modulation,
                                            rng_states=rng_states, transient=transient, note_ids=note_ids, start_time=start_time)
        if g is None:
            self.g = R.ModelOnly(self.m)

    def route(self, t, source, target, amount, bipolar=False):
        self.times.append(t)
        self.g.sampler_set_modulation(self.s, source, target, amount, bipolar, t)
        self.m.set_modulation(source, target, amount, bipolar, t)

    def unroute(self, t, source, target):
        self.times.append(t)
        self.g.sampler_clear_modulation(self.s, source, target, t)
        self.m.clear_modulation(source, target, t)

    def lfo_rate(self, t, lfo, rate):
        self.times.append(t)
        self.g.sampler_set_lfo_rate(self.s, lfo, rate, t)
        self.m.set_lfo_rate(lfo, rate, t)

    def lfo_waveform(self, t, lfo, waveform):
        self.times.append(t)
        self.g.sampler_set_lfo_waveform(self.s, lfo, waveform, t)
        self.m.set_lfo_waveform(lfo, waveform, t)

    def loop(self, t, loop_range):
        self.times.append(t)
        self.g.sampler_set_loop_range(self.s, loop_range, t)
        self.m.set_loop_range(loop_range, t)

    def check_state(self, where):
        super().check_state(where)
        self.check_envelope(where, range(self.n))


class FRig(_LiveCalls, FR.Rig):
    """sampler_rig.Rig with a LiveSamplerModel."""

    def __init__(self, g, mixer, pcm, note_ids, voice_count, envelope=None, transient=False, loop_range=None, start_time=0, channels=2, rate=FR.SR, buffer_loop=None):
        super().__init__(g, mixer, pcm, note_ids, voice_count, envelope=envelope, transient=transient, loop_range=loop_range, start_time=start_time, channels=channels,
                         rate=rate, buffer_loop=buffer_loop)
        self.n = voice_count
        self.m = L.LiveSamplerModel(FR.SR, pcm.size // channels, channels, rate, voice_count=voice_count, envelope=envelope, transient=transient, note_ids=note_ids,
                                    loop_range=self.loop, start_time=start_time)

    def check_state(self, where):
        super().check_state(where)
        self.check_envelope(where, range(self.n))


class FModelRig(_LiveCalls, FR.ModelRig):
    """The file sampler's calls against the model alone."""

    def __init__(self, frames, voice_count, envelope=None, **kw):
        self.m = L.LiveSamplerModel(FR.SR, frames, 2, FR.SR, voice_count=voice_count, envelope=envelope, **kw)
        self.ids, self.times, self.g, self.s, self.n = [], [], FR._NoGraph(self.m), None, voice_count


# ---- the seeded random scripts of tests/test_gpu_granular_sampler_live.py; tests/test_sampler_live_model.py decides their conditions on the model ----
SCRIPT_FRAMES = 12000
SCRIPT_SIZES = [300, 20, 4300, 1, 5000, 777, 1602]
assert sum(SCRIPT_SIZES) == SCRIPT_FRAMES
SCRIPT_CASES = [(2, 1), (5, 1), (8, 1)]   # (slots, seed)
SCRIPT_ENV = R.ENV
SCRIPT_MOD = dict(rates=(7.0, 13.0), waveforms=(0, 5), rng_states=R.LFO_RNG, routes=[(0, 0, 0.5, True), (1, 5, 0.3, False), (2, 1, -0.4, False)])
ENV_IDS = L.ENV_IDS


def script_rng(n_slots, seed):
    return np.random.default_rng(11000 * seed + 10 * n_slots)


def random_script(r, rng, n_slots):
    """tests/test_gpu_granular_sampler.py's random_script with its message mix extended by the new kinds: bursts of note-ons (three more than
    the pool has slots), then note-offs, setters, parameters and — about half of the messages behind a burst — envelope parameters, routes, LFO
    rates and waveforms and loop ranges; the pool drains before the next burst, and the burst behind it starts notes in slots that were free
    when a route changed."""
    bursts = 6
    t0 = 0
    frames = len(R.BUF)
    for b in range(bursts):
        t = t0 = max(t0, b * SCRIPT_FRAMES // bursts + int(rng.integers(0, 100))) + 1
        for _ in range(n_slots + 3):
            r.on(t, int(rng.integers(48, 84)), float(np.float32(rng.uniform(0.3, 1.0))), float(np.float32(rng.uniform(-1.0, 1.0))))
            t += int(rng.integers(0, 9))
        for _ in range(10):
            t += int(rng.integers(1, 60))
            k = int(rng.integers(0, len(r.ids))) if rng.random() < 0.9 else None
            u = rng.random()
            if u < 0.15:
                r.off(t, k)
            elif u < 0.22:
                r.vol(t, k, float(np.float32(rng.uniform(0.0, 1.2))))
            elif u < 0.30:
                r.speed(t, k, float(rng.uniform(0.5, 2.0)))
            elif u < 0.38:
                r.param(t, ("transpose", "finetune")[int(rng.integers(0, 2))], int(rng.integers(-12, 13)))
            elif u < 0.46:
                fourcc = ("GSIZ", "GDEN", "GVAR", "GSPY", "GPAN", "GPOS")[int(rng.integers(0, 6))]
                r.gparam(t, fourcc, float(np.float32(rng.uniform(0.0, 0.12) if fourcc == "GSIZ" else rng.uniform(0.0, 1.0))), True)
            elif u < 0.66:
                fourcc = ENV_IDS[int(rng.integers(0, 5))]
                if fourcc == "ASTN":
                    r.env(t, fourcc, float(np.float32(rng.uniform(0.0, 1.0))), bool(rng.random() < 0.5))
                else:   # milliseconds, a zero time now and then
                    r.env(t, fourcc, 0.0 if rng.random() < 0.15 else float(np.float32(rng.uniform(0.0005, 0.01))))
            elif u < 0.78:
                amount = 0.0 if rng.random() < 0.2 else float(np.float32(rng.uniform(-1.0, 1.0)))
                r.route(t, int(rng.integers(0, 4)), int(rng.integers(0, 7)), amount, bool(rng.random() < 0.5))
            elif u < 0.86:
                r.lfo_rate(t, int(rng.integers(0, 2)), float(np.float32(rng.uniform(0.0, 25.0))))
            elif u < 0.92:
                r.lfo_waveform(t, int(rng.integers(0, 2)), int(rng.integers(0, 7)))
            else:
                a = int(rng.integers(0, frames - 1))
                r.loop(t, None if rng.random() < 0.3 else (a, int(rng.integers(a + 1, frames + 1))))
        t += int(rng.integers(1, 30))
        r.all_off(t)
        t += 400 + int(rng.integers(1, 20))   # (SCRIPT_ENV's release is 240 frames: the pool has drained)
        r.route(t, int(rng.integers(0, 2)), int(rng.integers(0, 7)), float(np.float32(rng.uniform(0.2, 1.0))), True)   # every slot is free
        t0 = t + 50


def script_conditions(m):
    """What a script must contain, from the model alone: (an envelope message that found a note in Attack / Hold / Decay, one that found a note in
    Release, a route message and an LFO message with >= 2 slots sounding, a loop-range message while grains live, a note-on into a slot that was
    free at a route change before it)."""
    import ahdsr_model as A

    env_log = m.env_log or []
    rising = any(any(s in (A.ATTACK, A.HOLD, A.DECAY) for s in stages) for _, _, stages in env_log)
    releasing = any(A.RELEASE in stages for _, _, stages in env_log)
    route = any(kind == "route" and active >= 2 for _, kind, active, _, _ in m.live_log)
    lfo = any(kind == "lfo" and active >= 2 for _, kind, active, _, _ in m.live_log)
    loop = any(kind == "loop" and living >= 1 for _, kind, _, living, _ in m.live_log)
    routes = [(now, free) for now, kind, _, _, free in m.live_log if kind == "route"]
    free_then_note = any(any(now < frame and slot in free for now, free in routes) for frame, _, slot, _ in m.allocations)
    return dict(rising=rising, releasing=releasing, route=route, lfo=lfo, loop=loop, free_then_note=free_then_note)
