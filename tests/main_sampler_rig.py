"""The rigs of the GPU tests of samplers on the main mixer (tests/test_gpu_main_sampler.py): tests/sampler_live_rig.py's two rigs with the sampler
added through pg_graph_add_sampler_to_main / pg_graph_add_granular_sampler_to_main, tests/main_sampler_model.py's models behind them, and the
two calls of the output stage sent to graph and model alike. After every write the existing bars hold (slot table, envelope read-back, a
granular sampler's grain, matrix and parameter state) and pg_graph_sampler_output_state equals the model's, bit for bit.
A plain module: no test lives here."""
import numpy as np

import granular_sampler_rig as GR
import main_sampler_model as MM
import sampler_live_rig as LR
import sampler_rig as FR

SR, MF = FR.SR, FR.MF


class _OutputCalls:
    def out_volume(self, t, v):
        self.times.append(t)
        self.g.sampler_set_volume(self.s, v, t)
        self.m.set_volume(v, t)

    def out_pan(self, t, p):
        self.times.append(t)
        self.g.sampler_set_panning(self.s, p, t)
        self.m.set_panning(p, t)

    def check_output(self, where):
        got, exp = self.g.sampler_output_state(self.s), self.m.output_state()
        bad = [k for k in exp if not (np.asarray(got[k]).tobytes() == np.asarray(exp[k]).tobytes())]
        assert bad == [], (where, "output stage", bad, got, exp)


class FileRig(_OutputCalls, LR.FRig):
    """A file sampler on the main mixer of `g` and its model."""

    def __init__(self, g, pcm, note_ids, voice_count, envelope=None, transient=False, loop_range=None, start_time=0, channels=2, rate=SR, buffer_loop=None,
                 volume=1.0, panning=0.0):
        self.g, self.pcm, self.n = g, pcm, voice_count
        self.channels, self.rate = channels, rate
        self.loop = loop_range if loop_range is not None else buffer_loop
        self.buf = g.add_sample_buffer(pcm, channels, rate, loop_range=buffer_loop)
        self.s = g.add_sampler_to_main(self.buf, volume, panning, voice_count=voice_count, envelope=envelope, transient=transient, loop_range=loop_range, start_time=start_time)
        self.m = MM.MainSamplerModel(SR, pcm.size // channels, channels, rate, voice_count=voice_count, envelope=envelope, transient=transient, note_ids=note_ids,
                                     loop_range=self.loop, start_time=start_time, volume=volume, panning=panning)
        self.ids, self.times = [], []

    def check_state(self, where):
        LR.FRig.check_state(self, where)
        self.check_output(where)

    def expected(self, n_frames, origin=0):
        """The pool's sum behind the output stage: tests/sampler_rig.py's expected_audio with every note rendered on the sampler's OWN write grid."""
        keep = FR._note_audio
        FR._note_audio = lambda rec, pcm, n, channels=2, rate=SR, loop_range=None, origin=0: _note_audio_on_grid(self.m.write_log, rec, pcm, n, channels, rate, loop_range, origin)
        try:
            pool = FR.expected_audio(self.m, self.pcm, n_frames, channels=self.channels, rate=self.rate, loop_range=self.loop, origin=origin)
        finally:
            FR._note_audio = keep
        return self.m.out.apply(pool, origin)


class GranularRig(_OutputCalls, LR.GRig):
    """A granular-mode sampler on the main mixer of `g` and its model."""

    def __init__(self, g, note_ids, voice_count, kw=GR.SHORT, envelope=None, modulation=None, rng_states=None, transient=False, start_time=0, loop_range=None, buf=GR.BUF,
                 buffer_id=None, volume=1.0, panning=0.0):
        self.m = MM.MainGranularSamplerModel(SR, buf, GR.model_params(kw, loop_range), voice_count=voice_count, envelope=envelope, modulation=modulation, rng_states=rng_states,
                                             transient=transient, note_ids=note_ids, start_time=start_time, volume=volume, panning=panning)
        self.n, self.modulation = voice_count, modulation
        self.ids, self.times = [], []
        self.g = g
        self.buf = buffer_id if buffer_id is not None else g.add_sample_buffer(buf, 1, SR)
        self.s = g.add_granular_sampler_to_main(self.buf, GR.capi_params(kw, loop_range), GR.capi_modulation(modulation), rng_states, volume, panning, voice_count=voice_count,
                                                envelope=envelope, transient=transient, start_time=start_time)

    def check_state(self, where):
        LR.GRig.check_state(self, where)
        self.check_output(where)


def _note_audio_on_grid(write_log, rec, pcm, n_frames, channels, rate, loop_range, origin):
    """tests/sampler_rig.py's _note_audio — one note as an ordinary oracle voice, uncut and without its envelope — with the oracle's writes cut where
    the SAMPLER's writes were (the model's write_log) instead of every 1024 frames. How a source's audio is cut into writes changes none of its
    samples but the last ones: a fade-out's fader is asked whether it has arrived once per source write, so the faded tail runs to the end of the
    write in which it arrives — on the main mixer's grid that is a chunk of up to 4096 frames that begins at a message, not a block of 1024."""
    import oracle

    o = oracle.OracleGraph(SR, 2, 4096)
    mx = o.add_mixer()
    loop = {} if loop_range is None else dict(has_repeat=1, repeat=FR.U64_MAX, has_loop_range=1, loop_start=int(loop_range[0]), loop_end=int(loop_range[1]))
    v = o.add_voice(mx, pcm, channels, rate, volume=float(rec.inherited_volume), panning=float(rec.inherited_panning), speed=rec.speed_events[0][1], start_time=rec.start, **loop)
    for t, x in rec.volume_events:
        o.set_voice_volume(v, float(x), t)
    for t, x in rec.panning_events:
        o.set_voice_panning(v, float(x), t)
    for t, sp, gl in rec.speed_events[1:]:
        o.set_voice_speed(v, sp, t, glide=gl)
    stop = origin + n_frames
    end = rec.end if rec.end is not None else stop
    audio = np.zeros((n_frames, 2), np.float32)
    for a, frames, _ in write_log:
        b = min(a + frames, stop)
        if b <= rec.start or a >= end or a < origin or b <= a:
            continue
        if a in rec.stop_frames:
            o.stop_voice(v, a)
        buf = np.zeros(2 * (b - a), np.float32)
        o.write(buf, a)
        audio[a - origin:b - origin] = buf.reshape(-1, 2)
    return audio


def run_file(g, rigs, sizes, pos=0, cuts=()):
    """The writes from frame `pos` on; after every one every rig's read-backs against its model. cuts: the main mixer's other events (every
    message of another rig is one). Returns the device's interleaved audio."""
    out = []
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, dtype=np.float32)
        g.write(buf, pos)
        for r in rigs:
            others = set(cuts) | set(t for q in rigs if q is not r for t in q.times)
            r.m.write(n, pos, cuts=others)
            r.check_state((k, pos + n))
        pos += n
        out.append(buf)
    assert g.device_errors() == 0
    return np.concatenate(out)


def assert_values_equal(got, exp, silent_ok=False):
    """Equal as values (an all-zero sample may carry the other zero's sign), and not silence."""
    got, exp = np.asarray(got, np.float32).reshape(-1), np.asarray(exp, np.float32).reshape(-1)
    assert silent_ok or np.abs(exp).max() > 1e-3
    same = got == exp
    assert same.all(), ("first differing frame", int(np.flatnonzero(~same)[0]) // 2, float(np.abs(got - exp).max()))
