"""Samplers on the MAIN mixer (pg_graph_add_sampler_to_main / pg_graph_add_granular_sampler_to_main): the two existing models of the note layer
(tests/sampler_model.py, tests/granular_sampler_model.py) driven on the main mixer's write grid, and the generator's output stage over the
sampler's sum. Written from the reference (src/player.rs:1048-1133, src/source/mixed.rs:659-719, src/source/amplified.rs:93-104,
src/source/panned.rs:93-104, src/utils/smoothing.rs:59-125), not from the device code. A plain module: no test lives here.

The grid. A message to a sampler on the main mixer is an event of the main mixer: it ends the mixer's chunk at its frame, and the next chunk
begins there and runs for min(remaining, 4096) frames (mixed.rs:679-712). The sampler's `write` runs once per such chunk. Under a sub-mixer the
PARENT's chunk goes on across the sub-mixer's events — the existing models' grid: fixed main chunks, cut inside at the messages. So the ends of
Sampler::write, where a slot becomes free and where a granular slot's generator stops drawing, differ between the two placements.
A message stamped before the sampler's start time cuts the chunk at its own time (the mixer pops the event there and finds a source that has not
started) and acts at the start time; THIS implementation makes the held message an event at the start time, so the chunk begins again there too —
the reference's goes on (DESIGN.md "Samplers on the main mixer", what is not exact). The model follows the implementation.

The output stage. AmplifiedSource::write and PannedSource::write take their message — a one-slot queue the mixer force_pushes into: of several
due in front of one write the last one sent counts — at the top of the write, then apply_smoothed_gain / apply_smoothed_panning over the samples
the Sampler returned: need_ramp() is asked ONCE, then one next() per interleaved sample (gain) or per frame (panning); at rest a scale iff
|1 - gain| > 1e-6 and the pan law iff |pan| > 1e-6. A write that returned 0 (sampler.rs:974-981) moves neither smoother. The smoother and the
pan law are tests/golden/numpy_restatement_fx.py's ExpSm and panning_factors, imported."""
import os
import sys

import numpy as np

import granular_sampler_model as G
import sampler_live_model as L
import sampler_model as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import numpy_restatement_fx as RF  # noqa: E402  (ExpSm, panning_factors)

F32 = np.float32
MAX_MIX_FRAMES = M.MAX_MIX_FRAMES


class OutputStage:
    """AmplifiedSource(volume) -> PannedSource(panning) over a stereo source, in f32."""

    def __init__(self, sample_rate, volume=1.0, panning=0.0):
        self.volume, self.panning = RF.ExpSm(F32(volume), sample_rate), RF.ExpSm(F32(panning), sample_rate)
        self.log = []   # per write that returned samples: (first frame, frames, gains, pans) — gains: [2 * frames] f32 or a scalar or None (left alone);
        #                 pans: ([frames] left, [frames] right) or a pair of scalars or None

    def message(self, kind, value):
        (self.volume if kind == "volume" else self.panning).set_target(F32(value))

    def write(self, now, frames):
        """The two wrappers over a write that returned `frames` frames."""
        if self.volume.need_ramp():
            gains = np.array([self.volume.next() for _ in range(2 * frames)], F32)
        else:
            g = self.volume.target
            gains = F32(g) if abs(float(F32(F32(1.0) - g))) > 0.000001 else None
        if self.panning.need_ramp():
            lr = [RF.panning_factors(self.panning.next()) for _ in range(frames)]
            pans = (np.array([a for a, _ in lr], F32), np.array([b for _, b in lr], F32))
        else:
            p = self.panning.target
            pans = RF.panning_factors(p) if abs(float(p)) > 0.000001 else None
        self.log.append((now, frames, gains, pans))

    def apply(self, audio, origin=0):
        """The stage over `audio` ([frames, 2] or interleaved f32 of the sampler's sum, first frame `origin`): a new array of the same shape."""
        a = np.array(audio, F32).reshape(-1, 2)
        for now, frames, gains, pans in self.log:
            lo, hi = max(now - origin, 0), min(now + frames - origin, len(a))
            if hi <= lo:
                continue
            s = slice(lo + origin - now, hi + origin - now)
            if gains is not None:
                g = gains.reshape(-1, 2)[s] if isinstance(gains, np.ndarray) else gains
                a[lo:hi] = (a[lo:hi] * g).astype(F32)
            if pans is not None:
                pl, pr = (pans[0][s], pans[1][s]) if isinstance(pans[0], np.ndarray) else pans
                a[lo:hi, 0] = (a[lo:hi, 0] * pl).astype(F32)
                a[lo:hi, 1] = (a[lo:hi, 1] * pr).astype(F32)
        return a.reshape(np.shape(audio))

    def state(self):
        """What pg_graph_sampler_output_state reports."""
        return dict(volume_current=F32(self.volume.current), volume_target=F32(self.volume.target), panning_current=F32(self.panning.current),
                    panning_target=F32(self.panning.target), volume_ramping=bool(self.volume.need_ramp()), panning_ramping=bool(self.panning.need_ramp()))


class _OnMain:
    """The main mixer's grid and the output stage around a model of the note layer (mixed in front of it). grid="sub" keeps the model's own
    grid — the sampler in a sub-mixer — and has no stage: what the two placements do to one script can be compared."""

    def _init_main(self, volume, panning, grid):
        self.grid = grid
        self.out = OutputStage(self.sr, volume, panning)
        self.out_queue = []       # (sample time, seq, kind, value)
        self.write_log = []       # (first frame, frames, returned samples?) of every Sampler::write

    def set_volume(self, volume, t=0):
        self.out_queue.append((int(t), self._seq, "volume", F32(volume)))
        self._seq += 1

    def set_panning(self, panning, t=0):
        self.out_queue.append((int(t), self._seq, "panning", F32(panning)))
        self._seq += 1

    def output_state(self):
        return self.out.state()

    def _next_cut(self, now, cuts):
        """The main mixer's next event behind `now`: a message's own time, the start time for one that is held until it, another source's event."""
        later = [t for t in cuts if t > now]
        for q in list(self.queue) + self.out_queue:
            if q[0] > now:
                later.append(q[0])
            elif self.start_time > now:   # (held: it came due before the start time)
                later.append(self.start_time)
        return min(later) if later else None

    def _main_write(self, frames, now, out):
        """One call of the sampler by the main mixer: the wrappers' messages, the Sampler's, its write, the stage."""
        due = sorted([q for q in self.out_queue if q[0] <= now], key=lambda q: (q[0], q[1]))
        self.out_queue = [q for q in self.out_queue if q[0] > now]
        for kind in ("volume", "panning"):
            last = [q for q in due if q[2] == kind]
            if last:
                self.out.message(kind, last[-1][3])
        due = sorted([q for q in self.queue if q[0] <= now], key=lambda q: (q[0], q[1]))
        self.queue = [q for q in self.queue if q[0] > now]
        for _, _, fn in due:
            fn(now)
        returned = not (self.stopped or (self.active_voices == 0 and not self.stopping))   # sampler.rs:974-981
        self.write_log.append((now, frames, returned))
        self._sampler_write(frames, now, out)   # (its messages are taken: it goes straight to the test above and the voices)
        if returned:
            self.out.write(now, frames)
            if out is not None:
                out[:] = self._staged(out, now)

    def _staged(self, out, now):
        """The last logged write's stage over its own frames."""
        keep, self.out.log = self.out.log, self.out.log[-1:]
        try:
            return self.out.apply(out, now)
        finally:
            self.out.log = keep

    def _write_main_grid(self, frames, pos, cuts, audio):
        cuts = sorted(set(self.extra_cuts) | set(int(t) for t in cuts))
        done = 0
        while done < frames:
            now = pos + done
            nxt = self._next_cut(now, cuts)
            n = min(frames - done, MAX_MIX_FRAMES, nxt - now if nxt is not None else frames)
            out = None if audio is None else audio[done:done + n]
            if now + n <= self.start_time:        # process_sources skips a source that starts behind this chunk (mixed.rs:565-573)
                pass
            elif now < self.start_time:           # ... and writes one that starts inside it from its start time on (:574-582)
                k = self.start_time - now
                self._main_write(n - k, self.start_time, None if out is None else out[k:])
            else:
                self._main_write(n, now, out)
            done += n
        self.pos = pos + frames


class MainSamplerModel(_OnMain, L.LiveSamplerModel):
    """A file sampler on the main mixer (with the messages-while-playing of tests/sampler_live_model.py). Audio is not modelled
    (tests/sampler_model.py): tests render the notes and pass the sum through `self.out.apply`."""

    def __init__(self, *a, volume=1.0, panning=0.0, grid="main", **kw):
        L.LiveSamplerModel.__init__(self, *a, **kw)
        self._init_main(volume, panning, grid)

    def _sampler_write(self, frames, now, out):
        M.SamplerModel._write_chunk(self, frames, now)

    def write(self, frames, pos=None, cuts=()):
        pos = self.pos if pos is None else pos
        if self.grid == "sub":
            return M.SamplerModel.write(self, frames, pos)
        self._write_main_grid(frames, pos, cuts, None)
        return self.state()


class MainGranularSamplerModel(_OnMain, L.LiveGranularSamplerModel):
    """A granular-mode sampler on the main mixer (with the messages-while-playing of tests/sampler_live_model.py): write returns the sampler's
    frames BEHIND the output stage."""

    def __init__(self, *a, volume=1.0, panning=0.0, grid="main", **kw):
        L.LiveGranularSamplerModel.__init__(self, *a, **kw)
        self._init_main(volume, panning, grid)

    def _sampler_write(self, frames, now, out):
        G.GranularSamplerModel._write_span(self, frames, now, out)

    def write(self, frames, pos=None, cuts=()):
        pos = self.pos if pos is None else pos
        if self.grid == "sub":
            return G.GranularSamplerModel.write(self, frames, pos, cuts)
        audio = np.zeros((frames, 2), dtype=F32)
        self._write_main_grid(frames, pos, cuts, audio)
        return audio
