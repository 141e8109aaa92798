"""What the note layer of granular-mode samplers costs: 16 sub-mixers, each with one 64-slot granular sampler whose slots all sound (1024 pools,
the 100-grain cloud of tools/granular_cost.py, no matrix), against 1024 lone granular voices with the same parameters, as ms per 1024-frame
step; the samplers with 0, 1 and 8 messages per step (per-note volume changes at evenly spaced frames, sent to every sampler: that many more
spans, each a pg_gsampler_kernel and a pg_grain_kernel launch). The configurations are measured interleaved, round after round; a step is one
pg_graph_write_device call on a caller's stream, timed by a hipEvent pair; medians over all rounds. PHONIC_LIB (tools/ab_libs/*.so) selects
another build of the library for the whole run: the lone voices of the parent commit are measured by running the tool once under each library.
The card's clocks while the steps ran are recorded (bench.py's sampler). The cost is reported, not gated.

    python tools/granular_sampler_cost.py [--steps 40] [--rounds 4] [--only <part of a configuration's name>] [--out profiles/granular_sampler_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phonic_amd import _capi  # noqa: E402
from phonic_amd.graph import Graph  # noqa: E402

SR, MF, WARMUP = 48000, 1024, 96
CLOUD = dict(density=100.0, size=1000.0, variation=1.0, spray=1.0, pan_spread=1.0, playback_direction=_capi.GRAIN_RANDOM, step=1.0)
MIXERS, SLOTS = 16, 64


def source(n=SR):
    t = np.arange(n, dtype=np.float64) / SR
    return (0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 3.0 * t)).astype(np.float32)


class Lone:
    def __init__(self):
        self.g = Graph(SR, 2, MF, 0)
        buf = self.g.add_sample_buffer(source(), 1, SR)
        for i in range(MIXERS * SLOTS):
            p = _capi.granular_params(rng_state=(i + 1, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, i * 7919 + 3), position=0.1 + 0.8 * (i % 97) / 97.0, **CLOUD)
            self.g.add_granular_voice_from_buffer(0, buf, p, volume=0.02, panning=((i % 21) - 10) / 10.0)

    def messages(self, pos):
        pass


class Samplers:
    def __init__(self, per_step):
        self.g, self.per_step = Graph(SR, 2, MF, 0), per_step
        buf = self.g.add_sample_buffer(source(), 1, SR)
        self.s, self.notes = [], []
        for m in range(MIXERS):
            p = _capi.granular_params(rng_state=(m + 1, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, m * 7919 + 3), position=0.1 + 0.8 * (m % 97) / 97.0, **CLOUD)
            s = self.g.add_granular_sampler(self.g.add_mixer(), buf, p, voice_count=SLOTS)
            self.s.append(s)
            self.notes.append([self.g.sampler_note_on(s, 60, 0.02, ((k % 21) - 10) / 10.0, 0) for k in range(SLOTS)])

    def messages(self, pos):
        for k in range(self.per_step):
            t = pos + (k + 1) * MF // (self.per_step + 1)
            for s, notes in zip(self.s, self.notes):
                self.g.sampler_set_note_volume(s, notes[k % SLOTS], 0.02, t)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "granular_sampler_cost.json"))
    a = ap.parse_args()
    import bench

    configs = {"lone_1024_voices": Lone}
    configs.update({f"16_samplers_x_64_slots_{k}_messages_per_step": (lambda k=k: Samplers(k)) for k in (0, 1, 8)})
    if a.only:   # (one configuration alone, by a part of its name: what a kernel trace of the run is read against)
        configs = {n: c for n, c in configs.items() if a.only in n}
    stream = torch.cuda.Stream(device=0)
    out = torch.zeros(2 * MF, dtype=torch.float32, device="cuda:0")
    rigs, pos, ms = {}, {}, {n: [] for n in configs}
    sampler = bench.ClockSampler(0)
    sampler.start()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        for name, make in configs.items():
            r = rigs[name] = make()
            pos[name] = 0
            for _ in range(WARMUP):
                assert r.g.write_device(out.data_ptr(), 2 * MF, pos[name], stream.cuda_stream) == 2 * MF
                pos[name] += MF
            stream.synchronize()
        per_round = max(1, a.steps // a.rounds)
        for _ in range(a.rounds):   # interleaved: every configuration in every round
            for name, r in rigs.items():
                for _ in range(per_round):
                    r.messages(pos[name])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    assert r.g.write_device(out.data_ptr(), 2 * MF, pos[name], stream.cuda_stream) == 2 * MF
                    e1.record(stream)
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
                    pos[name] += MF
    sampler.stop()
    try:
        clocks = sampler.summary([(t0, time.perf_counter())])
    except Exception as e:  # noqa: BLE001
        clocks = {"note": f"no clock record ({type(e).__name__}: {e})"}
    res = {}
    for name, r in rigs.items():
        v = sorted(ms[name])
        res[name] = {"ms_per_step_median": v[len(v) // 2], "ms_per_step_p10": v[len(v) // 10], "ms_per_step_p90": v[(9 * len(v)) // 10], "steps": len(v)}
        if isinstance(r, Samplers):
            res[name]["active_voices_of_sampler_0"] = r.g.sampler_state(r.s[0])["active_voices"]
        assert r.g.device_errors() == 0
    if "lone_1024_voices" in res:
        base = res["lone_1024_voices"]["ms_per_step_median"]
        for name in res:
            res[name]["ratio_to_lone_voices"] = res[name]["ms_per_step_median"] / base
    doc = {"workload": f"{MIXERS * SLOTS} grain pools (100-grain cloud, no matrix), {SR} Hz, steps of {MF} frames", "library": os.environ.get("PHONIC_LIB") or "this build",
           "timing": "hipEvent pair around one pg_graph_write_device call per step on a caller's stream; configurations interleaved per round; medians",
           "source_hash": _capi.source_hash(), "runs": res, "clocks": clocks}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
