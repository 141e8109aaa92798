"""What a sampler on the MAIN mixer costs against the same pool in a sub-mixer: 16 samplers x 64 slots whose slots all sound, in file mode (a
looped one-second buffer) and in granular mode (tools/granular_sampler_cost.py's 100-grain cloud, no matrix) —
    sub      16 sub-mixers with one sampler each (pg_graph_add_sampler / pg_graph_add_granular_sampler): the existing placement
    main     16 samplers on the main mixer (pg_graph_add_sampler_to_main / _granular_sampler_to_main) at unity: the output stage's skip branches
    ramp     ... with a volume ramp always running: every step begins with a pg_graph_sampler_set_volume to every sampler, alternating 0.5 / 1.0
             (an exponential ramp outlasts the step's 1024 frames at the per-sample rate; the message is an event of the main mixer at the
             step's first frame, where a chunk begins anyway)
as ms per 1024-frame step. The configurations are measured interleaved, round after round; a step is one pg_graph_write_device call on a
caller's stream, timed by a hipEvent pair; medians over all rounds. The cost is reported, not gated.

    python tools/main_sampler_cost.py [--steps 60] [--rounds 6] [--only <part of a configuration's name>] [--out profiles/main_sampler_cost.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import granular_sampler_cost as base  # noqa: E402  (the source buffer, the cloud, the sizes)
from phonic_amd import _capi  # noqa: E402
from phonic_amd.graph import Graph  # noqa: E402

SR, MF, WARMUP, MIXERS, SLOTS, CLOUD = base.SR, base.MF, base.WARMUP, base.MIXERS, base.SLOTS, base.CLOUD


class Pools:
    def __init__(self, granular, place):
        self.g, self.place, self.step = Graph(SR, 2, MF, 0), place, 0
        pcm = base.source()
        buf = self.g.add_sample_buffer(pcm, 1, SR, loop_range=None if granular else (0, len(pcm) - 1))
        self.s = []
        for m in range(MIXERS):
            if granular:
                p = _capi.granular_params(rng_state=(m + 1, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, m * 7919 + 3), position=0.1 + 0.8 * (m % 97) / 97.0, **CLOUD)
                s = self.g.add_granular_sampler(self.g.add_mixer(), buf, p, voice_count=SLOTS) if place == "sub" else self.g.add_granular_sampler_to_main(buf, p, voice_count=SLOTS)
            else:
                s = self.g.add_sampler(self.g.add_mixer(), buf, voice_count=SLOTS) if place == "sub" else self.g.add_sampler_to_main(buf, voice_count=SLOTS)
            self.s.append(s)
            for k in range(SLOTS):
                self.g.sampler_note_on(s, 48 + k % 25, 0.02, ((k % 21) - 10) / 10.0, 0)

    def messages(self, pos):
        if self.place != "ramp":
            return
        self.step += 1
        for s in self.s:
            self.g.sampler_set_volume(s, 0.5 if self.step % 2 else 1.0, pos)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "main_sampler_cost.json"))
    a = ap.parse_args()
    import bench

    configs = {f"{'granular' if gr else 'file'}_{place}": (lambda gr=gr, place=place: Pools(gr, place)) for gr in (False, True) for place in ("sub", "main", "ramp")}
    if a.only:
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
                r.messages(pos[name])
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
        res[name] = {"ms_per_step_median": v[len(v) // 2], "ms_per_step_p10": v[len(v) // 10], "ms_per_step_p90": v[(9 * len(v)) // 10], "steps": len(v),
                     "active_voices_of_sampler_0": r.g.sampler_state(r.s[0])["active_voices"]}
        if r.place != "sub":
            res[name]["output_state_of_sampler_0"] = {k: (bool(x) if isinstance(x, bool) else float(x)) for k, x in r.g.sampler_output_state(r.s[0]).items()}
        assert r.g.device_errors() == 0
    for name in res:
        sub = res.get(name.split("_")[0] + "_sub")
        if sub:
            res[name]["ratio_to_sub_mixers"] = res[name]["ms_per_step_median"] / sub["ms_per_step_median"]
    doc = {"workload": f"{MIXERS} samplers x {SLOTS} slots, every slot sounding, {SR} Hz, steps of {MF} frames: file pools (looped buffer) and granular pools (100-grain cloud, no matrix)",
           "timing": "hipEvent pair around one pg_graph_write_device call per step on a caller's stream; configurations interleaved per round; medians",
           "source_hash": _capi.source_hash(), "runs": res, "clocks": clocks}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
