"""What granular voices cost: 1024 granular voices on the main mixer at 48 kHz, three settings — the defaults (about one grain per voice), ten
concurrent grains per voice (density 100 Hz, size 100 ms) and the full pool of 100 (density 100 Hz, size 1000 ms, full variation, spray, pan
spread, random direction, a moving playhead) — as ms per 1024-frame step and grain-frames per second. A step is one pg_graph_write_device call
on a caller's stream, timed by a hipEvent pair around the call's launches (pg_grain_kernel, the exact unit kernel that takes its frames, the
mixer sum); medians over the timed steps, behind a warm-up long enough for the pools to fill. The card's clocks while the steps ran are
recorded (bench.py's sampler). Beside them: the single-thread rate of tests/granular_model.py on the same box — a Python model, NOT a target —
and, for the 100-grain case, the bytes the algorithm needs per step against what the time would move at the card's HBM bandwidth (DESIGN.md,
"Granular voices").

    python tools/granular_cost.py [--voices 1024] [--steps 40] [--out profiles/granular_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from phonic_amd import _capi  # noqa: E402
from phonic_amd.graph import Graph  # noqa: E402

SR, MF = 48000, 1024
HBM_BYTES_PER_S = 8.0e12   # MI355X: 8 TB/s HBM3E
SETTINGS = {
    "defaults_1_grain": (dict(), 8),
    "10_grains": (dict(density=100.0, size=100.0, pan_spread=0.5), 12),
    "100_grain_cloud": (dict(density=100.0, size=1000.0, variation=1.0, spray=1.0, pan_spread=1.0, playback_direction=_capi.GRAIN_RANDOM, step=1.0), 96),
}
REC_BYTES = 56 + 72 + 72 + 100 * 80   # sizeof(PgGrainVoice): parameters, pool, pointers and times, 100 grains


def source(n=SR):
    t = np.arange(n, dtype=np.float64) / SR
    return (0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 3.0 * t)).astype(np.float32)


def run(name, voices, steps, matrix=None, before_step=None):
    """matrix: keywords of set_voice_modulation_matrix for every voice (None: no matrix). before_step(g, ids, k, pos): called in front of every
    step's write, outside the timed span (tools/granular_params_cost.py schedules its commands there)."""
    import torch

    kw, warmup = SETTINGS[name]
    g = Graph(SR, 2, MF, 0)
    pcm = source()
    ids = []
    for i in range(voices):
        p = _capi.granular_params(rng_state=(i + 1, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, i * 7919 + 3), position=0.1 + 0.8 * (i % 97) / 97.0, **kw)
        ids.append(g.add_granular_voice(0, pcm, p, volume=0.02, panning=((i % 21) - 10) / 10.0))
        if matrix is not None:
            g.set_voice_modulation_matrix(ids[-1], rng_states=((i + 11, 2, 3, 4), (i + 5, 6, 7, 8)), **matrix)
    stream = torch.cuda.Stream(device=0)
    out = torch.zeros(2 * MF, dtype=torch.float32, device="cuda:0")
    pos = 0
    with torch.cuda.stream(stream):
        for k in range(warmup):
            if before_step:
                before_step(g, ids, k, pos)
            assert g.write_device(out.data_ptr(), 2 * MF, pos, stream.cuda_stream) == 2 * MF
            pos += MF
        stream.synchronize()
        ms = []
        for k in range(steps):
            if before_step:
                before_step(g, ids, warmup + k, pos)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert g.write_device(out.data_ptr(), 2 * MF, pos, stream.cuda_stream) == 2 * MF
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            pos += MF
    probe = ids[:: max(1, voices // 16)]
    active = float(np.mean([int(g.voice_grain_state(v)["active"].sum()) for v in probe]))
    peak = float(out.abs().max().item())
    assert g.device_errors() == 0 and np.isfinite(peak) and peak > 0.0
    g.close()
    ms.sort()
    med = ms[len(ms) // 2]
    return {"ms_per_step_median": med, "ms_per_step_p10": ms[len(ms) // 10], "ms_per_step_p90": ms[(9 * len(ms)) // 10], "warmup_steps": warmup,
            "active_grains_per_voice_at_the_end": active, "grain_frames_per_s": active * voices * MF / (med * 1e-3), "last_step_peak": peak}


def model_rate():
    import granular_model as gm

    m = gm.GrainPool(8000, gm.make_buffer(2048), gm.Params(density=100.0, size=1000.0, variation=1.0, spray=1.0, pan_spread=1.0, playback_direction=gm.RANDOM, step=1.0), (1, 2, 3, 4))
    m.process(8200)   # the pool fills
    t0 = time.perf_counter()
    _, cnt, _ = m.process(1024)
    dt = time.perf_counter() - t0
    return {"what": "tests/granular_model.py, one thread, numpy over the 100 slots of ONE voice: a Python model, not a target", "grain_frames_per_s": float(cnt.sum()) / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "granular_cost.json"))
    a = ap.parse_args()
    import bench

    sampler = bench.ClockSampler(0)
    sampler.start()
    res, spans = {}, []
    for name in SETTINGS:
        t0 = time.perf_counter()
        res[name] = run(name, a.voices, a.steps)
        spans.append((t0, time.perf_counter()))
    sampler.stop()
    try:
        clocks = sampler.summary(spans)
    except Exception as e:  # noqa: BLE001
        clocks = {"note": f"no clock record ({type(e).__name__}: {e})"}
    c = res["100_grain_cloud"]
    # Bytes one step of the 100-grain case has to move: per voice the record in and out, the staged chunk out (pg_grain_kernel) and in
    # (the unit kernel), the unit's output row out and in (the mixer sum); the source buffer (192 KB here, shared by all voices) stays in cache.
    need = a.voices * (2 * REC_BYTES + 4 * MF * 8)
    out = {"workload": f"{a.voices} granular voices on the main mixer, {SR} Hz, steps of {MF} frames", "steps_timed": a.steps,
           "timing": "hipEvent pair around one pg_graph_write_device call per step on a caller's stream; medians", "source_hash": _capi.source_hash(),
           "runs": res, "model": model_rate(), "clocks": clocks,
           "hbm_100_grain_cloud": {"bytes_needed_per_step": need, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
                                   "achieved_fraction_of_hbm_bandwidth": need / (c["ms_per_step_median"] * 1e-3) / HBM_BYTES_PER_S,
                                   "note": "the step is bound by the grains' arithmetic and the serial scheduler / slot walks, not by memory"}}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
