"""What the modulation matrix of granular voices costs: 1024 granular voices on the main mixer at 48 kHz, one-grain pools (the defaults) and full
pools (the 100-grain cloud of tools/granular_cost.py), each in three configurations — without a matrix, with an empty matrix (the LFOs run, all
seven sums are 0.0) and with all 28 routes — as ms per 1024-frame step. A step is one pg_graph_write_device call on a caller's stream, timed by a
hipEvent pair around the call's launches; medians over the timed steps behind a warm-up long enough for the pools to fill. The card's clocks
while the steps ran are recorded (bench.py's sampler). The cost is reported, not gated. With --resources the kernels' resource listing
(tools/check_kernel_resources.py --print) is written beside it.

    python tools/modulation_cost.py [--voices 1024] [--steps 40] [--out profiles/modulation_cost.json] [--resources profiles/modulation_kernel_resources.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phonic_amd import _capi  # noqa: E402
from phonic_amd.graph import Graph  # noqa: E402

SR, MF = 48000, 1024
POOLS = {
    "1_grain": (dict(), 8),
    "100_grain_cloud": (dict(density=100.0, size=1000.0, variation=1.0, spray=1.0, pan_spread=1.0, playback_direction=_capi.GRAIN_RANDOM, step=1.0), 96),
}
# amounts small enough that the modulated cloud stays a full pool (density and size move by a few per cent)
ALL_ROUTES = [(s, t, [0.05, -0.05, 0.03][(s + t) % 3], (s * 7 + t) % 2 == 0) for s in range(_capi.MOD_SOURCES) for t in range(_capi.MOD_TARGETS)]
MATRICES = {"no_matrix": None, "empty_matrix": dict(), "all_28_routes": dict(rates=(5.0, 0.7), waveforms=(0, 6), velocity=0.8, note=72, routes=ALL_ROUTES)}


def source(n=SR):
    t = np.arange(n, dtype=np.float64) / SR
    return (0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 3.0 * t)).astype(np.float32)


def run(pool, matrix, voices, steps):
    import torch

    kw, warmup = POOLS[pool]
    g = Graph(SR, 2, MF, 0)
    pcm = source()
    ids = []
    for i in range(voices):
        p = _capi.granular_params(rng_state=(i + 1, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, i * 7919 + 3), position=0.1 + 0.8 * (i % 97) / 97.0, **kw)
        v = g.add_granular_voice(0, pcm, p, volume=0.02, panning=((i % 21) - 10) / 10.0)
        if MATRICES[matrix] is not None:
            g.set_voice_modulation_matrix(v, rng_states=((i + 11, 2, 3, 4), (i + 5, 6, 7, 8)), **MATRICES[matrix])
        ids.append(v)
    stream = torch.cuda.Stream(device=0)
    out = torch.zeros(2 * MF, dtype=torch.float32, device="cuda:0")
    pos = 0
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            assert g.write_device(out.data_ptr(), 2 * MF, pos, stream.cuda_stream) == 2 * MF
            pos += MF
        stream.synchronize()
        ms = []
        for _ in range(steps):
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
    return {"ms_per_step_median": ms[len(ms) // 2], "ms_per_step_p10": ms[len(ms) // 10], "ms_per_step_p90": ms[(9 * len(ms)) // 10], "warmup_steps": warmup,
            "active_grains_per_voice_at_the_end": active, "last_step_peak": peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modulation_cost.json"))
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    import bench

    sampler = bench.ClockSampler(0)
    sampler.start()
    res, spans = {}, []
    for pool in POOLS:
        res[pool] = {}
        for matrix in MATRICES:
            t0 = time.perf_counter()
            res[pool][matrix] = run(pool, matrix, a.voices, a.steps)
            spans.append((t0, time.perf_counter()))
    sampler.stop()
    try:
        clocks = sampler.summary(spans)
    except Exception as e:  # noqa: BLE001
        clocks = {"note": f"no clock record ({type(e).__name__}: {e})"}
    for pool in POOLS:
        base = res[pool]["no_matrix"]["ms_per_step_median"]
        for matrix in ("empty_matrix", "all_28_routes"):
            res[pool][matrix]["ms_over_no_matrix"] = res[pool][matrix]["ms_per_step_median"] - base
            res[pool][matrix]["ratio_to_no_matrix"] = res[pool][matrix]["ms_per_step_median"] / base
    out = {"workload": f"{a.voices} granular voices on the main mixer, {SR} Hz, steps of {MF} frames", "steps_timed": a.steps,
           "timing": "hipEvent pair around one pg_graph_write_device call per step on a caller's stream; medians", "source_hash": _capi.source_hash(),
           "runs": res, "clocks": clocks}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if a.resources:
        listing = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py"), "--print"], check=True, capture_output=True, text=True).stdout
        with open(a.resources, "w") as fh:
            fh.write("# python tools/check_kernel_resources.py --print, source hash " + _capi.source_hash() + "\n" + listing)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
