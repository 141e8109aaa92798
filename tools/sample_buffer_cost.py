"""What sample buffers cost and save (pg_graph_add_sample_buffer, pg_k_sample.hip) —
  conversion   the granular mono buffer of a 10 s stereo 44100 Hz buffer on a 48000 Hz graph: upload, pass A (pg_sample_sched_kernel, the f32
               schedule) and pass B (pg_sample_interp_kernel, Hermite + down-mix) by the library's hipEvents (pg_debug_sample_buffer_times),
               median of 10 runs after 2 warm-ups; beside it the CPU oracle doing the same conversion on one thread of this machine
               (po_cubic_resample in 1024-frame writes + the numpy down-mix), and a check that both give the same samples;
  add_voices   device memory (hipMemGetInfo before - after), PCM bytes requested, the library's allocation count and wall time to build a graph of
               1024 voices of one 2 s stereo sample: pg_graph_add_voice (a private copy each) against one shared buffer +
               pg_graph_add_voice_from_buffer; the same with a 10 s sample, whose copies are large enough for hipMemGetInfo to resolve;
  steady       ms per 1024-frame block of those two 1024-voice graphs (Gain -> Reverb per voice): hipEvent pair around one
               pg_graph_write_device call on a caller's stream, five interleaved legs each (the order inside a pair of legs alternates), the median
               of every leg — once with all voices started together (they read the same frames of the sample at the same time) and once with
               the voices started at different times, each at its own place in the sample.
One timed process; the card's clocks and power are recorded while it runs, as bench.py --full does. Reported, not gated.

    python tools/sample_buffer_cost.py [--voices 1024] [--steps 40] [--out profiles/sample_buffers.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

os.environ["PHONIC_DEBUG_HOOKS"] = "1"   # arms the library's hipEvent timing of the upload and the conversion (pg_debug_sample_buffer_times)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from phonic_amd import _capi, workloads  # noqa: E402
from phonic_amd.graph import Graph, hip_calls  # noqa: E402

SR, MF = 48000, 1024


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def conversion(runs=10, warmups=2, seconds=10.0):
    import oracle

    pcm = workloads.tone_buffer(0, 44100, seconds)
    n_frames = pcm.size // 2
    g = Graph(SR, 2, MF, 0)
    rows = []
    mono = None
    for k in range(warmups + runs):
        t0 = time.perf_counter()
        b = g.add_sample_buffer(pcm, 2, 44100)
        g.prepare_granular_buffer(b)
        wall = (time.perf_counter() - t0) * 1e3
        info = g.sample_buffer_times(b)
        if mono is None:
            mono = g.read_granular_buffer(b)
        g.release_sample_buffer(b)
        if k >= warmups:
            rows.append((info["upload_ms"], info["sched_ms"], info["interp_ms"], wall))
    g.close()
    lib = oracle.lib()
    f32p = C.POINTER(C.c_float)
    cpu = []
    ref = None
    for k in range(warmups + runs):
        out = np.zeros(2 * (mono.size + 2048), np.float32)
        consumed = C.c_size_t(0)
        t0 = time.perf_counter()
        produced = lib.po_cubic_resample(pcm.ctypes.data_as(f32p), pcm.size, 44100, SR, 2, out.ctypes.data_as(f32p), out.size, 2 * 1024, C.byref(consumed))
        ref = _capi.mono_downmix(out[:produced], 2)
        if k >= warmups:
            cpu.append((time.perf_counter() - t0) * 1e3)
    n = min(ref.size, mono.size)
    up, a, b_, wall = (med([r[i] for r in rows]) for i in range(4))
    return {"buffer": f"{seconds:g} s stereo 44100 Hz ({n_frames} frames, {pcm.nbytes / 1e6:.2f} MB) -> 48000 Hz mono", "frames_out": int(mono.size),
            "upload_ms": up, "pass_a_schedule_ms": a, "pass_b_interpolate_ms": b_, "device_total_ms": up + a + b_, "wall_ms_add_and_prepare": wall,
            "cpu_oracle_one_thread_ms": med(cpu), "cpu_oracle_frames_out": int(ref.size),
            "samples_that_differ_from_the_cpu_oracle": int(np.count_nonzero(ref[:n] != mono[:n])), "runs": runs, "warmups": warmups}


STAGGER_FRAMES = 353   # start time of voice i in the staggered graphs: (i % 251) x 353 frames, up to 88250 — one pass through the 2 s sample


def build(shared, voices, pcm, stagger=False):
    """stagger: the voices start at different times (start_time, as a sampler's notes do), so that once all have started every voice reads its
    own place of the sample; without it all voices start together and read the same frames at the same time."""
    import torch

    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    calls0 = hip_calls()
    t0 = time.perf_counter()
    g = Graph(SR, 2, MF, 0)
    vol = workloads.voice_level(voices)
    buf = g.add_sample_buffer(pcm, 2, 44100) if shared else None
    for i in range(voices):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_GAIN, {"gain": 0.9})
        g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
        o = dict(volume=vol, panning=float(np.float32(workloads.voice_pan(i))), has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        if stagger:
            o["start_time"] = (i % 251) * STAGGER_FRAMES
        if shared:
            g.add_voice_from_buffer(m, buf, **o)
        else:
            g.add_voice(m, pcm, 2, 44100, **o)
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    calls1 = hip_calls()
    return g, {"seconds_to_build": dt, "device_bytes": int(free0 - free1), "pcm_bytes_requested": int(pcm.nbytes * (1 if shared else voices)),
               "device_allocations": int(calls1["alloc"] - calls0["alloc"]), "blocking_copies": int(calls1["blocking_copy"] - calls0["blocking_copy"])}


def leg(g, stream, out, pos, steps):
    import torch

    ms = []
    with torch.cuda.stream(stream):
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert g.write_device(out.data_ptr(), 2 * MF, pos, stream.cuda_stream) == 2 * MF
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            pos += MF
    return med(ms), pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_buffers.json"))
    a = ap.parse_args()
    import bench
    import torch

    torch.zeros(1, device="cuda:0")
    sampler = bench.ClockSampler(0)
    sampler.start()
    t_all = time.perf_counter()
    conv = conversion()
    pcm = workloads.tone_buffer(0, 44100, 2.0)
    gp, add_private = build(False, a.voices, pcm)
    gs, add_shared = build(True, a.voices, pcm)
    stream = torch.cuda.Stream(device=0)

    def steady_legs(gp, gs, warmup):
        """`legs` pairs of legs, the order inside a pair alternating (private first, then shared first, ...)."""
        outs = {k: torch.zeros(2 * MF, dtype=torch.float32, device="cuda:0") for k in ("private", "shared")}
        graphs, pos, legs = {"private": gp, "shared": gs}, {"private": 0, "shared": 0}, {"private": [], "shared": []}
        for k in graphs:   # warm-up: topology upload, the first blocks' deferrals, (staggered) every voice started
            _, pos[k] = leg(graphs[k], stream, outs[k], pos[k], warmup)
        for i in range(a.legs):
            for k in (("private", "shared") if i % 2 == 0 else ("shared", "private")):
                m, pos[k] = leg(graphs[k], stream, outs[k], pos[k], a.steps)
                legs[k].append(m)
        stream.synchronize()
        same = bool(torch.equal(outs["private"], outs["shared"]))
        assert gp.device_errors() == 0 and gs.device_errors() == 0
        gp.close()
        gs.close()
        r = {k: {"ms_per_block_leg_medians": v, "median": med(v), "min": min(v), "max": max(v)} for k, v in legs.items()}
        r["shared_at_or_below_private_max"] = r["shared"]["median"] <= r["private"]["max"]
        r["shared_over_private"] = r["shared"]["median"] / r["private"]["median"]
        r["last_block_identical"] = same
        return r

    steady = steady_legs(gp, gs, 16)
    # the same with the voices started at different times: behind the warm-up every voice plays, each at its own place in the sample
    gp2, gs2 = build(False, a.voices, pcm, stagger=True)[0], build(True, a.voices, pcm, stagger=True)[0]
    steady_staggered = steady_legs(gp2, gs2, 250 * STAGGER_FRAMES // MF + 8)
    # the same two graphs with a 10 s sample (3.5 MB a copy): hipMemGetInfo resolves copies of that size; it did not resolve the 0.7 MB copies of
    # the 2 s sample (both graphs read the same 2.26 GB)
    long_pcm = workloads.tone_buffer(0, 44100, 10.0)
    add_long = {}
    for name, shared in (("private_copies", False), ("shared_buffer", True)):
        gl, add_long[name] = build(shared, a.voices, long_pcm)
        gl.close()
    spans = [(t_all, time.perf_counter())]
    sampler.stop()
    try:
        clocks = sampler.summary(spans)
    except Exception as e:  # noqa: BLE001
        clocks = {"note": f"no clock record ({type(e).__name__}: {e})"}
    out = {"conversion": conv,
           "add_voices": {"what": f"{a.voices} voices of one 2 s stereo 44100 Hz sample ({pcm.nbytes / 1e6:.2f} MB), Gain -> Reverb per voice; device_bytes = hipMemGetInfo before - after (whole graph)",
                          "private_copies": add_private, "shared_buffer": add_shared, "bytes_saved": add_private["device_bytes"] - add_shared["device_bytes"],
                          "with_a_10_s_sample": {"sample_mb": long_pcm.nbytes / 1e6, **add_long, "bytes_saved": add_long["private_copies"]["device_bytes"] - add_long["shared_buffer"]["device_bytes"]}},
           "steady": {"what": f"ms per {MF}-frame block, hipEvent pair around pg_graph_write_device, {a.legs} interleaved legs of {a.steps} steps each (the order inside a pair alternates); all voices start together: they read the same frames of the sample at the same time", **steady},
           "steady_staggered": {"what": f"the same with voice i started at frame (i % 251) x {STAGGER_FRAMES} (start_time): behind the warm-up every voice plays, each at its own place in the sample", **steady_staggered},
           "source_hash": _capi.source_hash(), "clocks": clocks}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
