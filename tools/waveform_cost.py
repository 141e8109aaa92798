"""What a waveform overview costs (pg_graph_sample_buffer_waveform, pg_k_waveform.hip): a 2^22-frame stereo buffer (32 MB) on the device, overviews
of the whole buffer at resolutions 16, 1024 and 4096 in both modes —
  kernel_ms    the call's kernels by the library's hipEvents on the graph's stream (pg_debug_sample_buffer_waveform_time), warm: the median of
               `--runs` calls after `--warmups`; bytes read / that time, and that as a fraction of the 8 TB/s peak;
  call_ms      the whole call as the host sees it (waits, the staging allocation, the launches, the copy of the points to the host, the release);
  ratio        resolution 16 against resolution 4096 on the same buffer: few long buckets are split over workgroups, so it should stay near 1 —
               a ratio of more than a few would say the split rule is not doing its job.
Every overview is compared with tests/waveform_model.py before it is timed. One timed process; the card's clocks are recorded while it runs, as
bench.py --full does. Nobody has measured this before and there is no parent to compare with: reported, not gated.

    python tools/waveform_cost.py [--frames 4194304] [--runs 20] [--out profiles/waveform_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ["PHONIC_DEBUG_HOOKS"] = "1"   # arms the library's hipEvent timing (pg_debug_sample_buffer_waveform_time)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from phonic_amd import _capi  # noqa: E402
from phonic_amd.graph import Graph  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def med(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waveform_cost.json"))
    a = ap.parse_args()
    import waveform_model as W

    sampler = None
    try:
        import bench
        import torch

        torch.zeros(1, device="cuda:0")
        sampler = bench.ClockSampler(0)
        sampler.start()
    except Exception as e:  # noqa: BLE001
        print(f"no clock record ({type(e).__name__}: {e})", file=sys.stderr)
    t_all = time.perf_counter()
    pcm = np.random.default_rng(1).uniform(-1.0, 1.0, 2 * a.frames).astype(np.float32)
    g = Graph(48000, 2, 1024, 0)
    buf = g.add_sample_buffer(pcm, 2, 44100)
    rows = []
    for mode in ("mixed_down", "multi_channel"):
        for res in (16, 1024, 4096):
            want = W.waveform(pcm, 2, 44100, res, mode)
            kernel, call = [], []
            for k in range(a.warmups + a.runs):
                t0 = time.perf_counter()
                got = g.sample_buffer_waveform(buf, res, mode=mode)
                wall = (time.perf_counter() - t0) * 1e3
                if k == 0:
                    assert all(np.array_equal(got[key], want[key]) for key in want), (mode, res)
                if k >= a.warmups:
                    kernel.append(g.sample_buffer_waveform_time(buf))
                    call.append(wall)
            ms = med(kernel)
            rows.append({"mode": mode, "resolution": res, "frames_per_bucket": a.frames / res, "kernel_ms": ms, "kernel_ms_min": min(kernel), "kernel_ms_max": max(kernel),
                         "call_ms": med(call), "bytes_read": int(pcm.nbytes), "bytes_per_s": pcm.nbytes / (ms * 1e-3) if ms > 0 else None,
                         "fraction_of_8_TB_per_s": pcm.nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S if ms > 0 else None})
    assert g.device_errors() == 0
    g.close()
    clocks = {"note": "no clock record"}
    if sampler is not None:
        sampler.stop()
        try:
            clocks = sampler.summary([(t_all, time.perf_counter())])
        except Exception as e:  # noqa: BLE001
            clocks = {"note": f"no clock record ({type(e).__name__}: {e})"}
    by = {(r["mode"], r["resolution"]): r["kernel_ms"] for r in rows}
    out = {"what": f"pg_graph_sample_buffer_waveform over a {a.frames}-frame stereo buffer ({pcm.nbytes / 1e6:.1f} MB), the whole buffer; kernel_ms: hipEvents around the call's kernels on the graph's stream, "
                   f"median of {a.runs} warm calls; call_ms: the host's wall time of the call (python wrapper included); every overview equals tests/waveform_model.py",
           "rows": rows,
           "resolution_16_over_4096": {m: (by[(m, 16)] / by[(m, 4096)] if by[(m, 4096)] > 0 else None) for m in ("mixed_down", "multi_channel")},
           "source_hash": _capi.source_hash(), "clocks": clocks}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
