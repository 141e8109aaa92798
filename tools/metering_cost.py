"""What level metering costs: the headline graph at 1024 voices (phonic_amd.workloads.build_headline: 1024 sub-mixers, one meter each, plus
the main mixer's), rendered three ways on the same build — metering off, on with a 50 ms interval (a record per block, a publish every third
block), on with interval 0 (a publish per record) — as ms per 1024-frame block and the ratios on / off. The meter reads every sub-mixer's
output row once more (1024 x 8 KB = 8 MB per block on top of the ~444 MB the block already moves) in one extra launch per launch sequence,
plus one workgroup for the main mixer's record per call ("Level metering").

    python tools/metering_cost.py [--voices 1024] [--blocks 64] [--warmup 16] [--out profiles/metering_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phonic_amd import _capi, workloads  # noqa: E402
from phonic_amd.graph import Graph  # noqa: E402

SR, MF = 48000, 1024
MODES = {"off": None, "on_50ms": 0.05, "on_interval_0": 0.0}


def run(mode, voices, blocks, warmup):
    g = Graph(SR, 2, MF, 0)
    workloads.build_headline(g, n_voices=voices)
    if MODES[mode] is not None:
        g.set_metering(MODES[mode])
    buf = np.zeros(2 * MF, dtype=np.float32)
    pos = 0
    for _ in range(warmup):
        g.write(buf, pos)
        pos += MF
    times = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        g.write(buf, pos)
        times.append((time.perf_counter() - t0) * 1e3)
        pos += MF
    res = {"last_block_peak": float(np.abs(buf).max())}
    if MODES[mode] is not None:
        main, sub = g.audio_level(0), g.audio_level(1)
        res.update(main_peak=main.peak, main_rms=main.rms, mixer_1_peak=sub.peak, mixer_1_rms=sub.rms)
        assert max(main.peak) > 0.0 and max(sub.peak) > 0.0
    assert g.device_errors() == 0 and np.isfinite(buf).all()
    g.close()
    times.sort()
    res.update(ms_per_block_median=times[len(times) // 2], ms_per_block_p10=times[len(times) // 10], ms_per_block_p90=times[(9 * len(times)) // 10])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metering_cost.json"))
    a = ap.parse_args()
    res = {m: run(m, a.voices, a.blocks, a.warmup) for m in MODES}
    base = res["off"]["ms_per_block_median"]
    out = {"workload": "headline", "voices": a.voices, "block_frames": MF, "blocks_timed": a.blocks, "warmup_blocks": a.warmup,
           "timing": "wall clock of synchronous pg_graph_write calls of one block each (the call returns when the block is on the host)",
           "source_hash": _capi.source_hash(), "runs": res,
           "ratio_on_50ms_over_off": res["on_50ms"]["ms_per_block_median"] / base, "ratio_on_interval_0_over_off": res["on_interval_0"]["ms_per_block_median"] / base}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
