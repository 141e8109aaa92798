"""What a volume envelope costs today: the headline graph at 1024 voices (phonic_amd.workloads.build_headline), rendered three ways on the same
build — no envelopes (the staged kernels), every voice enveloped and in Sustain, every voice enveloped and in a moving stage (a long attack) —
as ms per 1024-frame block and the two ratios. A unit with a living enveloped voice is rendered by the exact kernel, one workgroup per CU
("Volume envelopes"); moving such voices into the staged kernels is what this number is for.

    python tools/ahdsr_cost.py [--voices 1024] [--blocks 64] [--warmup 16] [--out profiles/ahdsr_cost.json]
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


def run(mode, voices, blocks, warmup):
    g = Graph(SR, 2, MF, 0)
    workloads.build_headline(g, n_voices=voices)
    if mode == "sustain":      # no attack, hold or decay: Sustain from the first frame on (the constant path: one multiply per sample)
        for v in range(voices):
            g.set_voice_envelope(v, attack_s=0.0, hold_s=0.0, decay_s=0.0, sustain_level=0.75)
    elif mode == "moving":     # an attack longer than the run: the per-frame walk on every block
        for v in range(voices):
            g.set_voice_envelope(v, attack_s=60.0)
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
    stage = g.voice_envelope_stage(0)
    deferred = g.deferred_units()
    peak = float(np.abs(buf).max())
    assert g.device_errors() == 0 and np.isfinite(buf).all()
    g.close()
    times.sort()
    return {"ms_per_block_median": times[len(times) // 2], "ms_per_block_p10": times[len(times) // 10], "ms_per_block_p90": times[(9 * len(times)) // 10],
            "stage_of_voice_0": stage, "deferred_units": deferred, "last_block_peak": peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ahdsr_cost.json"))
    a = ap.parse_args()
    res = {m: run(m, a.voices, a.blocks, a.warmup) for m in ("none", "sustain", "moving")}
    base = res["none"]["ms_per_block_median"]
    out = {"workload": "headline", "voices": a.voices, "block_frames": MF, "blocks_timed": a.blocks, "warmup_blocks": a.warmup,
           "timing": "wall clock of synchronous pg_graph_write calls of one block each (the call returns when the block is on the host)",
           "source_hash": _capi.source_hash(), "runs": res,
           "ratio_sustain_over_none": res["sustain"]["ms_per_block_median"] / base, "ratio_moving_over_none": res["moving"]["ms_per_block_median"] / base}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
