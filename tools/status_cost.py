"""What playback status events cost: the headline graph at 1024 voices (phonic_amd.workloads.build_headline) rendered three ways on the same
build — status never enabled, enabled with no voice reporting, every voice reporting at the reference's default emit rate of one second
(FilePlaybackOptions::default, src/source/file.rs) with Stopped records — in two call patterns: one synchronous pg_graph_write per 1024-frame
block (a real-time host), and calls of 16 blocks with super-block launches allowed (an offline pull loop). A graph with a voice that reports
renders chunk by chunk, pg_playback_status_kernel behind every piece ("Playback status"): the second pattern shows what leaving the
launches of several blocks costs, the first what the extra launch per piece does.

    python tools/status_cost.py [--voices 1024] [--blocks 64] [--warmup 16] [--out profiles/status_events.json]
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


def run(mode, voices, blocks, warmup, per_call):
    g = Graph(SR, 2, MF, 0)
    g.set_max_blocks_per_launch(per_call)
    if mode != "none":
        g.enable_status(1 << 16)
    workloads.build_headline(g, n_voices=voices)
    if mode == "reporting":
        for v in range(voices):
            g.set_voice_status(v, 1.0, True)
    buf = np.zeros(2 * MF * per_call, dtype=np.float32)
    pos, records = 0, 0
    for _ in range(warmup):
        g.write(buf, pos)
        pos += MF * per_call
    times = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        g.write(buf, pos)
        times.append((time.perf_counter() - t0) * 1e3 / per_call)
        pos += MF * per_call
        if mode != "none":
            records += len(g.poll_status(4096))   # (outside the timed span: what a binding's event thread does)
    dropped = g.status_dropped() if mode != "none" else 0
    peak = float(np.abs(buf).max())
    assert g.device_errors() == 0 and np.isfinite(buf).all()
    g.close()
    times.sort()
    return {"ms_per_block_median": times[len(times) // 2], "ms_per_block_p10": times[len(times) // 10], "ms_per_block_p90": times[(9 * len(times)) // 10],
            "records_polled": records, "dropped": dropped, "last_block_peak": peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "status_events.json"))
    a = ap.parse_args()
    out = {"workload": "headline", "voices": a.voices, "block_frames": MF, "calls_timed": a.blocks, "warmup_calls": a.warmup, "emit_rate_seconds": 1.0,
           "timing": "wall clock of synchronous pg_graph_write calls (the call returns when its frames are on the host), per 1024-frame block",
           "source_hash": _capi.source_hash(), "patterns": {}}
    for name, per_call in (("one_block_per_call", 1), ("sixteen_blocks_per_call", 16)):
        res = {m: run(m, a.voices, a.blocks, a.warmup, per_call) for m in ("none", "enabled", "reporting")}
        base = res["none"]["ms_per_block_median"]
        out["patterns"][name] = {"runs": res, "ratio_enabled_over_none": res["enabled"]["ms_per_block_median"] / base,
                                 "ratio_reporting_over_none": res["reporting"]["ms_per_block_median"] / base}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
