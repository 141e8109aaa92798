"""What changing granular parameters on running voices costs, on top of tools/granular_cost.py (its voices, its pools, its timing: run()): 1024
granular voices on the main mixer at 48 kHz, one-grain pools and full pools, without a matrix and with an empty one, as ms per 1024-frame step —
  no_commands               the voices never receive a command (the case tools/granular_cost.py and tools/modulation_cost.py measure on any tree:
                            run those on the parent commit's tree for the comparison);
  one_command_per_voice     every voice gets one pg_graph_set_voice_granular_parameter (GPOS, two alternating values) per step, due at the
                            step's first frame (no extra chunk cut: the cost of the commands themselves, 1024 in every launch's list);
  mixed_windows             full pools only: every voice gets one GWND per step, cycling through the eight windows. The grains live for tens of
                            steps, so the pool holds grains of all eight windows while one row is staged in LDS: about seven of eight window
                            lookups of phase 3 go to the global table (against one_command_per_voice: the same commands, every lookup in LDS).
The commands are pushed in front of the step's first event, outside the timed span. The cost is reported, not gated.

    python tools/granular_params_cost.py [--voices 1024] [--steps 40] [--out profiles/granular_params_cost.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import granular_cost  # noqa: E402
from phonic_amd import _capi  # noqa: E402

POOLS = ("defaults_1_grain", "100_grain_cloud")
MATRICES = {"no_matrix": None, "empty_matrix": dict()}


def position_commands(g, ids, k, pos):
    for v in ids:
        g.set_voice_granular_parameter(v, "GPOS", 0.3 if k % 2 else 0.6, pos)


def window_commands(g, ids, k, pos):
    for v in ids:
        g.set_voice_granular_parameter(v, "GWND", k % 8, pos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "granular_params_cost.json"))
    a = ap.parse_args()
    import bench

    sampler = bench.ClockSampler(0)
    sampler.start()
    res, spans = {}, []

    def case(pool, matrix, name, before_step):
        t0 = time.perf_counter()
        res.setdefault(pool, {}).setdefault(matrix, {})[name] = granular_cost.run(pool, a.voices, a.steps, matrix=MATRICES[matrix], before_step=before_step)
        spans.append((t0, time.perf_counter()))

    for pool in POOLS:
        for matrix in MATRICES:
            case(pool, matrix, "no_commands", None)
            case(pool, matrix, "one_command_per_voice", position_commands)
    case("100_grain_cloud", "no_matrix", "mixed_windows", window_commands)
    sampler.stop()
    try:
        clocks = sampler.summary(spans)
    except Exception as e:  # noqa: BLE001
        clocks = {"note": f"no clock record ({type(e).__name__}: {e})"}
    for pool in res:
        for matrix, r in res[pool].items():
            for name in ("one_command_per_voice", "mixed_windows"):
                if name in r:
                    r[name]["ms_over_no_commands"] = r[name]["ms_per_step_median"] - r["no_commands"]["ms_per_step_median"]
    out = {"workload": f"{a.voices} granular voices on the main mixer, {granular_cost.SR} Hz, steps of {granular_cost.MF} frames", "steps_timed": a.steps,
           "timing": "tools/granular_cost.py's: hipEvent pair around one pg_graph_write_device call per step on a caller's stream; medians",
           "source_hash": _capi.source_hash(), "runs": res, "clocks": clocks}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
