"""The effects' time-parallel paths at their eligibility and chunk edges, on the device against the oracle at the same mixer rate.

The cases are the table of tests/effect_edge_cases.py (derived from the restated rules; tests/test_effect_edge_cases.py proves on the CPU that each
is a sharp one: the nearest wrong variant is at least 10 x this file's tolerance away). Every case runs in up to three placements, because
`fc.tmp_floats`, the workgroup size and the LDS arena differ between the kernels, and the chunk cap of delay_fast, the ramp paths' `cap` and
chorus_ramp_fast's `nt == 256` depend on them:

  1. the standalone Effect handle, with the index log armed for Delay / Chorus / Reverb: where the table expects the time-parallel path every slot
     must be written, where it expects the serial path none; logged indices are compared with the oracle's under INDEX_FLIP_RATE_MAX;
  2. on a sub-mixer with one looping voice — alone (pg_unit_kernel_fast_mid / _fast_wide) and in front of a Reverb under set_staged(1 / 2 / 0)
     (pg_stage_fused_wide_kernel, the per-stage kernels, the fused kernel): the three agree to 2e-6, each matches the oracle, and
     deferred_units() says which path the unit took: 0 where the rule picks the time-parallel path, 1 where it picks the serial one;
  3. on the main mixer's bus (pg_unit_kernel), written four blocks per call and block by block.

Placements 2 and 3 take the edge cases only, not the rate sweep. Tolerance: RMS <= 1e-5 x scale, max <= 1e-4 x scale, scale = max(1, max |oracle|)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import effect_edge_cases as ec
import oracle

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5
MAX_TOL = 1e-4
STAGED_AGREE = 2e-6
INDEX_FLIP_RATE_MAX = 1e-4


def _record(case, placement, rms, mx, scale, **more):
    """One line per comparison: printed, and appended to the file PHONIC_EDGE_FIGURES names (docs/parity_findings.md quotes the worst per group)."""
    line = dict(case=case.id, group=case.group, placement=placement, rms=rms, max=mx, scale=scale, **more)
    print(json.dumps(line))
    path = os.environ.get("PHONIC_EDGE_FIGURES")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(line) + "\n")


def check(case, placement, got, want, **more):
    assert np.isfinite(got).all(), f"{case.id} [{placement}]: non-finite output"
    scale = max(1.0, float(np.abs(want).max()))
    rms, mx = ec.diff_figures(got, want)
    _record(case, placement, rms, mx, scale, **more)
    assert rms <= RMS_TOL * scale, f"{case.id} [{placement}]: rms {rms:.3e} (scale {scale:.3f})"
    assert mx <= MAX_TOL * scale, f"{case.id} [{placement}]: max {mx:.3e} (scale {scale:.3f})"


def standalone(case):
    import phonic_amd

    want, want_logs = ec.run_oracle(case, with_log=True) if case.kind in ec.INDEX_WORDS_PER_FRAME else (ec.run_oracle(case), [])
    e = phonic_amd.Effect(case.kind, case.params, case.seeds)
    lib = e._lib

    def begin(words):
        assert lib.pg_effect_debug_index_log(e._h, None, words) == 0

    def end(words):
        buf = np.zeros(words, np.int32)
        assert lib.pg_effect_debug_index_log(e._h, buf.ctypes.data_as(C.POINTER(C.c_int32)), words) == 0
        return buf

    got, got_logs = ec.run_effect(e, case, log_begin=begin, log_end=end)
    more = {}
    if got_logs:
        g, w = np.concatenate(got_logs), np.concatenate(want_logs)
        written = g >= 0
        if case.path == "fast":
            assert written.all(), f"{case.id}: the rule picks the time-parallel path, but {int((~written).sum())} of {g.size} reads were not logged"
        elif case.path == "serial":
            assert not written.any(), f"{case.id}: the rule picks the serial path, but {int(written.sum())} of {g.size} reads were logged"
        reads = int(written.sum())
        flips = int((g[written] != w[written]).sum())
        more = dict(reads=reads, flips=flips)
        assert flips <= int(np.floor(INDEX_FLIP_RATE_MAX * reads)), f"{case.id}: {flips} index flips in {reads} logged reads"
    check(case, "standalone", got, want, **more)


def in_graphs(case):
    from phonic_amd.graph import Graph

    x = ec.make_signal(case)
    max_frames = max(1, min(1024, max(case.block_sizes())))

    def render(placement, staged=None, blocks_per_write=1, on_oracle=False):
        g = oracle.OracleGraph(case.sr, 2, max_frames) if on_oracle else Graph(case.sr, 2, max_frames, 0)
        if not on_oracle:
            if staged is not None:
                g.set_staged(staged)
            if blocks_per_write > 1:
                g.set_max_blocks_per_launch(blocks_per_write)
        fx = ec.build_graph(g, case, placement, x)
        out = ec.render_graph(g, case, fx, blocks_per_write)
        if not on_oracle:
            assert g.device_errors() == 0, f"{case.id} [{placement}]: device_errors {g.device_errors()}"
            deferred[placement, staged, blocks_per_write] = g.deferred_units()
        g.close()
        return out

    deferred = {}
    want = render("sub", on_oracle=True)
    assert float(np.abs(want).max()) > 1e-3
    got = render("sub")
    check(case, "sub", got, want, deferred=deferred["sub", None, 1])
    # units the time-parallel kernels handed to the exact serial kernel in the last block: none where the rule picks the time-parallel path, this
    # one where it picks the serial path — the only view of the path inside a graph, and the only one at all for the Compressor
    def path_taken(key):
        if case.path == "fast":
            assert deferred[key] == 0, f"{case.id} {key}: the rule picks the time-parallel path, the sub-mixer's unit was deferred"
        elif case.path == "serial":
            assert deferred[key] >= 1, f"{case.id} {key}: the rule picks the serial path, the sub-mixer's unit was not deferred"

    path_taken(("sub", None, 1))
    want = render("sub_reverb", on_oracle=True)
    outs = {mode: render("sub_reverb", staged=mode) for mode in (1, 2, 0)}
    for mode in (1, 2, 0):
        check(case, f"sub_reverb_staged{mode}", outs[mode], want, deferred=deferred["sub_reverb", mode, 1])
        path_taken(("sub_reverb", mode, 1))
    for a, b in ((1, 2), (1, 0)):
        d = float(np.abs(outs[a] - outs[b]).max())
        assert d <= STAGED_AGREE, f"{case.id}: set_staged({a}) and set_staged({b}) differ by {d:.3e}"
    # (the oracle is written with the same calls: the Chorus re-seats its oscillators on a phase it advances once per process call while rate or
    # phase ramp, so its output depends on where the calls end)
    got = render("main", blocks_per_write=4)
    check(case, "main_four_blocks_per_write", got, render("main", blocks_per_write=4, on_oracle=True), deferred=deferred["main", None, 4])
    got = render("main")
    check(case, "main_block_by_block", got, render("main", on_oracle=True), deferred=deferred["main", None, 1])


def run(case):
    standalone(case)
    if case.edge:
        in_graphs(case)


def _param(group):
    cs = ec.cases(group)
    return pytest.mark.parametrize("case", cs, ids=[c.id for c in cs])


@_param("comp")
def test_compressor_and_limiter_window_edges(case):
    """Look-ahead windows on both sides of every rule of comp_fast_eligible, once as a compressor (ratio 4, knee 6) and once as a limiter (ratio 20,
    knee 0), on noise with isolated loud peaks further apart than the window (the tracked peak expires and the window is rescanned). The Compressor
    has no index log: the PAIR of cases either side of an edge is the proof. Powers of two (8, 64, 128, 512) and everything above 3073 frames
    (3074, 3840 = the default at 96 kHz) take the serial path; 9, 49, 65, 127, 129, 511, 513, 1600, 1764 (the default at 44.1 kHz) and 3073 the
    time-parallel one, where 65 / 129 / 513 end the doubling with a combine that overlaps all but one entry. The hand-over cases change `look`
    across 3073 / 3074 and back while a peak is tracked."""
    run(case)


@_param("delay")
def test_delay_eligibility_and_chunk_edges(case):
    """The Delay one f32 either side of the 66-sample bound at 8, 22.05, 44.1 and 48 kHz (below: serial, at: time-parallel with 65-frame chunks whose
    last frame reads the last frame written before the chunk), at the parameter's minimum at 96 / 192 kHz, at the upper bound mask - 8 on a ring
    that the longest delay nearly fills, LFO -> time at depth +-1 either side of what the 1 % margin admits for the five periodic shapes in both
    routing modes, feedback-only and filter-only modulation at the lower edge (t_max from the unmodulated branch), and ramps of `dlay` and `lfdt`
    across the edge at 8 kHz (over inside one piece) and 192 kHz (several blocks). The index log confirms the path the rule picks."""
    run(case)


@_param("chorus")
def test_chorus_eligibility_edges(case):
    """The Chorus one f32 either side of floorf(2 + delay) >= 66 at the four lower rates, at dlay = 0 (always serial), at dlay 100 ms with depth 1
    (the longest lag the ring is sized for: still below mask - 8, time-parallel, at 8 / 44.1 / 192 kHz), `dlay` ramps across the lower edge in both
    directions, and rate / phase ramps that end inside a piece of at most 16 frames at 8 kHz. The index log confirms the path the rule picks."""
    run(case)


@_param("nyquist")
def test_cutoffs_at_nyquist(case):
    """Filter, Eq5, the Delay's feedback filter and the Chorus's pre-filter with their cutoff clamped to sr / 2: the Filter as new() makes it (its
    coefficients are those of 44 100 Hz until initialize() moves the cutoff), `cuto` set to its maximum mid-run for each of the four filter types
    (coefficients at tan(pi / 2)), `frq5` / `cuto` / `fltf` at their maxima at 22.05 kHz, and a cutoff ramp that crosses the clamp. Filter and Eq5
    have no index log; the CPU test shows that a cutoff 10 % short of the clamp, or the other rate's clamp, is 10 x the tolerance away."""
    run(case)


@_param("sweep")
def test_every_effect_at_every_rate(case):
    """Every effect, by default and with one with_parameters set, at 8, 22.05, 44.1, 96 and 192 kHz over ragged block sizes (empty, one frame, 4096)
    with a parameter ramp that starts mid-run: ramp lengths, envelope times, ring sizes and clamps all scale with the rate. Standalone handle only."""
    run(case)
