"""Nested mixers past the 64-call budget (PG_MAX_CALLS, pg_dev.h): a parent's events cut one chunk of the main mixer into 63 / 64 / 65 / 130
calls of its child. The host ends the chunk at every 64th cut (pg_host.hip), the device keeps one `audible` bit per call (pg_unit_body.inl), the
meter sizes its records by the same number (pg_k_meter.hip) and a deferred bus chain must walk the grid the write walked. The scenarios
(tests/call_budget_scenarios.py, pre-checked on the CPU by tests/test_call_budget_scenarios.py) put the reference's per-call decisions — the
child's silence gate, the bypass of the parent's chain — at chosen calls of that chunk; what such a decision changes lies below 1e-3, so next to
the tolerances the tests compare WHERE the bus is exactly zero: a decision that moves by one call moves that by one call."""
import time

import numpy as np
import pytest

import call_budget_scenarios as cb
import oracle
from metering_model import AudioLevelState, interval_frames, ulp_distance

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_bus(sc):
    """The oracle's render of a scenario: computed once, shared, read-only."""
    if sc.name not in _ORACLE:
        bus = sc.render(oracle.OracleGraph(cb.SR, 2, sc.max_frames))
        bus.setflags(write=False)
        _ORACLE[sc.name] = bus
    return _ORACLE[sc.name]


def gpu_graph(sc):
    from phonic_amd.graph import Graph

    return Graph(cb.SR, 2, sc.max_frames, 0)


def compare(a, b, rms_tol=1e-5, max_tol=1e-4):
    """tests/test_gpu_graph.py: compare()."""
    assert np.isfinite(a).all()
    d = a.astype(np.float64) - b.astype(np.float64)
    rms = float(np.sqrt(np.mean(d * d)))
    assert rms <= rms_tol, f"rms {rms}"
    assert float(np.abs(d).max()) <= max_tol, f"max {np.abs(d).max()}"
    return rms


def zero_mask_report(a, b):
    """Where the exact zeros of two buses differ: (frames that differ, first, last) — for the assertion message."""
    d = np.nonzero(((a == 0) != (b == 0)).reshape(-1, 2).any(axis=1))[0]
    return (int(d.size), int(d[0]), int(d[-1])) if d.size else (0, -1, -1)


@pytest.mark.parametrize("sc", cb.SCENARIOS, ids=lambda s: s.name)
def test_parity_and_exact_zeros(sc):
    """Every scenario without a main chain against the oracle: the tolerances of tests/test_gpu_graph.py, and the same exact zeros."""
    g = gpu_graph(sc)
    t0 = time.perf_counter()
    a = sc.render(g)
    b = oracle_bus(sc)
    print(sc.name, "gpu render s", round(time.perf_counter() - t0, 3), "zero onset gpu", cb.zero_onset(a), "oracle", cb.zero_onset(b), "mask diff", zero_mask_report(a, b))
    assert np.abs(b).max() > 1e-2
    compare(a, b)
    assert np.array_equal(a == 0, b == 0), (cb.zero_onset(a), cb.zero_onset(b), zero_mask_report(a, b))
    assert g.device_errors() == 0


def deferred_render(sc):
    """One graph, bus chain deferred: write_device + export_audible + process_bus_device with the exported words, call by call
    (test_deferred_bus_words_follow_the_pieces_when_events_cut_the_call, part (a)). -> (bus, words per call, every word's value)."""
    import torch

    L = sc.call_frames
    g = gpu_graph(sc)
    g.set_defer_bus(True)
    ids = sc.build(g)
    buf = torch.zeros(2 * L + 256, dtype=torch.float32, device="cuda:0")
    flags_ptr = buf.data_ptr() + 4 * 2 * L
    out = np.zeros((sc.n_calls, 2 * L), np.float32)
    n_words, values = [], []
    for b in range(sc.n_calls):
        sc.schedule(g, ids, b * L, (b + 1) * L)
        buf.zero_()
        w = g.write_device(buf.data_ptr(), 2 * L, b * L)
        g.synchronize()
        assert w == 2 * L
        nw = g.audible_words()
        assert 1 <= nw <= 256
        g.export_audible(flags_ptr, nw)
        g.synchronize()
        values.extend(buf[2 * L: 2 * L + nw].cpu().numpy().tolist())
        g.process_bus_device(buf.data_ptr(), 2 * L, b * L, flags_ptr=flags_ptr, n_words=nw)
        g.synchronize()
        out[b] = buf[: 2 * L].cpu().numpy()
        n_words.append(nw)
    assert g.device_errors() == 0
    return out.reshape(-1), n_words, values


@pytest.mark.parametrize("sc", cb.MAIN_CHAIN_SCENARIOS, ids=lambda s: s.name)
def test_deferred_bus_equals_self_rendered_bus(sc):
    """Gain -> Delay on the main mixer, 64 / 130 cuts in the chunk in which the main mixer's gate on P expires: the bus chain run by the caller
    behind a deferred write equals the graph rendering its own bus, BIT FOR BIT — the chunk that the call budget ends early has words of its
    own, and the chain must consume them on the grid the write walked."""
    g = gpu_graph(sc)
    own = sc.render(g)
    assert g.device_errors() == 0
    deferred, n_words, values = deferred_render(sc)
    pieces = -(-sc.call_frames // sc.max_frames)
    print(sc.name, "words per call", n_words, "zero onset own", cb.zero_onset(own), "deferred", cb.zero_onset(deferred))
    assert n_words[sc.target] > pieces and n_words[sc.target] > 1, n_words       # the budget's cut added words to the call
    assert n_words[2] == pieces                                                     # (a call without events)
    assert set(values) == {0.0, 1.0}, set(values)
    d = np.nonzero(own != deferred)[0]
    assert np.array_equal(own, deferred), f"{d.size} samples differ, frames {d[0] // 2}..{d[-1] // 2}; zero onset own {cb.zero_onset(own)}, deferred {cb.zero_onset(deferred)}"


@pytest.mark.parametrize("sc", [s for s in cb.SCENARIOS + cb.MAIN_CHAIN_SCENARIOS if s.two_parents], ids=lambda s: s.name)
def test_sharded_equals_single(sc):
    """P and Q on different shards of one handle: the single graph ends its chunks where the MERGED cuts of both parents use up the budget, and the
    handle must cut its shards' spans there too — bit for bit (build-twice, as test_sharded_equals_single of tests/test_gpu_granular.py)."""
    from phonic_amd.graph import ShardedGraph

    L = sc.call_frames
    single, sharded = gpu_graph(sc), ShardedGraph([0, 0], cb.SR, 2, sc.max_frames)
    sid, hid = sc.build(single), sc.build(sharded)
    assert sharded.shard_of_mixer(hid["P"]) != sharded.shard_of_mixer(hid["Q"])
    assert sharded.shard_of_mixer(hid["C"]) == sharded.shard_of_mixer(hid["P"])
    a, b = np.zeros((sc.n_calls, 2 * L), np.float32), np.zeros((sc.n_calls, 2 * L), np.float32)
    for k in range(sc.n_calls):
        sc.schedule(single, sid, k * L, (k + 1) * L)
        sc.schedule(sharded, hid, k * L, (k + 1) * L)
        assert single.write(a[k], k * L) == 2 * L and sharded.write(b[k], k * L) == 2 * L
    a, b = a.reshape(-1), b.reshape(-1)
    d = np.nonzero(a != b)[0]
    print(sc.name, "zero onset single", cb.zero_onset(a), "sharded", cb.zero_onset(b), "samples that differ", d.size)
    assert np.abs(a).max() > 1e-2
    assert np.array_equal(a, b), f"{d.size} samples differ, frames {d[0] // 2}..{d[-1] // 2}; zero onset single {cb.zero_onset(a)}, sharded {cb.zero_onset(b)}"
    assert single.device_errors() == 0 and sharded.device_errors() == 0


@pytest.mark.parametrize("interval_frames_", [0, 300], ids=["every_call", "every_300_frames"])
def test_metering_of_the_child_across_70_events(interval_frames_):
    """C metered under P across a write that holds 70 events of P (the budget ends the chunk at the 64th): one record per call of C, cut at P's
    event times, however the host cut the chunk. The model (tests/metering_model.py) is fed C's own output — the same graph without P's voice,
    chain and events, rendered by the device — cut on that grid. Peak exact, RMS within one ulp (tests/test_gpu_metering.py: assert_level)."""
    sc = cb.METER_SCENARIO
    interval = interval_frames_ / cb.SR
    assert interval_frames(interval, cb.SR) == interval_frames_
    n_calls, L = 3, sc.call_frames
    assert len(sc.cuts_in_chunk(1 * L, "P")) == 70 and sc.c_len > n_calls * L       # the write of block 1 holds the 70 events, C plays throughout
    solo = sc.render(gpu_graph(sc), solo="C", n_calls=n_calls)
    assert np.abs(solo).max() > 1e-2
    g = gpu_graph(sc)
    ids = sc.build(g)
    g.set_metering(interval)
    model = AudioLevelState(interval, cb.SR)
    grid = sc.grid("P")
    out = np.zeros(2 * L, np.float32)
    for b in range(n_calls):
        sc.schedule(g, ids, b * L, (b + 1) * L)
        assert g.write(out, b * L) == 2 * L
        calls = [t for t in grid if b * L <= t <= (b + 1) * L]
        assert len(calls) - 1 == (71 if b == 1 else 1)
        for t0, t1 in zip(calls[:-1], calls[1:]):
            model.record(solo[2 * t0: 2 * t1], t0)
        l = g.audio_level(ids["C"])
        (mp, mr), gp, gr = model.level(), l.peak, l.rms
        print("call", b, "publishes", model.publishes, "gpu", gp, gr, "model", mp, mr, "rms ulps", [ulp_distance(gr[c], mr[c]) for c in range(2)])
        assert tuple(gp) == mp, (b, gp, mp)
        for c in range(2):
            assert ulp_distance(gr[c], mr[c]) <= 1, (b, c, gr[c], mr[c])
    assert model.publishes > 3 and max(model.level()[0]) > 0.0
    assert g.device_errors() == 0


def test_main_chain_against_the_oracle():
    """The 64-cut scenario with Gain -> Delay on the main mixer. The reference does not cut the main mixer's chunk at a sub-mixer's events: it takes
    `audible_input` once for the chunk in which its gate on P expires (frames 17408..18431) and runs the chain once over it. The call budget makes
    the device end that chunk at the 64th cut (frame 18304) and begin another: the chain is called twice, its Gain bypasses one reference call
    early, the Delay takes its tail one call early, and the bus is exactly zero from frame 24576 on where the oracle's is from 25600 on — 1024
    frames of a trickle of 8e-19 .. 2.6e-18, far inside the tolerances (measured on an MI355X, before and after this file's host fix). The budget itself moves a decision of the reference, and the host cannot mend
    it without the render kernels (a continuation that is no new chunk for the device would not reset its call count): docs/parity_findings.md,
    finding (20). So this test holds the scenario to the tolerances only; the zero masks are printed, not asserted."""
    sc = cb.BY_NAME["c64_main_chain"]
    g = gpu_graph(sc)
    a, b = sc.render(g), oracle_bus(sc)
    print(sc.name, "zero onset gpu", cb.zero_onset(a), "oracle", cb.zero_onset(b), "mask diff (frames, first, last)", zero_mask_report(a, b))
    assert np.abs(b).max() > 1e-2
    compare(a, b)
    assert g.device_errors() == 0
