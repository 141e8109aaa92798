"""CPU pre-check of tests/call_budget_scenarios.py: every scenario, rendered by the oracle alone, reaches what tests/test_gpu_call_budget.py
needs it to reach — the counted cuts in the targeted chunk, the gate's expiry in the intended call, a trickle below 1e-3 behind it, and exact
zeros from a frame on that the restated decisions (`gate_expiry`, `chain_onset`) predict and that moves when the decision moves by one call."""
import numpy as np
import pytest

import call_budget_scenarios as cb
import oracle
from phonic_amd import _capi

_TAILS = {}


def tails(delay_params):
    """Effect::process_tail of the chain Gain -> Delay at 8 kHz, from the oracle's effects."""
    key = tuple(sorted(delay_params.items()))
    if key not in _TAILS:
        out = []
        for kind, p in ((_capi.FX_GAIN, cb.GAIN), (_capi.FX_DELAY, delay_params)):
            e = oracle.OracleEffect(kind, p)
            e.initialize(cb.SR, 2, 1024)
            out.append(e.process_tail())
            assert out[-1] is not None
        _TAILS[key] = out
    return _TAILS[key]


def oracle_render(sc, **kw):
    return sc.render(oracle.OracleGraph(cb.SR, 2, sc.max_frames), **kw)


def parent_onset(sc, par, s, shift=0):
    grid = sc.grid(par)
    k = cb.gate_expiry(grid, s)
    return (grid[k], grid[k + 1]), cb.chain_onset(grid, k + shift, tails(cb.P_DELAY))


@pytest.mark.parametrize("sc", cb.SCENARIOS, ids=lambda s: s.name)
def test_scenario_reaches_its_call(sc):
    # the cuts: n distinct times in the targeted chunk (duplicates counted once, both parents' merged), more events than cuts
    assert len(sc.cuts_in_chunk(sc.t0)) == sc.n_cuts
    n_events = sum(1 for t, *_ in sc.events if sc.t0 < t < sc.t0 + sc.call_frames)
    assert n_events > sc.n_cuts
    kinds = set(k for _, _, k, _ in sc.events)
    assert kinds == {"gain", "volume", "panning"}
    call, onset = parent_onset(sc, "P", sc.s_p)
    assert call == sc.expiry_call, (call, sc.expiry_call)
    assert call[0] == sc.t0 + sc.offsets[sc.place - 1]                 # the call that begins at cut `place - 1`
    onsets = [onset]
    if sc.two_parents:
        qcall, qonset = parent_onset(sc, "Q", sc.s_q)
        assert sc.t0 <= qcall[0] < sc.t0 + sc.call_frames
        onsets.append(qonset)
    # a decision one call early or late moves the onset
    for par, s, on in zip("PQ", (sc.s_p, sc.s_q), onsets):
        assert parent_onset(sc, par, s, -1)[1] < on < parent_onset(sc, par, s, +1)[1]

    bus = oracle_render(sc)
    got = cb.zero_onset(bus)
    print(sc.name, "expiry call", call, "onsets", onsets, "oracle", got)
    assert got == max(onsets)
    assert got < sc.total - sc.call_frames                             # exact zeros for at least one whole call
    # C's own output (P without voice and chain) is exactly zero from its voice's last frame on, and audible in the call in front of S
    solo = oracle_render(sc, solo="C", n_calls=-(-(sc.s_p + 64) // sc.call_frames))
    assert cb.zero_onset(solo) <= sc.s_p and np.abs(solo[2 * (sc.s_p - 64): 2 * sc.s_p]).max() >= 0.002
    # the trickle: behind P's voice and C's silence the bus is non-zero and below 1e-3 up to the onset
    tr = np.abs(bus.reshape(-1, 2)[max(sc.p_len, sc.c_len) + 2048: got])
    assert tr.shape[0] > 1024 and tr.max() < 1e-3 and tr.any(axis=1).all()
    assert tr[-64:].min() > 1e-30                                       # (normal f32 numbers: nothing here hangs on how denormals are treated)


@pytest.mark.parametrize("sc", cb.MAIN_CHAIN_SCENARIOS, ids=lambda s: s.name)
def test_main_chain_scenario_reaches_the_capped_chunk(sc):
    """With a chain on the main mixer: the main mixer's gate on P (one count per chunk of the main mixer) expires in the targeted chunk, the one
    the call budget cuts on the device, and the main bus trickles until the chain has run down."""
    assert len(sc.cuts_in_chunk(sc.t0)) == sc.n_cuts
    L = sc.call_frames
    p_bus = oracle_render(sc, main_chain=False).reshape(-1, L * 2)
    quiet = np.abs(p_bus).max(axis=1) < 1e-3
    first = int(np.nonzero(~quiet)[0][-1]) + 1                          # the first chunk from which P stays below the threshold
    grid = list(range(0, sc.total + 1, L))
    k = cb.gate_expiry(grid, first * L)
    assert k == sc.target, (first, k)
    onset = cb.chain_onset(grid, k, tails(sc.main_delay))
    bus = oracle_render(sc)
    got = cb.zero_onset(bus)
    print(sc.name, "first quiet chunk", first, "expiry chunk", k, "onset", onset, "oracle", got)
    assert got == onset and got <= sc.total - L
    assert cb.chain_onset(grid, k - 1, tails(sc.main_delay)) < onset < cb.chain_onset(grid, k + 1, tails(sc.main_delay))
    tr = np.abs(bus.reshape(-1, 2)[(k + 1) * L: got])
    assert tr.max() < 1e-3 and tr.any(axis=1).all() and tr[-64:].min() > 1e-30
