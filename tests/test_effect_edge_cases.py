"""CPU proof that the table of tests/effect_edge_cases.py is a sharp one — no device.

  * the restated rules agree with the oracle where the oracle can be asked (the Compressor's look-ahead window, the distance of the Delay's taps
    behind the write head) and with the edge values the rules were measured to have;
  * every case is DETECTABLE: the oracle run of its nearest wrong variant (window or delay off by one frame, LFO depth scaled by 0.99, a cutoff
    short of the clamp, the rate swapped with 48 000) differs from the right run by at least 10 x the tolerance the GPU test grants;
  * the signal does what the case needs: the tracked peak leaves the look-ahead window at least three times, the LFO passes two full cycles, the
    wet path is audible."""
import numpy as np
import pytest

import effect_edge_cases as ec
import oracle
from phonic_amd import _capi

F = np.float32
RMS_TOL, MAX_TOL = 1e-5, 1e-4          # what tests/test_gpu_effect_edges.py grants the device (x scale)
ALL = ec.cases()
_RIGHT = {}


def right(case):
    if case.id not in _RIGHT:
        _RIGHT[case.id] = ec.run_oracle(case, with_log=case.kind in ec.INDEX_WORDS_PER_FRAME)
    r = _RIGHT[case.id]
    return r if isinstance(r, tuple) else (r, [])


def same_f32(a, b):
    """`b` is a decimal quoted to eight digits: the same f32, or its neighbour where the quote fell between two."""
    return abs(int(F(a).view(np.int32)) - int(F(b).view(np.int32))) <= 1


def test_table_has_the_expected_shape():
    by = {g: ec.cases(g) for g in ("comp", "delay", "chorus", "nyquist", "sweep")}
    assert all(by.values())
    assert len(by["sweep"]) == 10 * 2 * len(ec.SWEEP_RATES)
    for c in ALL:
        assert c.path in ("fast", "serial", "unknown") and c.wrong, c.id
        assert max(c.block_sizes()) <= 4096
    # which side of each edge takes which path
    paths = {c.id: c.path for c in ALL}
    for law in ("comp", "lim"):
        for W, p in ((49, "fast"), (64, "serial"), (65, "fast"), (127, "fast"), (128, "serial"), (129, "fast"), (511, "fast"), (512, "serial"), (513, "fast"),
                     (3073, "fast"), (3074, "serial")):
            assert [v for k, v in paths.items() if k.startswith(f"{law}_48000_W{W}_")] == [p], (law, W)
        assert paths[f"{law}_8000_W8_min"] == "serial" and paths[f"{law}_8000_W9_w"] == "fast" and paths[f"{law}_8000_W1600_max"] == "fast"
        assert paths[f"{law}_44100_W1764_default"] == "fast" and paths[f"{law}_96000_W3840_default"] == "serial"
    for sr in ec.LOW_RATES:
        assert paths[f"delay_{sr}_below_edge"] == "serial" and paths[f"delay_{sr}_at_edge"] == "fast" and paths[f"delay_{sr}_floor66_top"] == "fast"
        assert paths[f"chorus_{sr}_below_edge"] == "serial" and paths[f"chorus_{sr}_at_edge"] == "fast"
    assert paths["delay_96000_minimum"] == "fast" and paths["delay_192000_minimum"] == "fast"
    assert paths["chorus_48000_dlay_minimum"] == "serial"
    # dlay 100 ms with dpth 1 stays below mask - 8 at every rate: the ring is sized for exactly that sum and padded to a power of two
    for sr, lfo_range in ((8000, 46), (44100, 256), (192000, 1114)):
        assert int(ec.chorus_lfo_range(sr)) == lfo_range and paths[f"chorus_{sr}_longest_deepest"] == "fast"
    sr_hi = ec.delay_upper_edge_rate()
    assert sr_hi == 32360 and ec.delay_mask(sr_hi) + 1 == 131072
    assert paths[f"delay_{sr_hi}_longest"] == "fast" and paths[f"delay_{sr_hi}_longest_lfdt"] == "serial"
    for c in ec.cases("delay"):
        if c.id.startswith("delay_lfdt_"):
            assert c.path == ("fast" if "accepted" in c.id else "serial"), c.id


def test_every_case_and_variant_is_inside_the_parameter_ranges():
    """pg_effect_create validates the host description without a device call: no case may ask for a value the product refuses (the oracle clamps)."""
    import phonic_amd

    for c in ALL:
        for v in [c] + [ec.apply_variant(c, ch) for _, ch in c.wrong]:
            phonic_amd.Effect(v.kind, v.params, v.seeds).close()
            for ups in v.updates.values():
                for (id4, val, norm) in ups:
                    lo, hi, _ = ec.prange(v.kind, id4)
                    assert (0.0 <= val <= 1.0) if norm else (lo <= F(val) <= hi), (v.id, id4, val)


def test_restated_rules_reproduce_the_measured_edges():
    delay = {8000: (8.2499990, 8.25), 22050: (2.9931967, 2.9931970), 44100: (1.4965984, 1.4965985), 48000: (1.3749998, 1.3749999)}
    chorus = {8000: (7.9999986, 7.9999990), 22050: (2.9024937, 2.9024940), 44100: (1.4512469, 1.4512470), 48000: (1.3333330, 1.3333331)}
    for sr in ec.LOW_RATES:
        for got, want in ((ec.delay_lower_edge(sr), delay[sr]), (ec.chorus_lower_edge(sr), chorus[sr])):
            assert F(np.nextafter(F(got[0]), F(1e9))) == F(got[1]), "the two sides of an edge are one f32 apart"
            assert same_f32(got[0], want[0]) and same_f32(got[1], want[1]), (sr, got, want)
    assert ec.delay_lower_edge(96000) is None and ec.delay_lower_edge(192000) is None
    assert [ec.comp_window(0.001, sr) for sr in (8000, 44100, 48000, 96000)] == [8, 45, 49, 97]
    assert [ec.comp_window(0.2, sr) for sr in (8000, 44100, 48000, 96000)] == [1600, 8820, 9600, 19200]
    assert [ec.comp_window(F(k / 48000), 48000) for k in (63.5, 64.5, 3072.5, 3073.5)] == [64, 65, 3073, 3074]
    assert ec.comp_window(0.04, 192000) == 7680
    lo, _ = ec.delay_lower_edge(48000, {"lfdt": 1.0})
    assert abs(lo - 51.885) < 0.001
    assert ec.delay_chunk({"dlay": ec.delay_lower_edge(48000)[1]}, 48000) == 65
    assert ec.delay_chunk({"dlay": 375.0}, 48000) == 1024 and ec.delay_chunk({"dlay": 375.0, "ldfb": 0.5}, 48000, tmp_floats=512) == 512
    assert ec.delay_chunk({"dlay": ec.delay_lower_edge(48000, {"lfdt": 1.0})[1], "lfdt": 1.0}, 48000) == 64


COMP_WINDOWS = sorted({(c.sr, c.params["look"]) for c in ec.cases("comp")} | {(192000, 0.04), (44100, 0.001), (96000, 0.2)})


@pytest.mark.parametrize("sr,look", COMP_WINDOWS, ids=[f"{sr}_{look:.6g}" for sr, look in COMP_WINDOWS])
def test_comp_window_is_the_look_ahead_the_oracle_applies(sr, look):
    """A limiter that never limits (threshold 0 dB, make-up 0 dB) returns its input delayed by the look-ahead: the impulse comes out W frames late."""
    W = ec.comp_window(look, sr)
    e = oracle.OracleEffect(_capi.FX_COMPRESSOR, {"thrs": 0.0, "rato": 20.0, "knee": 0.0, "gain": 0.0, "look": look})
    e.initialize(sr, 2, 4096)
    n = W + 16
    x = np.zeros(2 * n, np.float32)
    x[0], x[1] = 0.5, -0.25
    for off in range(0, n, 4096):
        e.process(x[2 * off:2 * min(off + 4096, n)])
    assert np.flatnonzero(x).tolist() == [2 * W, 2 * W + 1] and x[2 * W] == F(0.5)


def tap_distances(case, logs):
    """Frames between the write head and the SECOND tap (index1 + 1) of every frame's read, left channel, from the oracle's index log."""
    i1 = np.concatenate(logs).reshape(-1, 2)[:, 0].astype(np.int64)
    mask = ec.delay_mask(case.sr) if case.kind == _capi.FX_DELAY else ec.chorus_mask(case.sr)
    n = np.arange(i1.size, dtype=np.int64)
    return ((n - i1) & mask) - 1


DELAY_FAST = [c for c in ec.cases("delay") if c.path == "fast"]


@pytest.mark.parametrize("case", DELAY_FAST, ids=[c.id for c in DELAY_FAST])
def test_delay_chunk_keeps_every_read_behind_the_chunk(case):
    """Frame k of a chunk may read nothing the chunk writes: its second tap lies at least k + 1 frames behind its own write position, so a chunk of
    T frames needs the taps at least T frames back. At floor(samples) == 66 with no fraction that is met with nothing to spare."""
    _, logs = right(case)
    dist = tap_distances(case, logs)
    T = ec.delay_chunk(case.params, case.sr)
    assert int(dist.min()) >= T, (int(dist.min()), T)
    if case.id.endswith("_at_edge"):
        assert T == 65
        if ec.delay_samples(case.params["dlay"], case.sr) == F(66.0):
            assert int(dist.min()) == T                       # the chunk's last frame reads the last frame written before the chunk
    if case.lfo_cycles:
        assert int(dist.min()) <= T + 30, "the LFO never brings the tap near the chunk"


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_every_case_is_detectable(case):
    good, _ = right(case)
    scale = max(1.0, float(np.abs(good).max()))
    assert np.isfinite(good).all()
    for label, changes in case.wrong:
        bad = ec.run_oracle(ec.apply_variant(case, changes))
        rms, mx = ec.diff_figures(good, bad)
        print(f"{case.id} against {label}: rms {rms:.3e} max {mx:.3e}")
        assert rms >= 10 * RMS_TOL * scale and mx >= 10 * MAX_TOL * scale, (label, rms, mx)


COMP = ec.cases("comp")


@pytest.mark.parametrize("case", COMP, ids=[c.id for c in COMP])
def test_tracked_peak_leaves_the_window(case):
    W = ec.comp_window(case.params["look"], case.sr)
    x = ec.make_signal(case)
    assert ec.peak_expiries(x, W) >= 3
    assert case.total_frames() >= W + 3 * 1024                # the run outlasts the window by three blocks
    good, _ = right(case)
    assert float(np.abs(good[2 * (W + 1024):]).max()) > 1e-2  # (and what comes out behind the window is not silence)
    assert not np.array_equal(good[2 * W:], x[:good.size - 2 * W])   # the gain computer does act on it


LFO = [c for c in ALL if c.lfo_cycles]


@pytest.mark.parametrize("case", LFO, ids=[c.id for c in LFO])
def test_lfo_passes_full_cycles(case):
    _, logs = right(case)
    dist = tap_distances(case, logs).astype(np.float64)
    mid = 0.5 * (dist.max() + dist.min())
    assert dist.max() - dist.min() > 0.9 * 2 * 50.0 * 0.001 * case.sr    # depth +-1: the tap travels +-50 ms
    above = dist > mid
    rising = int(np.count_nonzero(~above[:-1] & above[1:]))
    falling = int(np.count_nonzero(above[:-1] & ~above[1:]))
    assert min(rising, falling) >= case.lfo_cycles, (rising, falling)


WET = [c for c in ALL if c.group in ("delay", "chorus")]


@pytest.mark.parametrize("case", WET, ids=[c.id for c in WET])
def test_wet_path_is_audible(case):
    """Against the same effect with wet_ = 0 the output differs by more than 1e-3: the delay-line reads of the case are compared, not zeros."""
    good, _ = right(case)
    dry = ec.run_oracle(case._replace(params=dict(case.params or {}, **{"wet_": 0.0})))
    assert ec.diff_figures(good, dry)[1] > 1e-3
