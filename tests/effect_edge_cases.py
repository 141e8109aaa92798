"""The effects' time-parallel paths at their eligibility and chunk edges: the rules restated, and the table of cases derived from them.

Each effect's time-parallel path starts with a few lines of f32 arithmetic that decide whether it may run and how long a chunk may be
(phonic_amd/csrc/pg_delay_fast.inl, pg_chorus_fast.inl, pg_comp_fast.inl; the state they look at is built in pg_fxstate.hip). Every one of those
rules is a function of the mixer rate. They are restated here in numpy float32, operation by operation in the device code's order (the library is
built with -ffp-contract=off, so no product is fused into a sum), and the cases are DERIVED from the restated rules — searched for, one f32 apart
where a rule has an edge — not typed in. tests/test_effect_edge_cases.py (CPU) proves the restatement against the oracle and that every case is a
sharp one; tests/test_gpu_effect_edges.py runs the device against the oracle on every case."""
from typing import NamedTuple, Optional

import numpy as np

import workloads
from phonic_amd import _capi

F = np.float32
RAGGED = [256, 1, 0, 3, 1024, 17, 1000, 2, 333, 4096]
LOW_RATES = (8000, 22050, 44100, 48000)


def next_pow2(n):
    n = int(n)
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


_DESC = {}


def prange(kind, id4):
    """(min, max, default) of a parameter, from the library's descriptors (Effect::parameters())."""
    if kind not in _DESC:
        from phonic_amd.graph import effect_parameters

        _DESC[kind] = {p["fourcc"]: p for p in effect_parameters(kind)}
    p = _DESC[kind][_capi.fourcc(id4)]
    return F(p["min"]), F(p["max"]), F(p["default"])


def _p(kind, params, id4):
    return F((params or {}).get(id4, prange(kind, id4)[2]))


# ---- Compressor: pg_fxstate.hip (delay_frames, mask), pg_comp_fast.inl (comp_fast_eligible) ---------------------------------------------------
COMP_FAST_CAP = 4096


def comp_window(look, sr):
    """delay_frames = ceil(f32(look) * f32(sr))."""
    return int(np.ceil(F(look) * F(sr)))


def comp_is_fast(W):
    """delay_frames >= 1 && delay_frames <= mask && delay_frames - 1 + 1024 <= 4096, mask = next_pow2(delay_frames) - 1: a power of two equals
    its own ring size and is above the mask."""
    mask = next_pow2(W) - 1 if W > 0 else 0
    return W >= 1 and W <= mask and W - 1 + 1024 <= COMP_FAST_CAP


def look_for_window(W, sr):
    """A look-ahead time in the middle of the interval that ceil() maps to W frames."""
    look = F((W - 0.5) / sr)
    assert comp_window(look, sr) == W, (W, sr)
    return float(look)


# ---- Delay: pg_fxstate.hip (ring size), pg_delay_fast.inl (delay_fast_eligible, delay_fast) ---------------------------------------------------
def delay_mask(sr):
    n = int(np.ceil((F(4000.0) + F(50.0)) * F(sr) / F(1000.0)))
    return next_pow2(n + 4) - 1


def delay_margin_ms(depth):
    """|depth| * 50 * 1.01 + 0.01 ms: the LFO -> time excursion with the 1 % that covers the parabolic sine's overshoot."""
    return F(abs(F(depth))) * F(50.0) * F(1.01) + F(0.01)


def delay_min_max_samples(params, sr):
    t, d = _p(_capi.FX_DELAY, params, "dlay"), _p(_capi.FX_DELAY, params, "lfdt")
    dev = delay_margin_ms(d) if d != 0 else F(0.0)
    lo = np.maximum(t - dev, F(1.0)) * F(0.001) * F(sr)
    hi = np.maximum(t + dev, F(1.0)) * F(0.001) * F(sr)
    return lo, hi


def delay_is_fast(params, sr):
    """delay_fast_eligible with nothing ramping: LFO shapes 0-4, min_samples >= 66 && max_samples < mask - 8."""
    if int((params or {}).get("lfos", 0)) >= 5:
        return False
    lo, hi = delay_min_max_samples(params, sr)
    return bool(lo >= F(66.0) and hi < F(delay_mask(sr) - 8))


def delay_chunk(params, sr, tmp_floats=None):
    """Frames per chunk of delay_fast: floor(delay_samples) - 1; with LFO -> time floor(min_samples) - 2; with any LFO modulation at most the
    kernel's `tmp_floats`; never more than 1024."""
    t = _p(_capi.FX_DELAY, params, "dlay")
    dt, dfb, dfl = (_p(_capi.FX_DELAY, params, k) for k in ("lfdt", "ldfb", "lfdf"))
    samples = np.maximum(t + F(0.0), F(1.0)) * F(0.001) * F(sr)
    t_max = int(np.floor(samples)) - 1
    if dt != 0:
        t_max = int(np.floor(np.maximum(t - delay_margin_ms(dt), F(1.0)) * F(0.001) * F(sr))) - 2
    if (dt != 0 or dfb != 0 or dfl != 0) and tmp_floats is not None:
        t_max = min(t_max, tmp_floats)
    return min(t_max, 1024)


def delay_samples(dlay, sr):
    return np.maximum(F(dlay), F(1.0)) * F(0.001) * F(sr)


# ---- Chorus: pg_fxstate.hip (lfo_range, ring size), pg_chorus_fast.inl (chorus_fast_eligible) ------------------------------------------------
def chorus_lfo_range(sr):
    return F(256.0) * (F(sr) / F(44100.0))


def chorus_mask(sr):
    max_depth = int(np.ceil(chorus_lfo_range(sr)))
    max_delay = int(np.ceil(F(100.0) * F(sr) / F(1000.0)))
    return next_pow2(2 + max_delay + 2 * max_depth + 1) - 1


def chorus_is_fast(params, sr):
    """floorf(2 + delay_in_samples) >= 66 && 2 + delay_in_samples + 2 * depth_in_samples < mask - 8, nothing ramping."""
    d = _p(_capi.FX_CHORUS, params, "dlay") * F(sr) * F(0.001)
    depth = chorus_lfo_range(sr) * _p(_capi.FX_CHORUS, params, "dpth")
    if not depth >= 0:
        return False
    return bool(np.floor(F(2.0) + d) >= F(66.0) and (F(2.0) + d + F(2.0) * depth) < F(chorus_mask(sr) - 8))


# ---- smoothers: pg_fxstate.hip make_smooth (comp = 44100 / sr) ----------------------------------------------------------------------------------
def linear_ramp_frames(current, target, step, sr):
    """LinearSmoothedValue: round(|target - current| / (step * 44100 / sr)) frames."""
    cs = F(step) * (F(44100.0) / F(sr))
    return int(max(np.round((F(target) - F(current)) / (cs if target >= current else -cs)), 0))


def f32_edge(pred, lo, hi):
    """(largest f32 for which pred is false, smallest for which it is true) between lo (false) and hi (true); pred is monotone there."""
    lo, hi = F(lo), F(hi)
    assert not pred(lo) and pred(hi), (lo, hi)
    a, b = int(lo.view(np.int32)), int(hi.view(np.int32))
    while b - a > 1:
        m = (a + b) // 2
        if pred(np.int32(m).view(np.float32)):
            b = m
        else:
            a = m
    return float(np.int32(a).view(np.float32)), float(np.int32(b).view(np.float32))


def delay_lower_edge(sr, extra=None):
    """The largest ineligible and the smallest eligible `dlay` (ms) at the 66-sample bound; None where it lies below the parameter's minimum."""
    lo, hi, _ = prange(_capi.FX_DELAY, "dlay")
    pred = lambda x: delay_is_fast(dict(extra or {}, dlay=x), sr)
    if pred(lo):
        return None
    return f32_edge(pred, lo, F(200.0))


def chorus_lower_edge(sr):
    lo, _, _ = prange(_capi.FX_CHORUS, "dlay")
    return f32_edge(lambda x: chorus_is_fast({"dlay": x}, sr), lo, F(50.0))


def delay_upper_edge_rate():
    """The first rate (a multiple of 10 Hz from 22 050 Hz up) whose ring — padded to a power of two — is so tightly filled that the longest delay
    with the full LFO -> time margin reaches mask - 8 while the same delay without modulation does not."""
    hi = float(prange(_capi.FX_DELAY, "dlay")[1])
    for sr in range(22050, 192001, 10):
        if delay_is_fast({"dlay": hi}, sr) and not delay_is_fast({"dlay": hi, "lfdt": 1.0}, sr):
            return sr
    raise AssertionError("no rate reaches the Delay's upper bound")


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    id: str
    group: str                   # "comp", "delay", "chorus", "nyquist", "sweep"
    kind: int
    params: Optional[dict]
    sr: int
    blocks: int
    frames: int
    signal: str                  # "noise", or "peaks:<spacing>"
    updates: dict                # {block: [(fourcc, value, normalized)]}
    path: str                    # what the restated rule picks in steady state: "fast", "serial", "unknown" (ramps, no rule restated)
    wrong: tuple = ()            # the nearest wrong variants: ((label, {field: value}), ...) — see test_every_case_is_detectable
    seeds: Optional[tuple] = None
    sizes: Optional[tuple] = None
    edge: bool = True            # an edge case of (a)-(d): also run inside graphs
    lfo_cycles: int = 0          # > 0: the oracle's index log must show that many full LFO cycles
    note: str = ""

    def block_sizes(self):
        return list(self.sizes) if self.sizes else [self.frames] * self.blocks

    def total_frames(self):
        return sum(self.block_sizes())

    def variant(self, changes):
        return self._replace(**changes)


def make_signal(case):
    """Interleaved stereo input of a case. "peaks:<spacing>": quiet noise with isolated loud single-frame peaks `spacing` frames apart (further apart
    than the look-ahead window: the tracked peak leaves the window and the window is rescanned, once per peak) of changing height and channel."""
    n = case.total_frames()
    if case.signal == "noise":
        return workloads.test_signal(n, seed=case.kind + 11, kind="noise")
    name, spacing = case.signal.split(":")
    assert name == "peaks"
    spacing = int(spacing)
    rng = np.random.default_rng(1000 + spacing)
    x = (rng.standard_normal(n * 2) * 0.02).astype(np.float32).reshape(n, 2)
    heights = (0.9, 0.55, 0.8, 0.35, 0.7)
    for k, pos in enumerate(range(37, n, spacing)):
        x[pos, k & 1] = F(heights[k % len(heights)] * (-1.0 if k % 3 == 0 else 1.0))
        x[pos, 1 - (k & 1)] = F(0.1)
    return x.reshape(-1)


def peak_expiries(x, W):
    """How often LookupDelayLine (dsp/delay.rs:206-265) finds its tracked peak leaving the window of W frames and rescans, over the interleaved
    stereo signal x — the reference's bookkeeping, frame by frame."""
    peaks = np.abs(x.astype(np.float64).reshape(-1, 2)).max(axis=1)
    n_buf = next_pow2(W)
    mask = n_buf - 1
    buf = np.zeros(n_buf)
    write_pos = peak_pos = 0
    peak_value = 0.0
    expiries = 0
    for p in peaks:
        read_idx = (write_pos + n_buf - W) & mask
        buf[write_pos & mask] = p
        expired = peak_pos == read_idx
        if p >= peak_value:
            peak_value, peak_pos = p, write_pos
        elif expired:
            if peak_value > 0.1:
                expiries += 1
            peak_value = 0.0
            for i in range(W):
                fi = (write_pos + n_buf - i) & mask
                if buf[fi] >= peak_value:
                    peak_value, peak_pos = buf[fi], fi
        write_pos = (write_pos + 1) & mask
    return expiries


def _comp_cases():
    K = _capi.FX_COMPRESSOR
    out = []
    look_lo, look_hi, look_def = prange(K, "look")
    laws = (("comp", {"rato": 4.0, "knee": 6.0}), ("lim", {"rato": 20.0, "knee": 0.0}))

    def add(tag, sr, look, note=""):
        W = comp_window(look, sr)
        spacing = W + max(24, W // 8)
        blocks = max(8, -(-(37 + 3 * spacing + W) // 1024) + 1, -(-W // 1024) + 3)
        wrong = []
        for dw in (-1, 1):
            other = F((W + dw - 0.5) / sr)
            if look_lo <= other <= look_hi and comp_window(other, sr) == W + dw:
                wrong.append((f"W{dw:+d}", {"params_update": {"look": float(other)}}))
        assert wrong, (tag, sr, W)
        for law, lp in laws:
            params = dict({"thrs": -18.0, "attk": 0.005, "rels": 0.1, "gain": 3.0, "look": float(look)}, **lp)
            out.append(Case(f"{law}_{sr}_W{W}_{tag}", "comp", K, params, sr, blocks, 1024, f"peaks:{spacing}", {}, "fast" if comp_is_fast(W) else "serial",
                            tuple(wrong), note=note))

    w_min = comp_window(look_lo, 48000)
    add("smallest", 48000, look_lo)
    for W in (64, 65, 127, 128, 129, 511, 512, 513, 3073, 3074):
        assert W > w_min
        add("pow2" if W & (W - 1) == 0 else "w", 48000, look_for_window(W, 48000))
    add("min", 8000, look_lo)
    add("w", 8000, look_for_window(comp_window(look_lo, 8000) + 1, 8000))
    add("max", 8000, look_hi)
    add("default", 44100, look_def)
    add("default", 96000, look_def)
    # one path hands over to the other with a live peak: 3073 (time-parallel) -> 3074 (serial) -> 3073, set while a loud peak is inside the window
    a, b = look_for_window(3073, 48000), look_for_window(3074, 48000)
    spacing = 3074 + 384
    for law, lp in laws:
        params = dict({"thrs": -18.0, "attk": 0.005, "rels": 0.1, "gain": 3.0, "look": a}, **lp)
        up = {5: [("look", b, False)], 12: [("look", a, False)]}
        wrong = (("W+1", {"updates": {5: [("look", look_for_window(3075, 48000), False)], 12: [("look", a, False)]}}),
                 ("W-1", {"updates": {5: [("look", b, False)], 12: [("look", look_for_window(3072, 48000), False)]}}))
        out.append(Case(f"{law}_48000_handover_3073_3074", "comp", K, params, 48000, 20, 1024, f"peaks:{spacing}", up, "unknown", wrong))
    return out


def _delay_sample_variants(dlay, sr):
    lo, hi, _ = prange(_capi.FX_DELAY, "dlay")
    out = []
    for sign in (-1, 1):
        other = F(dlay) + F(sign * 1000.0 / sr)
        if lo <= other <= hi:
            out.append((f"delay{sign:+d}", {"params_update": {"dlay": float(other)}}))
    return tuple(out)


def _delay_cases():
    K = _capi.FX_DELAY
    out = []
    base = {"fdbk": 0.6, "driv": 0.3, "cuto": 2500.0}   # (the default cutoff is clamped at 8 kHz: group "nyquist" has that)

    def steady(cid, sr, params, blocks=6, frames=1000, lfo_cycles=0, wrong=None, note=""):
        params = dict(base, **params)
        out.append(Case(cid, "delay", K, params, sr, blocks, frames, "noise", {}, "fast" if delay_is_fast(params, sr) else "serial",
                        wrong if wrong is not None else _delay_sample_variants(params["dlay"], sr), lfo_cycles=lfo_cycles, note=note))

    for i, sr in enumerate(LOW_RATES):
        below, above = delay_lower_edge(sr)
        # the largest dlay whose floor(samples) is still 66: the same 65-frame chunk with the fraction at its other end
        _, past = f32_edge(lambda x: np.floor(delay_samples(x, sr)) >= 67, above, above + 2000.0 / sr)
        top = float(np.nextafter(F(past), F(0.0)))
        steady(f"delay_{sr}_below_edge", sr, {"dlay": below, "mode": i & 1, "ftyp": i % 3})
        steady(f"delay_{sr}_at_edge", sr, {"dlay": above, "mode": i & 1, "ftyp": i % 3}, note="floor(samples) == 66: chunks of 65 frames")
        steady(f"delay_{sr}_floor66_top", sr, {"dlay": top, "mode": 1 - (i & 1), "ftyp": (i + 1) % 3})
    for sr in (96000, 192000):
        assert delay_lower_edge(sr) is None
        steady(f"delay_{sr}_minimum", sr, {"dlay": float(prange(K, "dlay")[0])})
    # upper edge: max_samples < mask - 8
    sr_hi = delay_upper_edge_rate()
    longest = float(prange(K, "dlay")[1])
    n_hi = -(-(int(delay_samples(longest, sr_hi)) + 3 * 1024) // 1024)   # the echo of the first blocks passes inside the run
    steady(f"delay_{sr_hi}_longest", sr_hi, {"dlay": longest}, blocks=n_hi, frames=1024)
    steady(f"delay_{sr_hi}_longest_lfdt", sr_hi, {"dlay": longest, "lfdt": 1.0, "lfor": 5.0}, blocks=n_hi, frames=1024,
           wrong=(("delay-1", {"params_update": {"dlay": float(F(longest) - F(1000.0 / sr_hi))}}),))
    # LFO -> time at the margin: depth +-1, the delay one f32 either side of what the margin admits; shapes 0-4, both routing modes
    sr = 48000
    lfor_hi = float(prange(K, "lfor")[1])
    for mode in (0, 1):
        depth = 1.0 if mode == 0 else -1.0
        below, above = delay_lower_edge(sr, {"lfdt": depth})
        frames = 1000
        blocks = -(-int(2.5 * sr / lfor_hi) // frames)
        for shape in range(5):
            for tag, dlay in (("rejected", below), ("accepted", above)):
                p = {"dlay": dlay, "lfdt": depth, "lfor": lfor_hi, "lfos": shape, "mode": mode}
                steady(f"delay_lfdt_{tag}_shape{shape}_mode{mode}", sr, p, blocks=blocks, frames=frames, lfo_cycles=2,
                       wrong=(("depth*0.99", {"params_update": {"lfdt": depth * 0.99}}),))
    below, above = delay_lower_edge(sr)
    steady("delay_48000_at_edge_ldfb_only", sr, {"dlay": above, "ldfb": 0.8, "lfor": lfor_hi, "lfos": 1})
    steady("delay_48000_at_edge_lfdf_only", sr, {"dlay": above, "lfdf": 0.7, "lfor": lfor_hi, "lfos": 2, "ftyp": 1})
    # ramps across the edge: over inside one piece at 8 kHz, spanning several blocks at 192 kHz
    for sr in (8000, 192000):
        e = delay_lower_edge(sr)
        low = e[0] if e else float(prange(K, "dlay")[0])
        blocks, frames, back = (9, 1000, 5) if sr == 8000 else (16, 1024, 10)   # (60 ms are 11 520 frames at 192 kHz: the echo must pass)
        up = {2: [("dlay", low, False)], back: [("dlay", 40.0, False)]}
        wrong = tuple((lab, {"updates": {2: [("dlay", ch["params_update"]["dlay"], False)], back: up[back]}}) for lab, ch in _delay_sample_variants(low, sr))
        out.append(Case(f"delay_{sr}_ramp_dlay_across_edge", "delay", K, dict(base, dlay=40.0), sr, blocks, frames, "noise", up, "unknown", wrong))
        up = {3: [("lfdt", 1.0, False)]}
        out.append(Case(f"delay_{sr}_ramp_lfdt_on", "delay", K, dict(base, dlay=60.0, lfor=lfor_hi, lfos=1), sr, blocks, frames, "noise", up, "unknown",
                        (("depth*0.99", {"updates": {3: [("lfdt", 0.99, False)]}}),)))
    return out


def _chorus_cases():
    K = _capi.FX_CHORUS
    out = []
    base = {"rate": 3.0, "dpth": 0.5, "fdbk": 0.6}

    def sample_variants(dlay, sr):
        lo, hi, _ = prange(K, "dlay")
        return tuple((f"delay{s:+d}", {"params_update": {"dlay": float(F(dlay) + F(s * 1000.0 / sr))}}) for s in (-1, 1) if lo <= F(dlay) + F(s * 1000.0 / sr) <= hi)

    def steady(cid, sr, params, blocks=6, frames=1000):
        params = dict(base, **params)
        out.append(Case(cid, "chorus", K, params, sr, blocks, frames, "noise", {}, "fast" if chorus_is_fast(params, sr) else "serial",
                        sample_variants(params["dlay"], sr)))

    for sr in LOW_RATES:
        below, above = chorus_lower_edge(sr)
        steady(f"chorus_{sr}_below_edge", sr, {"dlay": below})
        steady(f"chorus_{sr}_at_edge", sr, {"dlay": above})
    steady("chorus_48000_dlay_minimum", 48000, {"dlay": float(prange(K, "dlay")[0])})
    for sr in (8000, 44100, 192000):
        n = -(-(int(0.1 * sr) + 2 * int(chorus_lfo_range(sr)) + 3000) // 1000)   # the longest lag passes inside the run
        steady(f"chorus_{sr}_longest_deepest", sr, {"dlay": float(prange(K, "dlay")[1]), "dpth": float(prange(K, "dpth")[1])}, blocks=n)
    below, above = chorus_lower_edge(48000)
    for tag, start, end in (("down", 12.0, below), ("up", below, 12.0)):
        up = {2: [("dlay", end, False)]}
        wrong = (("delay+1", {"updates": {2: [("dlay", float(F(end) + F(1000.0 / 48000)), False)]}}),)
        out.append(Case(f"chorus_48000_ramp_dlay_{tag}_across_edge", "chorus", K, dict(base, dlay=start), 48000, 9, 1000, "noise", up, "unknown", wrong))
    # a rate / phase ramp that ends inside a piece of at most 16 frames: at 8 kHz the linear smoothers step 5.5 times as far per frame
    sr = 8000
    for pid, start, target, step in (("rate", 1.0, 1.5, 0.005), ("phas", 1.0, 1.1, 0.001)):
        n = linear_ramp_frames(start, target, step, sr)
        assert 8 < n < 23, n
        sizes = (512, 300, 7, 16, 1024, 333, 1000)   # the update sits in front of the 7-frame block: the ramp ends inside the 16-frame one
        up = {2: [(pid, target, False)]}
        out.append(Case(f"chorus_8000_{pid}_ramp_ends_in_short_piece", "chorus", K, dict(base, dlay=12.0, **{pid: start}), sr, len(sizes), 0, "noise", up,
                        "unknown", (("rate48000", {"sr": 48000}),), sizes=sizes, note=f"{pid} ramps for {n} frames"))
    return out


def _nyquist_cases():
    out = []
    KF = _capi.FX_FILTER
    cut_hi = float(prange(KF, "cuto")[1])
    # born by default: coefficients for 44 100 Hz, then initialize() clamps the cutoff to the mixer rate's Nyquist
    for sr in (8000, 22050, 32000, 44100):
        # (below 44 100 Hz the clamp moves the cutoff: another rate shows it. At 44 100 Hz the cutoff stays where new() put it, on Nyquist, which
        # is NOT what with_parameters makes of the descriptor's default)
        wrong = [("rate48000", {"sr": 48000})] if sr < 44100 else [("with_parameters_default_cutoff", {"params": {"cuto": float(prange(KF, "cuto")[2])}})]
        out.append(Case(f"filter_born_default_{sr}", "nyquist", KF, None, sr, 6, 700, "noise", {}, "unknown", tuple(wrong)))
        for ftype in range(4):
            up = {2: [("cuto", 1.0, True)]}
            clamp = min(cut_hi, sr / 2.0)
            wrong = (("cutoff_0.9_of_clamp", {"updates": {2: [("cuto", 0.9 * clamp, False)]}}), ("rate48000", {"sr": 48000}))
            out.append(Case(f"filter_type{ftype}_{sr}_cutoff_to_maximum", "nyquist", KF, {"type": ftype, "cuto": 1000.0, "fltq": 0.707}, sr, 6, 700, "noise",
                            up, "unknown", wrong))
    sr = 22050
    out.append(Case("eq5_22050_frq5_maximum", "nyquist", _capi.FX_EQ5, {"gan5": 9.0, "frq5": float(prange(_capi.FX_EQ5, "frq5")[1])}, sr, 6, 700, "noise", {},
                    "unknown", (("rate48000", {"sr": 48000}), ("cutoff_0.9_of_clamp", {"params_update": {"frq5": 0.9 * sr / 2.0}}))))
    pd = {"dlay": 10.0, "fdbk": 0.7, "cuto": float(prange(_capi.FX_DELAY, "cuto")[1])}
    out.append(Case("delay_22050_cutoff_maximum", "nyquist", _capi.FX_DELAY, pd, sr, 6, 700, "noise", {}, "fast" if delay_is_fast(pd, sr) else "serial", (("rate48000", {"sr": 48000}), ("cutoff_0.9_of_clamp", {"params_update": {"cuto": 0.9 * sr / 2.0}}))))
    pc = {"fltf": float(prange(_capi.FX_CHORUS, "fltf")[1]), "fltq": 0.5, "wet_": 1.0}
    out.append(Case("chorus_22050_prefilter_maximum", "nyquist", _capi.FX_CHORUS, pc, sr, 6, 700, "noise", {}, "fast" if chorus_is_fast(pc, sr) else "serial", (("rate48000", {"sr": 48000}), ("cutoff_0.9_of_clamp", {"params_update": {"fltf": 0.9 * sr / 2.0}}))))
    up = {1: [("cuto", 1.0, True)], 4: [("cuto", 3000.0, False)]}
    out.append(Case("filter_22050_cutoff_ramp_across_clamp", "nyquist", KF, {"type": 0, "cuto": 5000.0, "fltq": 1.0}, sr, 6, 700, "noise", up, "unknown",
                    (("rate48000", {"sr": 48000}), ("cutoff_0.9_of_clamp", {"updates": {1: [("cuto", 0.9 * sr / 2.0, False)], 4: up[4]}}))))
    return out


SWEEP_RATES = (8000, 22050, 44100, 96000, 192000)
SWEEP = [   # (name, kind, with_parameters set, reverb seed, the ramp that starts mid-run)
    ("gain", _capi.FX_GAIN, {"gain": 0.5, "dcfm": 2}, None, ("gain", 0.9, True)),
    ("pan", _capi.FX_PANNING, {"pan ": -0.3, "wdth": 1.5, "invr": 1}, None, ("pan ", 0.8, False)),
    ("filter", _capi.FX_FILTER, {"type": 3, "cuto": 500.0, "fltq": 2.0}, None, ("cuto", 800.0, False)),
    ("eq5", _capi.FX_EQ5, {"gan1": 6.0, "gan2": -3.0, "gan3": 4.0, "gan4": -6.0, "gan5": 2.0, "bw_2": 1.5}, None, ("gan2", 9.0, False)),
    ("delay", _capi.FX_DELAY, {"mode": 1, "dlay": 20.0, "fdbk": 0.7, "driv": 0.5, "ftyp": 2, "wdth": 1.0}, None, ("wet_", 0.8, False)),
    ("reverb", _capi.FX_REVERB, {"room": 1.0, "wet ": 0.5}, 5, ("wet ", 0.8, False)),
    ("chorus", _capi.FX_CHORUS, {"rate": 3.0, "dpth": 0.8, "fdbk": -0.6, "dlay": 5.0, "fltt": 1, "fltf": 300.0, "fltq": 0.4}, None, ("dpth", 0.3, False)),
    ("comp", _capi.FX_COMPRESSOR, {"thrs": -30.0, "rato": 20.0, "knee": 0.0, "attk": 0.02, "rels": 0.1, "gain": 0.0, "look": 0.02}, None, ("gain", -6.0, False)),
    ("gate", _capi.FX_GATE, {"thrs": -20.0, "attk": 0.002, "hold": 0.01, "rels": 0.05, "rnge": -40.0}, None, ("thrs", -10.0, False)),
    ("dist", _capi.FX_DISTORTION, {"type": 4, "driv": 4.0}, None, ("driv", 3.0, False)),
]


def _sweep_cases():
    out = []
    for sr in SWEEP_RATES:
        for name, kind, params, seed, ramp in SWEEP:
            for tag, p in (("default", None), ("params", params)):
                seeds = workloads.reverb_seeds(seed + (0 if p else 1)) if seed is not None else None
                out.append(Case(f"{name}_{tag}_{sr}", "sweep", kind, p, sr, len(RAGGED), 0, "noise", {5: [ramp]}, "unknown", (("rate48000", {"sr": 48000}),),
                                seeds=seeds, sizes=tuple(RAGGED), edge=False))
    return out


_CASES = None


def cases(group=None):
    global _CASES
    if _CASES is None:
        _CASES = _comp_cases() + _delay_cases() + _chorus_cases() + _nyquist_cases() + _sweep_cases()
        ids = [c.id for c in _CASES]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return [c for c in _CASES if group is None or c.group == group]


def apply_variant(case, changes):
    """A case with one of its wrong variants applied: "params_update" merges into the parameters, any other key replaces the field."""
    changes = dict(changes)
    upd = changes.pop("params_update", None)
    if upd is not None:
        changes["params"] = dict(case.params or {}, **upd)
    return case._replace(**changes)


# ---- running a case ------------------------------------------------------------------------------------------------------------------------------
INDEX_WORDS_PER_FRAME = {_capi.FX_DELAY: 2, _capi.FX_CHORUS: 2, _capi.FX_REVERB: 16}


def run_effect(effect, case, x=None, log_begin=None, log_end=None):
    """The case through one standalone effect handle (the product's or the oracle's: same calls). log_begin(words) / log_end(words) -> int32 array
    bracket every non-empty process call when given; returns (output, [index log per block])."""
    effect.initialize(case.sr, 2, 4096)
    y = (make_signal(case) if x is None else x).copy()
    per_frame = INDEX_WORDS_PER_FRAME.get(case.kind, 0)
    logs, off = [], 0
    for blk, n in enumerate(case.block_sizes()):
        for (id4, val, norm) in case.updates.get(blk, []):
            effect.set_parameter(id4, val, norm)
        logging = log_begin is not None and per_frame and n > 0
        if logging:
            log_begin(n * per_frame)
        effect.process(y[off * 2:(off + n) * 2])
        if logging:
            logs.append(log_end(n * per_frame))
        off += n
    return y, logs


def run_oracle(case, with_log=False):
    import ctypes as C

    import oracle

    e = oracle.OracleEffect(case.kind, case.params, case.seeds)
    if not with_log:
        return run_effect(e, case)[0]
    lib = oracle.lib()

    def end(words):
        buf = np.zeros(words, np.int32)
        n = lib.po_index_log_end(buf.ctypes.data_as(C.POINTER(C.c_int32)), words)
        assert n == words, (n, words)
        return buf
    return run_effect(e, case, log_begin=lambda words: lib.po_index_log_begin(), log_end=end)


def build_graph(g, case, placement, x=None):
    """The case's effect inside a graph, fed by one looping voice that plays the case's own signal at the mixer rate (no resampling):
    "sub": alone on a sub-mixer; "sub_reverb": on a sub-mixer in front of a Reverb; "main": on the main mixer's bus. Returns the effect's id."""
    x = make_signal(case) if x is None else x
    m = 0 if placement == "main" else g.add_mixer()
    fx = g.add_effect(m, case.kind, params=case.params, reverb_seeds=case.seeds)
    if placement == "sub_reverb":
        g.add_effect(m, _capi.FX_REVERB, params={"room": 0.4, "wet ": 0.4}, reverb_seeds=workloads.reverb_seeds(61))
    g.add_voice(m, x, 2, case.sr, volume=1.0, panning=0.0, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    return fx


def render_graph(g, case, fx, blocks_per_write=1):
    """The case's blocks, `blocks_per_write` of them per write call; the case's updates are scheduled at the first frame of the block they name."""
    sizes = case.block_sizes()
    out = np.zeros(sum(sizes) * 2, np.float32)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    for blk in range(0, len(sizes), blocks_per_write):
        end = min(blk + blocks_per_write, len(sizes))
        for b in range(blk, end):
            for (id4, val, norm) in case.updates.get(b, []):
                g.schedule_param(fx, id4, val, int(starts[b]), norm)
        if starts[end] > starts[blk]:
            w = g.write(out[starts[blk] * 2:starts[end] * 2], int(starts[blk]))
            assert w in (0, (starts[end] - starts[blk]) * 2), w
    return out


def diff_figures(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0, float(np.abs(d).max()) if d.size else 0.0
