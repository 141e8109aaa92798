"""Parity of the GPU mixer graph (`MixedSource::write` semantics through pg_graph_*) against the CPU oracle:
resampler schedule, looping, start/stop times with fade-out, volume/panning events, sub-mixers with effect chains,
bus effects, sample-accurate parameter events, and the benchmark workloads at reduced voice counts."""
import numpy as np
import pytest

import oracle
import workloads
from phonic_amd import _capi

pytestmark = pytest.mark.gpu
SR = 48000


def graphs(max_frames=4096):
    from phonic_amd.graph import Graph

    return Graph(SR, 2, max_frames, 0), oracle.OracleGraph(SR, 2, max_frames)


def compare(a, b, rms_tol=1e-5, max_tol=1e-4):
    assert np.isfinite(a).all()
    d = a.astype(np.float64) - b.astype(np.float64)
    rms = float(np.sqrt(np.mean(d * d)))
    assert rms <= rms_tol, f"rms {rms}"
    assert float(np.abs(d).max()) <= max_tol, f"max {np.abs(d).max()}"
    return rms


def both(build, n_blocks, block, actions=None, max_frames=4096):
    """Build the same graph twice, render fixed blocks (the WavOutput pull loop); `actions` = {block: fn(graph)}."""
    gg, gc = graphs(max_frames)
    outs = []
    for g in (gg, gc):
        ids = build(g)
        out = np.zeros((n_blocks, block * 2), np.float32)
        pos = 0
        for blk in range(n_blocks):
            if actions and blk in actions:
                actions[blk](g, ids, pos)
            w = g.write(out[blk], pos)
            assert w in (0, block * 2)
            pos += block
        outs.append(out.reshape(-1))
    return outs


def test_resampled_sources_bit_exact_schedule():
    """Main-mixer sources only (no effects): 44.1k->48k cubic, gain+pan, sum. The f32 sub_pos schedule and the Hermite
    taps are exact, so every voice must match the oracle bit for bit; the sum over voices is within f32 reassociation."""
    def build(g):
        return [g.add_voice(0, workloads.tone_buffer(i, 44100, 0.05), 2, 44100, volume=0.5, panning=workloads.voice_pan(i), has_repeat=1,
                            repeat=_capi.PG_REPEAT_FOREVER) for i in range(1)]
    a, b = both(build, 6, 1024)
    assert np.array_equal(a, b)  # single voice: bit exact, across several loop wraps (0.05 s buffer)

    def build8(g):
        return [g.add_voice(0, workloads.tone_buffer(i, 44100, 0.05 + 0.01 * i), 2, 44100, volume=0.3, panning=workloads.voice_pan(i),
                            has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER) for i in range(8)]
    a, b = both(build8, 4, 1024)
    compare(a, b, 1e-7, 1e-6)


def test_mono_source_speed_and_one_shot():
    """Mono file (ChannelMappedSource), speed 1.5 (ratio > 1 branch), plays once and ends (transient source removal):
    after the end the mixer is empty and write() returns 0 without touching the buffer."""
    def build(g):
        return [g.add_voice(0, workloads.tone_buffer(3, 44100, 0.03, channels=1), 1, 44100, speed=1.5, volume=0.8, panning=-0.4)]
    gg, gc = graphs()
    res = []
    for g in (gg, gc):
        build(g)
        outs, rets = [], []
        pos = 0
        for blk in range(4):
            o = np.full(512 * 2, 7.0, np.float32)
            rets.append(g.write(o, pos))
            outs.append(o)
            pos += 512
        res.append((np.concatenate(outs), rets))
    assert res[0][1] == res[1][1]
    assert res[0][1][-1] == 0 and np.all(res[0][0][-1024:] == 7.0)
    assert np.array_equal(res[0][0], res[1][0])


def test_equal_rate_bypass_and_loop_range():
    def build(g):
        return [g.add_voice(0, workloads.tone_buffer(5, 48000, 0.02), 2, 48000, has_repeat=1, repeat=3, has_loop_range=1, loop_start=100,
                            loop_end=700, volume=1.0)]
    a, b = both(build, 5, 1000)
    assert np.array_equal(a, b)


def test_start_stop_fade_and_events():
    """Delayed start inside a block, stop with the default 50 ms fade-out, volume and panning events mid-block."""
    def build(g):
        v0 = g.add_voice(0, workloads.tone_buffer(1, 44100, 0.5), 2, 44100, start_time=300, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        v1 = g.add_voice(0, workloads.tone_buffer(2, 48000, 0.5), 2, 48000, start_time=0, fade_in_seconds=0.01, has_repeat=1,
                         repeat=_capi.PG_REPEAT_FOREVER)
        return [v0, v1]

    def act1(g, ids, pos):
        g.set_voice_volume(ids[0], 0.3, pos + 100)
        g.set_voice_panning(ids[1], 0.7, pos + 517)
        g.stop_voice(ids[1], pos + 800)

    a, b = both(build, 8, 1024, actions={1: act1})
    compare(a, b, 1e-6, 1e-5)  # fader inertia goes through expf (device libm vs glibc): not bit exact
    assert np.abs(a[-2048:]).max() > 0  # voice 0 still plays


def test_submixer_chain_and_bus_effects():
    """Sub-mixers with per-voice chains + sources on the main mixer + bus chain; parameter events at sample times inside
    blocks for a sub-mixer effect (device-side split) and a bus effect (host-side split)."""
    def build(g):
        ids = {}
        for i in range(3):
            m = g.add_mixer()
            ids[f"f{i}"] = g.add_effect(m, _capi.FX_FILTER, params={"type": 0, "cuto": 1500.0 + 500 * i, "fltq": 0.9})
            ids[f"c{i}"] = g.add_effect(m, _capi.FX_CHORUS)
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.3), 2, 44100, volume=0.4, panning=workloads.voice_pan(i), has_repeat=1,
                        repeat=_capi.PG_REPEAT_FOREVER)
            g.add_voice(m, workloads.tone_buffer(i + 20, 48000, 0.2, channels=1), 1, 48000, volume=0.2, start_time=700 * i, has_repeat=1,
                        repeat=_capi.PG_REPEAT_FOREVER)
        g.add_voice(0, workloads.tone_buffer(9, 48000, 0.25), 2, 48000, volume=0.3, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        ids["eq"] = g.add_effect(0, _capi.FX_EQ5, params={"gan1": 4.0, "gan4": -5.0})
        ids["lim"] = g.add_effect(0, _capi.FX_COMPRESSOR, params={"thrs": -20.0, "rato": 20.0, "knee": 0.0, "gain": 0.0, "look": 0.02})
        return ids

    def act(g, ids, pos):
        g.schedule_param(ids["f1"], "cuto", 400.0, pos + 333)
        g.schedule_param(ids["c2"], "dpth", 0.9, pos + 50)
        g.schedule_param(ids["eq"], "gan2", 8.0, pos + 601)
        g.schedule_reset(ids["c0"], pos + 900)

    a, b = both(build, 6, 1024, actions={2: act})
    compare(a, b)


def test_auto_bypass_and_submixer_silence_gate():
    """A one-shot voice into a sub-mixer with a Gain effect and a Delay: after the source ends the effects run their tails,
    then bypass; the sub-mixer drops out of the sum after 2 s of silence (submixer.rs:47-77). 2.5 s at 48 kHz."""
    def build(g):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.8})
        g.add_effect(m, _capi.FX_DELAY, params={"dlay": 30.0, "fdbk": 0.3})
        g.add_voice(m, workloads.tone_buffer(4, 48000, 0.05), 2, 48000)
        g.add_effect(0, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(11))
        return {}
    a, b = both(build, 30, 4096)
    compare(a, b)


@pytest.mark.parametrize("name", ["headline", "c2", "c3", "c4", "c5"])
def test_benchmark_workloads_reduced(name):
    """The BASELINE.json configs at reduced voice counts (oracle finishes in seconds), 1024-frame blocks. C5 renders 45 blocks =
    46 080 frames: its Delay sits at the config's own default of 375 ms = 18 000 frames (src/effect/delay.rs:124-177), so two echoes
    come back through the wet / feedback path (SVF, saturation, DC filter) inside the run."""
    builders = {
        "headline": lambda g: workloads.build_headline(g, 6, seconds=0.2),
        "c2": lambda g: workloads.build_c2(g, 8, seconds=0.2),
        "c3": lambda g: workloads.build_c3(g, 8, seconds=0.2),
        "c4": lambda g: workloads.build_c4(g, 8, seconds=0.2),
        "c5": lambda g: workloads.build_c5(g, 4, seconds=0.2),
    }
    n_blocks = 45 if name == "c5" else 6
    a, b = both(lambda g: builders[name](g) or {}, n_blocks, 1024, max_frames=1024)
    compare(a, b)
    assert np.abs(a).max() > 1e-3
    if name == "c5":
        assert_delay_audible(a, lambda g: _build_c5_variant(g, 4, delay_wet=0.0), n_blocks, 1024)


def _build_c5_variant(g, n_voices, delay_wet):
    """C5 with the Delay's wet amount overridden (0 = the delay line's output never reaches the signal)."""
    vol = workloads.voice_level(n_voices)
    for i in range(n_voices):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_FILTER, params={"type": 0, "cuto": 8000.0, "fltq": 0.707})
        g.add_effect(m, _capi.FX_EQ5, params={"gan1": 3.0, "gan3": -4.0, "gan5": 2.0})
        g.add_effect(m, _capi.FX_DELAY, params={"wet_": delay_wet})
        g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
        g.add_voice(m, workloads.tone_buffer(i, 48000, 0.2), 2, 48000, volume=vol, panning=float(np.float32(workloads.voice_pan(i))), has_repeat=1,
                    repeat=_capi.PG_REPEAT_FOREVER)
    return {}


def assert_delay_audible(out, build_dry_only, n_blocks, block, first_echo_frame=18000):
    """The delay line's read must matter: against the same graph with the Delay fully dry (oracle), the output differs by more than
    1e-3 once the first echo is back — a delay read stubbed to zero (or a run shorter than the delay time) fails here."""
    gc = oracle.OracleGraph(SR, 2, block)
    build_dry_only(gc)
    dry = gc.render(n_blocks, block)
    late = slice(2 * first_echo_frame, None)
    assert float(np.abs(out[late].astype(np.float64) - dry[late].astype(np.float64)).max()) > 1e-3, "the delay's wet path is inaudible in this run"


def test_exact_mode_matches_fast_mode():
    """pg_graph_set_fast_math(0) forces the exact serial evaluation: both modes must agree with the oracle."""
    from phonic_amd.graph import Graph

    outs = []
    for fast in (0, 1):
        g = Graph(SR, 2, 1024, 0)
        g.set_fast_math(fast)
        workloads.build_headline(g, 3, seconds=0.2)
        outs.append(g.render(5, 1024))
    gc = oracle.OracleGraph(SR, 2, 1024)
    workloads.build_headline(gc, 3, seconds=0.2)
    ref = gc.render(5, 1024)
    compare(outs[0], ref)
    compare(outs[1], ref)


def test_write_device_matches_write():
    import torch
    from phonic_amd.graph import Graph

    g1, g2 = Graph(SR, 2, 1024, 0), Graph(SR, 2, 1024, 0)
    for g in (g1, g2):
        workloads.build_headline(g, 4, seconds=0.1)
    host = g1.render(3, 1024)
    dev = torch.zeros(3, 2048, dtype=torch.float32, device="cuda:0")
    pos = 0
    for b in range(3):
        assert g2.write_device(dev[b].data_ptr(), 2048, pos) == 2048
        pos += 1024
    g2.synchronize()
    assert np.array_equal(dev.cpu().numpy().reshape(-1), host)


def test_fast_kernel_generic_kernel_handover_on_parameter_ramp():
    """A reverb parameter change in the middle of a run: the unit leaves the time-parallel kernel for the exact per-frame
    path while room/wet ramp (delay lengths and filter coefficients change every frame) and returns afterwards."""
    def build(g):
        ids = []
        for i in range(3):
            m = g.add_mixer()
            ids.append(g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i)))
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.3), 2, 44100, volume=0.5, panning=workloads.voice_pan(i), has_repeat=1,
                        repeat=_capi.PG_REPEAT_FOREVER)
        return ids

    def act2(g, ids, pos):
        g.schedule_param(ids[0], "room", 0.2, pos + 100)
        g.schedule_param(ids[1], "wet ", 0.9, pos + 700)

    def act5(g, ids, pos):
        g.schedule_param(ids[0], "room", 0.95, pos)
        g.schedule_reset(ids[2], pos + 512)

    a, b = both(build, 10, 1024, actions={2: act2, 5: act5}, max_frames=1024)
    compare(a, b)


def test_speed_glide_and_seek():
    """FilePlaybackHandle::set_speed (immediate and with a glide in semitones/s: the resampler ratio is re-targeted every
    64 frames, common.rs:141-169) and seek (position jump + resampler reset), scheduled at sample times inside blocks."""
    def build(g):
        v0 = g.add_voice(0, workloads.tone_buffer(2, 44100, 0.4), 2, 44100, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        v1 = g.add_voice(0, workloads.tone_buffer(7, 48000, 0.4, channels=1), 1, 48000, volume=0.5, panning=0.3, has_repeat=1,
                         repeat=_capi.PG_REPEAT_FOREVER)
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(21))
        v2 = g.add_voice(m, workloads.tone_buffer(9, 44100, 0.4), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return [v0, v1, v2]

    def act1(g, ids, pos):
        g.set_voice_speed(ids[0], 1.5, pos + 200)             # immediate: ratio > 1 branch
        g.set_voice_speed(ids[1], 0.5, pos + 10, glide=48.0)  # glide down one octave at 48 st/s = 0.25 s
        g.set_voice_speed(ids[2], 2.0, pos + 333, glide=96.0)

    def act3(g, ids, pos):
        g.seek_voice(ids[0], 0.05, pos + 77)
        g.seek_voice(ids[2], 0.2, pos + 900)
        g.set_voice_speed(ids[0], 0.75, pos + 512, glide=24.0)

    a, b = both(build, 16, 1024, actions={1: act1, 3: act3}, max_frames=1024)
    compare(a, b)
    assert not np.array_equal(a[:2048], a[2048 * 8:2048 * 9])


def _render_modes(build, n_blocks, block, actions=None):
    """Renders the same graph with the staged kernel, with one launch per stage, with the fused kernel, and on the oracle."""
    from phonic_amd.graph import Graph

    outs = []
    for mode in ("staged", "per-stage", "fused", "oracle"):
        g = oracle.OracleGraph(SR, 2, block) if mode == "oracle" else Graph(SR, 2, block, 0)
        if mode != "oracle":
            g.set_staged({"staged": 1, "per-stage": 2, "fused": 0}[mode])
        ids = build(g)
        out = np.zeros((n_blocks, block * 2), np.float32)
        pos = 0
        for blk in range(n_blocks):
            if actions and blk in actions:
                actions[blk](g, ids, pos)
            w = g.write(out[blk], pos)
            assert w in (0, block * 2)
            pos += block
        outs.append(out.reshape(-1))
    return outs


def test_staged_pipeline_matches_fused_kernel_and_oracle():
    """[Gain|Panning]* -> Reverb sub-mixers go through pg_stage1/2/3_kernel by default; pg_graph_set_staged(0) keeps them
    in the fused kernel. Both must agree with each other (same stage functions, f64 rounding only) and with the oracle."""
    def build(g):
        workloads.build_headline(g, 5, seconds=0.2)
        m = g.add_mixer()   # two voices, leading Gain and Panning effects in front of the reverb
        g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.7})
        g.add_effect(m, _capi.FX_PANNING, params={"pan ": -0.3})
        g.add_effect(m, _capi.FX_REVERB, params={"room": 0.45, "wet ": 0.6}, reverb_seeds=workloads.reverb_seeds(77))
        for i in range(2):
            g.add_voice(m, workloads.tone_buffer(20 + i, 44100, 0.2), 2, 44100, volume=0.4, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return {}
    staged, per_stage, fused, ref = _render_modes(build, 8, 1024)
    assert np.array_equal(staged, per_stage)
    assert float(np.abs(staged - fused).max()) <= 2e-6
    compare(staged, ref)
    compare(fused, ref)
    assert np.abs(staged).max() > 1e-3


def test_staged_pipeline_tail_bypass_and_parameter_handover():
    """One-shot voice into a reverb sub-mixer: source ends, the reverb runs on silence (tail/silence counters, auto-bypass,
    sub-mixer silence gate); a second sub-mixer gets a room-size ramp in the middle (stage 1 defers it to the generic kernel)."""
    def build(g):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_REVERB, params={"room": 0.3}, reverb_seeds=workloads.reverb_seeds(5))
        g.add_voice(m, workloads.tone_buffer(4, 48000, 0.05), 2, 48000)
        m2 = g.add_mixer()
        fx = g.add_effect(m2, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(6))
        g.add_voice(m2, workloads.tone_buffer(9, 44100, 0.3), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return [fx]

    def act(g, ids, pos):
        g.schedule_param(ids[0], "room", 0.8, pos + 300)

    staged, per_stage, fused, ref = _render_modes(build, 130, 1024, actions={40: act})
    assert np.array_equal(staged, per_stage)
    assert float(np.abs(staged - fused).max()) <= 2e-6
    compare(staged, ref)


@pytest.mark.parametrize("rate,block,n_blocks", [(44100, 1024, 400), (32000, 1000, 60), (40000, 777, 80), (16000, 1024, 40), (22050, 512, 60), (47999, 1024, 60),
                                                 (88200, 1024, 300), (64000, 1000, 120), (50000, 777, 120), (48001, 1024, 120), (70000, 1024, 200), (96000, 512, 60),
                                                 (130000, 1024, 120), (150000, 1024, 120), (176400, 1000, 120), (100000, 640, 60), (191999, 1024, 60)])
def test_resampler_schedule_bit_exact_over_many_blocks(rate, block, n_blocks):
    """The f32 sub_pos schedule has several device implementations — the exact time-parallel ones (ratio in [0.5, 1) and in [1, 4): closed
    form + rounding-table scan, restarted where a decision differs, which happens in ~0.6 % of the blocks, hence 300-400 blocks at 44.1 and
    88.2 kHz), the schedule cache (ratio < 0.5, two voices of one class), the straight-line serial walks and the general serial replay (near
    the loop end of the 0.11 s file, every few blocks). All must equal the reference's serial recurrence bit for bit: a single unit-gain
    voice straight into the main mixer is compared with array_equal."""
    def build(g):
        return [g.add_voice(0, workloads.tone_buffer(1, rate, 0.11), 2, rate, volume=1.0, panning=0.0, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)]
    a, b = both(build, n_blocks, block, max_frames=1024)
    assert np.array_equal(a, b)
    assert np.abs(a).max() > 1e-3


def test_wide_staged_kernel_filter_eq5_delay_reverb_chain():
    """Reverb-terminated sub-mixers whose leading effects go beyond Gain / Panning (C5's Filter -> Eq5 -> Delay -> Reverb, plus a
    Distortion -> Reverb one) are rendered by pg_stage_fused_wide_kernel; pg_graph_set_staged(0) keeps them in the fused wide
    kernel. Same stage functions and effect paths: the two agree to f64 rounding, and both match the oracle. 45 blocks: the Delay
    (default 375 ms = 18 000 frames) returns two echoes inside the run."""
    def build(g):
        workloads.build_c5(g, 3, 0, 3, seconds=0.2)
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_DISTORTION, params={"type": 0, "driv": 2.0})
        g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.5})
        g.add_effect(m, _capi.FX_REVERB, params={"room": 0.35}, reverb_seeds=workloads.reverb_seeds(42))
        g.add_voice(m, workloads.tone_buffer(7, 44100, 0.2), 2, 44100, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return {}
    n_blocks = 45
    staged, _per_stage, fused, ref = _render_modes(build, n_blocks, 1024)
    assert float(np.abs(staged - fused).max()) <= 2e-6
    compare(staged, ref)
    compare(fused, ref)
    assert np.abs(staged).max() > 1e-3

    def build_dry(g):
        _build_c5_variant(g, 3, delay_wet=0.0)
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_DISTORTION, params={"type": 0, "driv": 2.0})
        g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.5})
        g.add_effect(m, _capi.FX_REVERB, params={"room": 0.35}, reverb_seeds=workloads.reverb_seeds(42))
        g.add_voice(m, workloads.tone_buffer(7, 44100, 0.2), 2, 44100, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    assert_delay_audible(staged, build_dry, n_blocks, 1024)


def test_staged_kernel_ragged_block_sizes():
    """Blocks of 1, 7, 63, 64, 65, 333, 1000 and 1024 frames through reverb sub-mixers (staged kernel: partial scan segments,
    partial sub-chunks, chunk cuts) and a Delay -> Reverb chain (wide staged kernel), against the oracle; then 2048-frame blocks,
    which the staged kernel does not take (> 1024 frames): the fused kernel renders those."""
    from phonic_amd.graph import Graph

    sizes = [1, 7, 63, 64, 65, 333, 1000, 1024, 129, 1024, 2, 511] * 2 + [2048, 2048]
    outs = []
    for mode in ("gpu", "oracle"):
        g = oracle.OracleGraph(SR, 2, 2048) if mode == "oracle" else Graph(SR, 2, 2048, 0)
        workloads.build_headline(g, 3, seconds=0.2)
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_DELAY, params={"dlay": 5.0, "fdbk": 0.5})
        g.add_effect(m, _capi.FX_REVERB, params={"room": 0.2}, reverb_seeds=workloads.reverb_seeds(8))
        g.add_voice(m, workloads.tone_buffer(3, 44100, 0.15), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        chunks, pos = [], 0
        for n in sizes:
            o = np.zeros(2 * n, np.float32)
            assert g.write(o, pos) == 2 * n
            chunks.append(o)
            pos += n
        outs.append(np.concatenate(chunks))
    compare(outs[0], outs[1])
    assert np.abs(outs[0]).max() > 1e-3


def test_sharded_voices_with_deferred_bus_and_bus_automation():
    """The multi-GPU data path on one device: two graphs hold half of the voices each (pg_graph_set_defer_bus), their partial master
    buses are summed (what the RCCL reduce does) and the root runs the bus chain — Eq5 -> Reverb -> limiter, with a parameter
    event on the Eq5 in the middle of a block — through pg_graph_process_bus_device. Must match the single graph holding
    everything (up to the f32 order of the voice sum) and the oracle."""
    import torch
    from phonic_amd.graph import Graph

    n_voices, blocks, block = 6, 8, 1024

    def build(g, lo, hi):
        ids = []
        ids.append(g.add_effect(0, _capi.FX_EQ5, params={"gan2": 4.0}))
        g.add_effect(0, _capi.FX_REVERB, params={"room": 0.4, "wet ": 0.3}, reverb_seeds=workloads.reverb_seeds(50))
        g.add_effect(0, _capi.FX_COMPRESSOR, params={"thrs": -6.0, "rato": 20.0, "look": 0.02})
        for i in range(lo, hi):
            g.add_voice(0, workloads.tone_buffer(i, 44100, 0.2), 2, 44100, volume=0.4, panning=workloads.voice_pan(i), has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return ids

    def automate(g, ids, blk, pos):
        if blk == 3:
            g.schedule_param(ids[0], "gan4", -9.0, pos + 300)
            g.schedule_param(ids[0], "frq2", 700.0, pos + 800)

    # single graph (GPU) and oracle
    outs = []
    for g in (Graph(SR, 2, block, 0), oracle.OracleGraph(SR, 2, block)):
        ids = build(g, 0, n_voices)
        o = np.zeros((blocks, 2 * block), np.float32)
        for b in range(blocks):
            automate(g, ids, b, b * block)
            assert g.write(o[b], b * block) == 2 * block
        outs.append(o.reshape(-1))
    # two shards + deferred bus on the root
    shards = [Graph(SR, 2, block, 0) for _ in range(2)]
    ids = [build(g, k * n_voices // 2, (k + 1) * n_voices // 2) for k, g in enumerate(shards)]
    for g in shards:
        g.set_defer_bus(True)
    parts = [torch.zeros(2 * block, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    sharded = np.zeros((blocks, 2 * block), np.float32)
    for b in range(blocks):
        for g, i in zip(shards, ids):
            automate(g, i, b, b * block)
        for g, p in zip(shards, parts):
            assert g.write_device(p.data_ptr(), 2 * block, b * block) == 2 * block
            g.synchronize()
        bus = parts[0] + parts[1]
        shards[0].process_bus_device(bus.data_ptr(), 2 * block, b * block)
        shards[0].synchronize()
        sharded[b] = bus.cpu().numpy()
    sharded = sharded.reshape(-1)
    compare(outs[0], outs[1])
    compare(sharded, outs[1])
    assert float(np.abs(sharded - outs[0]).max()) <= 1e-5
    assert np.abs(sharded).max() > 1e-3


def test_deferred_bus_words_follow_the_pieces_when_events_cut_the_call():
    """Round-4 advisor finding: the `audible` word of a deferred-bus write sat at done / max_frames — a main-mixer event that cuts a chunk at a
    frame that is no multiple of max_frames (here: a source's volume event at +500, a bus parameter at +700) put the next chunk's flag into the
    same word, and the bus chain indexed the words by its own cuts. Now: one word per piece in order (pg_graph_audible_words), and the chain
    walks the grid the write recorded. (a) ONE graph, deferred: write + export + process_bus_device_flags must equal the same graph rendering
    its bus chain itself, BIT FOR BIT — one-shots end, the Delay rings out and the chain bypasses itself (exact zeros), so a wrong flag shows.
    (b) two graphs (two ranks' worth) whose calls end at the main-mixer events of either (pg_graph_next_main_event): equal to the oracle."""
    import torch
    from phonic_amd.graph import Graph

    N, blocks = 1024, 110

    def build(g, lo, hi, bus=True):
        ids = []
        for i in range(lo, hi):   # main-mixer one-shots, ~1.4 blocks long, starting in block 2
            ids.append(g.add_voice(0, workloads.tone_buffer(i, 48000, 0.03), 2, 48000, volume=0.5, start_time=2 * N + 37 * i))
        fx = []
        if bus:
            fx.append(g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.8}))
            fx.append(g.add_effect(0, _capi.FX_DELAY, params={"dlay": 30.0, "fdbk": 0.3, "wet_": 0.6}))
        return ids, fx

    def automate(g, ids, fx, b, pos, lo=0):
        if b == 2:
            if lo == 0:
                g.set_voice_volume(ids[0], 0.2, pos + 500)
            if fx:
                g.schedule_param(fx[1], "fdbk", 0.35, pos + 700)
        if b == 3 and lo == 0:
            g.set_voice_panning(ids[1], -0.5, pos + 1000)

    # reference renders: the plain graph and the oracle, block by block
    outs = []
    for g in (Graph(SR, 2, N, 0), oracle.OracleGraph(SR, 2, N)):
        ids, fx = build(g, 0, 4)
        o = np.zeros((blocks, 2 * N), np.float32)
        for b in range(blocks):
            automate(g, ids, fx, b, b * N)
            w = g.write(o[b], b * N)
            assert w in (0, 2 * N)
        outs.append(o.reshape(-1))
    compare(outs[0], outs[1])
    assert np.abs(outs[0]).max() > 1e-2 and np.abs(outs[0][-2 * N:]).max() == 0.0   # the chain has bypassed itself at the end

    # (a) one graph, bus deferred
    g = Graph(SR, 2, N, 0)
    g.set_defer_bus(True)
    ids, fx = build(g, 0, 4)
    buf = torch.zeros(2 * N + 64, dtype=torch.float32, device="cuda:0")
    a = np.zeros((blocks, 2 * N), np.float32)
    words_seen = set()
    for b in range(blocks):
        automate(g, ids, fx, b, b * N)
        buf.zero_()
        w = g.write_device(buf.data_ptr(), 2 * N, b * N)
        g.synchronize()
        nw = g.audible_words()
        words_seen.add(nw)
        if w:
            assert w == 2 * N
            g.export_audible(buf.data_ptr() + 4 * 2 * N, nw)
        g.process_bus_device(buf.data_ptr(), 2 * N, b * N, flags_ptr=buf.data_ptr() + 4 * 2 * N if w else None, n_words=max(nw, 1) if w else 0)
        g.synchronize()
        a[b] = buf[: 2 * N].cpu().numpy()
    assert {1, 3} <= words_seen, words_seen    # block 2 is three pieces: [0, 500) [500, 700) [700, 1024)
    assert np.array_equal(a.reshape(-1), outs[0])
    assert g.device_errors() == 0

    # (b) two graphs, calls cut at the main-mixer events of either
    gs = [Graph(SR, 2, N, 0), Graph(SR, 2, N, 0)]
    built = [build(gs[0], 0, 2), build(gs[1], 2, 4)]
    # (the voices are the oracle's 0..3 split over the two graphs; the events of voice 0 / 1 live on graph 0 only)
    for g in gs:
        g.set_defer_bus(True)
    bufs = [torch.zeros(2 * N + 64, dtype=torch.float32, device="cuda:0") for _ in gs]
    o = np.zeros((blocks, 2 * N), np.float32)
    for b in range(blocks):
        for k, g in enumerate(gs):
            automate(g, built[k][0], built[k][1], b, b * N, lo=2 * k)
        done = 0
        while done < N:
            pos = b * N + done
            n = N - done
            for g in gs:
                t = g.next_main_event(pos)
                if t is not None:
                    n = min(n, t - pos)
            total = None
            for g, bf in zip(gs, bufs):
                bf.zero_()
                w = g.write_device(bf.data_ptr(), 2 * n, pos)
                g.synchronize()
                assert w in (0, 2 * n)
                nw = g.audible_words() if w else 0
                assert nw in (0, 1)
                if w:
                    g.export_audible(bf.data_ptr() + 4 * 2 * n, 1)
                total = bf.clone() if total is None else total + bf
            gs[0].process_bus_device(total.data_ptr(), 2 * n, pos, flags_ptr=total.data_ptr() + 4 * 2 * n, n_words=1)
            gs[0].synchronize()
            o[b, 2 * done: 2 * (done + n)] = total[: 2 * n].cpu().numpy()
            done += n
    compare(o.reshape(-1), outs[1])
    assert np.abs(o[-1]).max() == 0.0


@pytest.mark.parametrize("per_call", [1, 4])
def test_dynamic_workload_plan_matches_the_oracle(per_call):
    """bench.py --workload dyn in small: 24 per-voice Reverb sub-mixers, a quarter of the voices short one-shots, voices that are stopped and
    restarted at random sample times (successors added up front with their start times), reverb `wet` / source volume / source panning commands at
    random sample times — the SAME plan (phonic_amd.workloads.DynDriver) drives the product graph and the oracle through the same calls (one
    block per call, and four: super-block launches where the library finds a steady span, pieces where commands fall)."""
    from phonic_amd.graph import Graph

    N, blocks = 1024, 48
    outs = []
    for mode in ("gpu", "oracle"):
        g = Graph(SR, 2, N, 0) if mode == "gpu" else oracle.OracleGraph(SR, 2, N)
        if mode == "gpu":
            g.set_max_blocks_per_launch(per_call)
        plan = workloads.build_dyn(g, 24, blocks * N / SR, churn_pct_per_s=60.0, silent_pct=25.0, first_frame=4 * N, seed=99, sample_rate=SR)
        assert len(plan["restarts"]) >= 8 and len(plan["silent"]) == 6
        drv = workloads.DynDriver(plan, 150.0, 7, sample_rate=SR)
        o = np.zeros((blocks // per_call, per_call * 2 * N), np.float32)
        n_cmds = 0
        for c in range(blocks // per_call):
            pos = c * per_call * N
            if c * per_call >= 4:
                n_cmds += drv.schedule(g, pos, pos + per_call * N)
            assert g.write(o[c], pos) == o[c].size
        assert n_cmds > 100
        outs.append(o.reshape(-1))
        if mode == "gpu":
            assert g.device_errors() == 0
            st = g.dynamic_stats()
            assert st["unit_blocks"] >= 24 * blocks and 0 < st["deferred_unit_blocks"] < st["unit_blocks"]
    compare(outs[0], outs[1])
    assert np.abs(outs[0]).max() > 1e-2


def test_nested_submixers_tree():
    """Player::add_mixer(parent) (src/player.rs:771-822): main -> group (Eq5, Compressor, own voice) -> {reverb send, filter+chorus
    lane} -> a third level under the lane. The parent sums its sub-mixers in the order they were added, then its sources, then
    runs its chain (mixed.rs:696-703)."""
    def build(g):
        group = g.add_mixer()
        g.add_effect(group, _capi.FX_EQ5, params={"gan1": 3.0, "gan4": -4.0})
        g.add_effect(group, _capi.FX_COMPRESSOR, params={"thrs": -24.0, "rato": 4.0})
        send = g.add_mixer(group)
        g.add_effect(send, _capi.FX_GAIN, params={"gain": 0.7})
        g.add_effect(send, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(3))
        g.add_voice(send, workloads.tone_buffer(7, 44100, 0.2), 2, 44100, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        lane = g.add_mixer(group)
        g.add_effect(lane, _capi.FX_FILTER, params={"cuto": 1800.0})
        g.add_effect(lane, _capi.FX_CHORUS)
        g.add_voice(lane, workloads.tone_buffer(19, 48000, 0.2), 2, 48000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        leaf = g.add_mixer(lane)
        g.add_effect(leaf, _capi.FX_DISTORTION, params={"driv": 0.6})
        g.add_voice(leaf, workloads.tone_buffer(31, 32000, 0.2), 2, 32000, panning=-0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        g.add_voice(group, workloads.tone_buffer(2, 48000, 0.2), 2, 48000, panning=0.4, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        other = g.add_mixer()
        g.add_effect(other, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(9))
        g.add_voice(other, workloads.tone_buffer(40, 44100, 0.2), 2, 44100, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        g.add_voice(0, workloads.tone_buffer(11, 48000, 0.1), 2, 48000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.9})
        return {}
    a, b = both(build, 12, 1024, max_frames=1024)
    assert float(np.abs(b).max()) > 0.05
    compare(a, b)


def test_nested_submixer_events_split_child_calls():
    """Events on a mixer with sub-mixers split its block (mixed.rs:679-712) and so the write() calls of its sub-mixers: the nested
    one-shot voice ends, its delay tail runs out and the per-call silence gate (submixer.rs:47-77) closes while the parent keeps
    receiving parameter and voice events at odd frames. Unknown parent ids are rejected."""
    def build(g):
        group = g.add_mixer()
        fx = g.add_effect(group, _capi.FX_FILTER, params={"cuto": 4000.0})
        own = g.add_voice(group, workloads.tone_buffer(12, 48000, 0.3), 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        child = g.add_mixer(group)
        g.add_effect(child, _capi.FX_DELAY, params={"dlay": 40.0, "fdbk": 0.4})
        g.add_voice(child, workloads.tone_buffer(4, 48000, 0.05), 2, 48000)
        grand = g.add_mixer(child)
        cfx = g.add_effect(grand, _capi.FX_GAIN, params={"gain": 0.5})
        g.add_voice(grand, workloads.tone_buffer(25, 44100, 0.04), 2, 44100)
        with pytest.raises(Exception):
            g.add_mixer(99)
        return {"fx": fx, "own": own, "cfx": cfx}

    def ev(g, ids, pos):
        g.schedule_param(ids["fx"], "cuto", 0.2 + 0.01 * (pos % 7), pos + 301, normalized=True)
        g.set_voice_volume(ids["own"], 0.4, pos + 777)
        g.set_voice_volume(ids["own"], 0.6, pos + 777)
        g.schedule_param(ids["cfx"], "gain", 0.3, pos + 500, normalized=True)
    actions = {k: ev for k in (1, 2, 5, 30, 60, 100, 101, 102, 110)}
    a, b = both(build, 112, 1024, actions=actions, max_frames=1024)
    compare(a, b)


def test_write_device_does_not_touch_memory_past_the_block():
    """An odd frame count ends in the middle of the mixer sum's last float4: the samples behind the block stay untouched."""
    import torch
    from phonic_amd.graph import Graph

    g = Graph(SR, 2, 1024, 0)
    m = g.add_mixer()
    g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(1))
    g.add_voice(m, workloads.tone_buffer(10, 44100, 0.2), 2, 44100, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    g.add_voice(0, workloads.tone_buffer(20, 48000, 0.2), 2, 48000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    pos = 0
    for frames in (333, 1, 1023, 7):
        buf = torch.full((2 * frames + 8,), 7.0, dtype=torch.float32, device="cuda:0")
        assert g.write_device(buf.data_ptr(), 2 * frames, pos) == 2 * frames
        h = buf.cpu().numpy()
        assert np.all(h[2 * frames:] == 7.0), (frames, h[2 * frames:])
        assert np.all(np.abs(h[:2 * frames]) < 1.0)
        pos += frames


def test_odd_max_frames_graph():
    """max_frames = 333: unit rows start 8-byte (not 16-byte) aligned, blocks end inside a float4 — staged reverb units, a plain
    source, a bus effect, resampled voices."""
    def build(g):
        for i in range(3):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.8})
            g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(20 + i))
            g.add_voice(m, workloads.tone_buffer(5 + 7 * i, 44100, 0.2), 2, 44100, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        g.add_voice(0, workloads.tone_buffer(33, 48000, 0.2), 2, 48000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        g.add_effect(0, _capi.FX_FILTER, params={"cuto": 5000.0})
        return {}
    a, b = both(build, 9, 333, max_frames=333)
    assert float(np.abs(b).max()) > 0.05
    compare(a, b)


def test_gain_with_dc_filter_takes_the_time_parallel_path():
    """GainEffect with its DC filter on (gain.rs:147-153) in sub-mixer chains: alone, in front of a Reverb (wide staged kernel) and
    behind a Filter; the DC filter runs as a blocked scan (no deferral to the serial kernel in steady state). A fourth sub-mixer
    starts as a plain [Gain -> Reverb] chain of the lean staged kernel and gets its DC filter switched on by a parameter event
    in the middle of a block: the chain is classified again and moves to the wide variants."""
    def build(g):
        m1 = g.add_mixer()
        g.add_effect(m1, _capi.FX_GAIN, params={"gain": 0.7, "dcfm": 2})
        g.add_voice(m1, workloads.tone_buffer(3, 44100, 0.3) + 0.02, 2, 44100, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m2 = g.add_mixer()
        g.add_effect(m2, _capi.FX_GAIN, params={"gain": 1.3, "dcfm": 3})
        g.add_effect(m2, _capi.FX_REVERB, params={"room": 0.4}, reverb_seeds=workloads.reverb_seeds(11))
        g.add_voice(m2, workloads.tone_buffer(8, 48000, 0.25) - 0.01, 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m3 = g.add_mixer()
        g.add_effect(m3, _capi.FX_FILTER, params={"type": 0, "cuto": 3000.0})
        g.add_effect(m3, _capi.FX_GAIN, params={"gain": 0.9, "dcfm": 1})
        g.add_voice(m3, workloads.tone_buffer(15, 44100, 0.2), 2, 44100, volume=0.4, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m4 = g.add_mixer()
        fx = g.add_effect(m4, _capi.FX_GAIN, params={"gain": 0.8})
        g.add_effect(m4, _capi.FX_REVERB, params={"room": 0.5}, reverb_seeds=workloads.reverb_seeds(12))
        g.add_voice(m4, workloads.tone_buffer(21, 44100, 0.3) + 0.03, 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return [fx]

    def act(g, ids, pos):
        g.schedule_param(ids[0], "dcfm", 2, pos + 2500)  # lands two blocks later, 452 frames into the block

    a, b = both(build, 24, 1024, actions={6: act})
    compare(a, b)
    assert np.abs(a).max() > 1e-2
    for blk in (512, 1000, 1023):  # ragged blocks through the same chains
        a, b = both(build, 9, blk, actions={3: act})
        compare(a, b)
    # the time-parallel kernels keep these chains: nothing is handed to the serial kernel in steady state, the block that holds the
    # parameter event is (one unit), and the re-classified chain is back on the time-parallel path afterwards
    from phonic_amd.graph import Graph

    g = Graph(SR, 2, 1024, 0)
    ids = build(g)
    out = np.zeros(2048, np.float32)
    pos = 0
    for _ in range(4):
        g.write(out, pos); pos += 1024
    assert g.deferred_units() == 0
    g.schedule_param(ids[0], "dcfm", 2, pos + 100)
    g.write(out, pos); pos += 1024
    assert g.deferred_units() >= 1  # (the re-classification marks every unit of the graph for one block)
    for _ in range(3):
        g.write(out, pos); pos += 1024
    assert g.deferred_units() == 0


def test_remove_and_move_effects_between_blocks():
    """Player::move_effect / remove_effect (MixerMessage::MoveEffect / RemoveEffect, mixed.rs:433-462) on a sub-mixer chain and on the
    main mixer's bus chain: the chain order changes at the start of the next write, every effect keeps its state (filters, delay
    lines, bypass counters) across the move; a removed effect's pending parameter events vanish and its id is gone."""
    def build(g):
        m = g.add_mixer()
        a = g.add_effect(m, _capi.FX_DISTORTION, params={"type": 1, "driv": 4.0})
        b = g.add_effect(m, _capi.FX_FILTER, params={"type": 0, "cuto": 900.0})
        c = g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.5})
        d = g.add_effect(m, _capi.FX_REVERB, params={"room": 0.3}, reverb_seeds=workloads.reverb_seeds(21))
        g.add_voice(m, workloads.tone_buffer(6, 44100, 0.3), 2, 44100, volume=0.9, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        e = g.add_effect(0, _capi.FX_EQ5, params=None)
        f = g.add_effect(0, _capi.FX_DELAY, params={"dlay": 20.0})
        g.add_voice(0, workloads.tone_buffer(12, 48000, 0.2), 2, 48000, volume=0.3, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return dict(m=m, a=a, b=b, c=c, d=d, e=e, f=f)

    def act3(g, ids, pos):   # filter in front of the distortion: [b a c d]
        g.move_effect(ids["b"], ids["m"], _capi.MOVE_START)
    def act5(g, ids, pos):   # reverb one step towards the start: [b a d c] (no longer reverb-terminated), bus: [f e]
        g.move_effect(ids["d"], ids["m"], _capi.MOVE_DIRECTION, -1)
        g.move_effect(ids["e"], 0, _capi.MOVE_END)
        g.schedule_param(ids["a"], "driv", 1.0, pos + 5000)  # never fires: the effect is removed first
    def act7(g, ids, pos):   # distortion leaves, the move of a removed / foreign effect is refused
        g.remove_effect(ids["a"])
        for call in (lambda: g.remove_effect(ids["a"]), lambda: g.schedule_param(ids["a"], "driv", 2.0, pos), lambda: g.move_effect(ids["a"], ids["m"], _capi.MOVE_END),
                     lambda: g.move_effect(ids["b"], 0, _capi.MOVE_END)):
            with pytest.raises(Exception):
                call()
    def act9(g, ids, pos):   # clamped direction moves, reverb back to the end: [b c d]; bus delay removed: [e]
        g.move_effect(ids["d"], ids["m"], _capi.MOVE_DIRECTION, 7)
        g.move_effect(ids["b"], ids["m"], _capi.MOVE_DIRECTION, -3)
        g.remove_effect(ids["f"])
    def act12(g, ids, pos):  # chain emptied
        for k in ("b", "c", "d"):
            g.remove_effect(ids[k])

    actions = {3: act3, 5: act5, 7: act7, 9: act9, 12: act12}
    a, b = both(build, 16, 1024, actions=actions)
    compare(a, b)
    assert np.abs(a[-2048:]).max() > 1e-3
    # each rearrangement is audible: the same graph without the actions differs block for block after the first one
    a0, _ = both(build, 16, 1024)
    assert np.array_equal(a[: 3 * 2048], a0[: 3 * 2048]) and np.abs(a[3 * 2048 :] - a0[3 * 2048 :]).max() > 1e-3


def test_remove_mixer_with_nested_children_and_pending_events():
    """Player::remove_mixer (MixerMessage::RemoveMixer, mixed.rs:422-424): a sub-mixer of the main mixer, a nested sub-mixer (its parent
    goes back to the time-parallel kernels once it has no children left) and a whole branch with children, effects, voices and
    pending events leave between blocks; their ids are unknown afterwards; with the last sub-mixer gone and no sources the main
    mixer writes nothing."""
    def build(g):
        m1 = g.add_mixer()
        g.add_effect(m1, _capi.FX_REVERB, params={"room": 0.4}, reverb_seeds=workloads.reverb_seeds(31))
        v1 = g.add_voice(m1, workloads.tone_buffer(2, 44100, 0.3), 2, 44100, volume=0.7, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m2 = g.add_mixer()
        f2 = g.add_effect(m2, _capi.FX_FILTER, params={"type": 0, "cuto": 1500.0})
        g.add_voice(m2, workloads.tone_buffer(9, 48000, 0.3), 2, 48000, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m3 = g.add_mixer(m2)
        g.add_effect(m3, _capi.FX_CHORUS)
        g.add_voice(m3, workloads.tone_buffer(14, 44100, 0.3), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m4 = g.add_mixer(m2)
        f4 = g.add_effect(m4, _capi.FX_GAIN, params={"gain": 0.8})
        v4 = g.add_voice(m4, workloads.tone_buffer(17, 48000, 0.3), 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return dict(m1=m1, m2=m2, m3=m3, m4=m4, v1=v1, v4=v4, f2=f2, f4=f4)

    def act2(g, ids, pos):
        g.schedule_param(ids["f4"], "gain", 0.2, pos + 3000)   # dies with m4
        g.set_voice_volume(ids["v4"], 0.1, pos + 2500)
        g.remove_mixer(ids["m4"])
        for call in (lambda: g.remove_mixer(ids["m4"]), lambda: g.add_effect(ids["m4"], _capi.FX_GAIN), lambda: g.schedule_param(ids["f4"], "gain", 0.3, pos),
                     lambda: g.set_voice_volume(ids["v4"], 0.3, pos), lambda: g.remove_mixer(0), lambda: g.add_mixer(ids["m4"])):
            with pytest.raises(Exception):
                call()
    def act4(g, ids, pos):
        g.remove_mixer(ids["m3"])       # m2 has no children left
    def act7(g, ids, pos):
        g.remove_mixer(ids["m1"])
    def act9(g, ids, pos):
        g.schedule_param(ids["f2"], "cuto", 400.0, pos + 100)

    a, b = both(build, 12, 1024, actions={2: act2, 4: act4, 7: act7, 9: act9})
    compare(a, b)
    assert np.abs(a[-2048:]).max() > 1e-3

    def act_all(g, ids, pos):
        g.remove_mixer(ids["m2"])       # the whole branch: m2, m3, m4
        g.remove_mixer(ids["m1"])
        with pytest.raises(Exception):
            g.remove_mixer(ids["m3"])
    gg, gc = graphs()
    for g in (gg, gc):
        ids = build(g)
        out = np.full(2048, 5.0, np.float32)
        assert g.write(out, 0) == 2048
        act_all(g, ids, 1024)
        out[:] = 5.0
        assert g.write(out, 1024) == 0 and np.all(out == 5.0)


def test_stop_all_voices_and_pending_events():
    """Player::stop_all_sources (player.rs:1012-1045): playing sources fade out from the next block on (default 50 ms fade-out), a
    source scheduled for later never starts, events scheduled after the next write's position are dropped (MixerMessage::
    RemoveAllPendingEvents, mixed.rs:298-305) while one due exactly at that position still fires; sources added afterwards play."""
    def build(g):
        m = g.add_mixer()
        fx = g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.9})
        v0 = g.add_voice(m, workloads.tone_buffer(4, 44100, 0.5), 2, 44100, volume=0.8, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        v1 = g.add_voice(0, workloads.tone_buffer(10, 48000, 0.5), 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        late_sub = g.add_voice(m, workloads.tone_buffer(7, 44100, 0.5), 2, 44100, start_time=6000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        late_main = g.add_voice(0, workloads.tone_buffer(8, 48000, 0.5), 2, 48000, start_time=9000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return dict(m=m, fx=fx, v0=v0, v1=v1, late_sub=late_sub, late_main=late_main)

    def act3(g, ids, pos):
        g.schedule_param(ids["fx"], "gain", 0.3, pos)          # due at the next write's position: survives
        g.schedule_param(ids["fx"], "gain", 2.0, pos + 10)     # later: dropped
        g.set_voice_volume(ids["v1"], 1.0, pos + 700)          # dropped
        g.stop_all_voices()
    def act9(g, ids, pos):
        g.add_voice(ids["m"], workloads.tone_buffer(20, 44100, 0.2), 2, 44100, volume=0.4, start_time=pos + 100)

    a, b = both(build, 14, 1024, actions={3: act3, 9: act9})
    compare(a, b)
    blk = lambda i: a[i * 2048 : (i + 1) * 2048]
    assert np.abs(blk(2)).max() > 0.02 and np.abs(blk(3)).max() > 1e-3    # fading
    assert np.abs(blk(7)).max() < 1e-4 and np.abs(blk(8)).max() < 1e-4    # 50 ms later: silence; the late sources never start
    assert np.abs(blk(10)).max() > 1e-3                                     # the source added afterwards plays


@pytest.mark.parametrize("shape", [0, 1, 2, 3, 4])
def test_delay_with_lfo_on_time_and_feedback_takes_the_time_parallel_path(shape):
    """DelayEffect with its LFO modulating delay time and / or feedback (delay.rs:343-372):
    per-frame tap positions, feedback and filter coefficients from the exact f32 phase sequence, chunk length from the shortest delay of
    the sweep. Every deterministic LFO shape, stereo and ping-pong, a fast LFO; nothing is handed to the serial kernel in steady state."""
    def build(g):
        m1 = g.add_mixer()
        g.add_effect(m1, _capi.FX_DELAY, params={"dlay": 120.0, "fdbk": 0.6, "lfor": 7.3, "lfos": shape, "lfdt": 0.6, "ldfb": -0.5})
        g.add_voice(m1, workloads.tone_buffer(5, 44100, 0.3), 2, 44100, volume=0.8, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m2 = g.add_mixer()
        g.add_effect(m2, _capi.FX_DELAY, params={"mode": 1, "dlay": 30.0, "fdbk": 0.4, "lfor": 0.8, "lfos": shape, "lfdt": -0.2, "driv": 0.3})
        g.add_effect(m2, _capi.FX_REVERB, params={"room": 0.3}, reverb_seeds=workloads.reverb_seeds(51))
        g.add_voice(m2, workloads.tone_buffer(13, 48000, 0.3), 2, 48000, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m3 = g.add_mixer()
        g.add_effect(m3, _capi.FX_DELAY, params={"dlay": 250.0, "fdbk": 0.7, "lfor": 2.0, "lfos": shape, "ldfb": 0.9})
        g.add_voice(m3, workloads.tone_buffer(19, 44100, 0.3), 2, 44100, volume=0.7, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        # LFO -> filter cutoff: per-frame SVF coefficients (time-varying blocked scan), each filter type, alone and with the other two
        for i, (ftyp, extra) in enumerate(((0, {}), (1, {"lfdt": 0.3}), (2, {"ldfb": 0.4, "lfdt": -0.5}))):
            m = g.add_mixer()
            p = {"dlay": 90.0 + 40.0 * i, "fdbk": 0.65, "ftyp": ftyp, "cuto": 1500.0 + 900.0 * i, "lfor": 3.1 + i, "lfos": shape, "lfdf": 0.8 - 0.7 * i, "driv": 0.2 * i}
            p.update(extra)
            g.add_effect(m, _capi.FX_DELAY, params=p)
            g.add_voice(m, workloads.tone_buffer(23 + i, 44100, 0.3), 2, 44100, volume=0.7, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return {}

    for blk, n in ((1024, 30), (700, 12)):
        a, b = both(build, n, blk, max_frames=1024)
        compare(a, b)
        assert np.abs(a[-2048:]).max() > 1e-3
    from phonic_amd.graph import Graph

    g = Graph(SR, 2, 1024, 0)
    build(g)
    out = np.zeros(2048, np.float32)
    for i in range(5):
        g.write(out, i * 1024)
    assert g.deferred_units() == 0


@pytest.mark.parametrize("shape", [5, 6])
def test_delay_with_the_random_lfo_shapes_from_an_explicit_seed(shape):
    """LfoWaveform::Random (sample & hold) and SmoothRandom (cosine-interpolated jitter), src/utils/dsp/lfo.rs:145-169,241-252: the reference
    seeds their SmallRng from the OS; with the generator's state as an explicit input (pg_effect_init::lfo_rng_state, Xoshiro256++ = rand 0.9's
    SmallRng) the device and the oracle draw the same sequence — at construction (three values), on every phase wrap (a 9 Hz LFO wraps ~ 4 times
    per block), and again on a Reset message. Routed to time, feedback and filter at once; also switched to from a deterministic shape by a
    parameter event, with the default seed, and on the bus. Random shapes take the exact serial lane (the fast paths decline them)."""
    seed = (0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978, 0x1122334455667788)

    def build(g):
        m1 = g.add_mixer()
        d1 = g.add_effect(m1, _capi.FX_DELAY, params={"dlay": 60.0, "fdbk": 0.55, "lfor": 9.0, "lfos": shape, "lfdt": 0.5, "ldfb": -0.4, "lfdf": 0.6}, lfo_seed=seed)
        g.add_voice(m1, workloads.tone_buffer(5, 44100, 0.3), 2, 44100, volume=0.8, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m2 = g.add_mixer()
        d2 = g.add_effect(m2, _capi.FX_DELAY, params={"mode": 1, "dlay": 25.0, "fdbk": 0.4, "lfor": 3.0, "lfos": 1, "lfdt": -0.3})      # default seed, shape set later
        g.add_effect(m2, _capi.FX_REVERB, params={"room": 0.3}, reverb_seeds=workloads.reverb_seeds(52))
        g.add_voice(m2, workloads.tone_buffer(13, 48000, 0.3), 2, 48000, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        d3 = g.add_effect(0, _capi.FX_DELAY, params={"dlay": 15.0, "fdbk": 0.3, "wet_": 0.3, "lfor": 5.0, "lfos": shape, "lfdt": 0.2}, lfo_seed=(7, 8, 9, 10))
        return {"d1": d1, "d2": d2, "d3": d3}

    def at4(g, ids, pos):
        g.schedule_param(ids["d2"], "lfos", shape, pos + 333)
        g.schedule_reset(ids["d1"], pos + 700)

    def at8(g, ids, pos):
        g.schedule_param(ids["d1"], "lfos", 11 - shape, pos + 10)       # the other random shape: same state, other read-out
        g.schedule_reset(ids["d3"], pos + 512)

    a, b = both(build, 14, 1024, actions={4: at4, 8: at8}, max_frames=1024)
    compare(a, b)
    assert np.abs(a[-2048:]).max() > 1e-3
    # a different seed gives different audio: the generator is really in the path
    def build_other(g):
        m1 = g.add_mixer()
        g.add_effect(m1, _capi.FX_DELAY, params={"dlay": 60.0, "fdbk": 0.55, "lfor": 9.0, "lfos": shape, "lfdt": 0.5, "ldfb": -0.4, "lfdf": 0.6}, lfo_seed=(1, 2, 3, 4))
        g.add_voice(m1, workloads.tone_buffer(5, 44100, 0.3), 2, 44100, volume=0.8, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return {}
    c, d = both(build_other, 6, 1024, max_frames=1024)
    compare(c, d)
    from phonic_amd.graph import Graph

    def first_sub_mixer_only(seed_):
        g = Graph(SR, 2, 1024, 0)
        m1 = g.add_mixer()
        g.add_effect(m1, _capi.FX_DELAY, params={"dlay": 60.0, "fdbk": 0.55, "lfor": 9.0, "lfos": shape, "lfdt": 0.5, "ldfb": -0.4, "lfdf": 0.6}, lfo_seed=seed_)
        g.add_voice(m1, workloads.tone_buffer(5, 44100, 0.3), 2, 44100, volume=0.8, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return g.render(6, 1024)
    assert np.array_equal(first_sub_mixer_only((1, 2, 3, 4)), c)
    assert np.abs(first_sub_mixer_only(seed) - c).max() > 1e-3


@pytest.mark.parametrize("ftype", [0, 1, 2, 3])
def test_filter_cutoff_and_q_ramps_take_the_time_parallel_path(ftype):
    """FilterEffect while cutoff and Q ramp (filter.rs:166-192: coefficients recomputed every frame): smoother value sequences laid out
    exactly, per-frame coefficients, time-varying blocked scan. Every filter type, ramps that start mid-block, overlap and end
    mid-block; also in front of a Reverb (wide staged kernel). After the block that holds the parameter event the unit is back on
    the time-parallel kernels although the ramp is still running."""
    def build(g):
        m1 = g.add_mixer()
        f1 = g.add_effect(m1, _capi.FX_FILTER, params={"type": ftype, "cuto": 4000.0, "fltq": 0.9})
        g.add_voice(m1, workloads.tone_buffer(6, 44100, 0.3), 2, 44100, volume=0.8, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        g.add_voice(m1, workloads.tone_buffer(30, 48000, 0.3), 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m2 = g.add_mixer()
        f2 = g.add_effect(m2, _capi.FX_FILTER, params={"type": ftype, "cuto": 800.0})
        g.add_effect(m2, _capi.FX_REVERB, params={"room": 0.3}, reverb_seeds=workloads.reverb_seeds(61))
        g.add_voice(m2, workloads.tone_buffer(11, 44100, 0.3), 2, 44100, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return dict(f1=f1, f2=f2)

    def act2(g, ids, pos):
        g.schedule_param(ids["f1"], "cuto", 300.0, pos + 333)
        g.schedule_param(ids["f2"], "cuto", 6000.0, pos + 900)
    def act4(g, ids, pos):
        g.schedule_param(ids["f1"], "fltq", 3.0, pos + 10)
    def act9(g, ids, pos):
        g.schedule_param(ids["f1"], "cuto", 9000.0, pos + 512)
        g.schedule_param(ids["f1"], "fltq", 0.3, pos + 700)

    for blk, n in ((1024, 40), (600, 30)):
        a, b = both(build, n, blk, actions={2: act2, 4: act4, 9: act9}, max_frames=1024)
        compare(a, b)
        assert np.abs(a).max() > 1e-2
    from phonic_amd.graph import Graph

    g = Graph(SR, 2, 1024, 0)
    ids = build(g)
    out = np.zeros(2048, np.float32)
    for i in range(3):
        g.write(out, i * 1024)
    g.schedule_param(ids["f1"], "fltq", 3.5, 3 * 1024 + 5)   # Q: linear steps of 0.01 per frame at 44.1 kHz -> some hundred frames
    g.schedule_param(ids["f1"], "cuto", 200.0, 3 * 1024 + 5)
    g.write(out, 3 * 1024)
    assert g.deferred_units() >= 1
    g.write(out, 4 * 1024)
    g.write(out, 5 * 1024)
    assert g.deferred_units() == 0


def test_superblock_launch_is_bit_identical_to_single_blocks():
    """pg_graph_set_max_blocks_per_launch: a write call spanning several blocks of max_frames is rendered by ONE launch sequence whose
    workgroups loop over the blocks of their unit (steady state, nothing scheduled inside). Every per-block decision stays per block,
    so the result must equal the block-by-block render BIT FOR BIT: staged lean units (headline), staged wide units (C5 chain), fused
    units (Filter -> Chorus), plain main-mixer sources incl. two voices of one resampler-schedule-cache class (ratio < 0.5), a one-shot
    voice whose reverb tail runs out, auto-bypasses and closes the sub-mixer's 2 s silence gate inside super-blocks, and parameter /
    voice events that split super-blocks at their sample times. Also checked against the oracle, and that super-block launches really
    happened (blocks per timed launch > 1) without any consistency flag from the kernels."""
    from phonic_amd.graph import Graph

    N, per_call, calls = 1024, 8, 15

    def build(g):
        workloads.build_headline(g, 3, seconds=0.2)
        workloads.build_c5(g, 2, 0, 2, seconds=0.2)
        workloads.build_c3(g, 2, 0, 2, seconds=0.2)
        for i in range(2):
            g.add_voice(0, workloads.tone_buffer(3 + i, 16000, 0.2), 2, 16000, volume=0.2, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m = g.add_mixer()
        rv = g.add_effect(m, _capi.FX_REVERB, params={"room": 0.2}, reverb_seeds=workloads.reverb_seeds(61))
        g.add_voice(m, workloads.tone_buffer(8, 48000, 0.05), 2, 48000, volume=0.5)
        m2 = g.add_mixer()
        rv2 = g.add_effect(m2, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(62))
        v2 = g.add_voice(m2, workloads.tone_buffer(12, 44100, 0.3), 2, 44100, volume=0.4, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return {"rv2": rv2, "v2": v2}

    def events(g, ids, call, pos):
        if call == 3:
            g.schedule_param(ids["rv2"], "room", 0.8, pos + 3 * N + 100)     # inside the 4th block of the call
            g.set_voice_volume(ids["v2"], 0.2, pos + 6 * N)                  # exactly on a block boundary
        if call == 9:
            g.schedule_param(ids["rv2"], "wet ", 0.6, pos + 17)

    outs, stats = [], []
    for mode in ("single", "super", "oracle"):
        g = oracle.OracleGraph(SR, 2, N) if mode == "oracle" else Graph(SR, 2, N, 0)
        if mode == "super":
            g.set_max_blocks_per_launch(per_call)
        if mode != "oracle":
            g.set_timing_period(1)
        ids = build(g)
        chunks, pos = [], 0
        warm = np.zeros(2 * 2 * N, np.float32)   # two blocks: every unit reaches the steady state
        assert g.write(warm, pos) == warm.size
        chunks.append(warm)
        pos += 2 * N
        if mode != "oracle":
            g.kernel_stats(reset=True)
        for c in range(calls):
            events(g, ids, c, pos)
            o = np.zeros(per_call * 2 * N, np.float32)
            assert g.write(o, pos) == o.size
            chunks.append(o)
            pos += per_call * N
        outs.append(np.concatenate(chunks))
        if mode != "oracle":
            _, launches, blocks = g.kernel_stats(reset=True)
            stats.append((launches, blocks))
            assert g.device_errors() == 0
    single, sup, ref = outs
    assert np.array_equal(single, sup)
    compare(sup, ref)
    assert stats[0][1] == stats[0][0]                 # one block per launch
    assert stats[1][1] > 2 * stats[1][0]              # super-block launches carried most blocks
    assert np.abs(sup[-2 * N:]).max() > 1e-3


def test_bus_pipeline_keeps_the_chain_flags_per_block_when_a_stage_runs_far_ahead(monkeypatch):
    """The pipelined bus chain (pg_bus_pipeline): `an earlier effect of the chain was active on THIS block` travels from stage to stage per block —
    the progress word holds the flags of the producer's last 24 blocks, a second word one flag per block of the launch. A Gain in front of a Reverb is
    a producer that runs far ahead (microseconds per block against the reverb's tens): in a 60-block launch sequence (PHONIC_BUS_GROUP=64) the
    reverb's workgroup finds the Gain tens of blocks ahead and must still see block c's flag, not the latest one. The flag flips in the MIDDLE of such a
    sequence, in steady state: the voices sit on a sub-mixer whose silence gate closes 2 s after they played out (submixer.rs:47-77) — from that
    block on the main mixer's input is inaudible, the Gain's processor (no tail) bypasses itself, and the reverb starts counting silence; were
    it told so tens of blocks early it would bypass itself (exact zeros instead of its denormal guard's trickle) inside the rendered span.
    Bit-identical to single-block launches, within tolerance of the oracle pulled in the same calls."""
    from phonic_amd.graph import Graph

    monkeypatch.setenv("PHONIC_BUS_GROUP", "64")     # (read when a graph is created)
    N, per_call, calls = 1024, 64, 4

    def build(g):
        m = g.add_mixer()
        for i in range(4):   # one-shots, 12-20 blocks long; non-transient: a played-out source stays, nothing rebuilds the topology inside the calls
            g.add_voice(m, workloads.tone_buffer(i, 48000, 0.25 + 0.06 * i), 2, 48000, volume=0.3, panning=workloads.voice_pan(i), non_transient=1)
        return [g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.8}), g.add_effect(0, _capi.FX_REVERB, params={"room": 0.2}, reverb_seeds=workloads.reverb_seeds(3))]

    outs = []
    for mode in ("single", "super", "oracle"):
        g = oracle.OracleGraph(SR, 2, N) if mode == "oracle" else Graph(SR, 2, N, 0)
        if mode == "super":
            g.set_max_blocks_per_launch(per_call)
        if mode != "oracle":
            g.set_timing_period(1)
        build(g)
        chunks, pos = [], 0
        for c in range(calls):
            o = np.zeros(per_call * 2 * N, np.float32)
            assert g.write(o, pos) in (0, o.size)
            chunks.append(o)
            pos += per_call * N
            if mode == "super":
                _, launches, blocks = g.bus_kernel_stats(reset=True)
                # the first call renders the voices' fades chunk by chunk; from the second on a one-chunk sequence opens the call and ONE sequence takes the other 60 blocks
                assert blocks == per_call and (c == 0 or launches <= 3), (c, launches, blocks)
        outs.append(np.concatenate(chunks))
        if mode != "oracle":
            assert g.device_errors() == 0
    single, sup, ref = outs
    assert np.array_equal(single, sup), int(np.count_nonzero(single != sup))
    compare(sup, ref)
    per_block = np.abs(ref.reshape(-1, 2 * N)).max(axis=1)
    # the block from which the chain is bypassed (exact zeros; until then the reverb's denormal guard trickles) is the oracle's, not one of tens of blocks earlier
    zero_ref = (ref.reshape(-1, 2 * N) == 0.0).all(axis=1), (sup.reshape(-1, 2 * N) == 0.0).all(axis=1)
    assert np.array_equal(zero_ref[0], zero_ref[1])
    first_zero = int(np.argmax(zero_ref[0]))
    assert per_block[3] > 1e-2 and zero_ref[0][-1] and per_call + 4 < first_zero < calls * per_call, first_zero      # (inside one of the 60-block sequences)


@pytest.mark.parametrize("bus", ["limiter", "eq5_reverb"])
def test_superblock_launch_with_a_bus_chain_is_bit_identical_to_single_blocks(bus):
    """Super-block launches for graphs whose MAIN mixer has effects (BASELINE configs 2 and 4): the mixer sum of all blocks is one launch
    (grid.y = blocks, one `audible` word per block) and ONE bus launch walks the summed blocks in order, taking the chain's per-block
    decisions — audible_input, bypass, tails (src/source/mixed.rs:627-655) — block by block, as MixedSource::write does with its chunks
    inside one call (mixed.rs:679-712). Bit-identical to the block-by-block pull: one-shot voices end inside a call, the chain rings
    out, bypasses itself and wakes up again when a late voice starts; a bus parameter event splits a call."""
    from phonic_amd.graph import Graph

    N, per_call, calls = 1024, 8, 14

    def build(g):
        for i in range(6):
            g.add_voice(0, workloads.tone_buffer(i, 44100, 0.3 + 0.05 * i), 2, 44100, volume=0.3, panning=workloads.voice_pan(i))      # one-shots, 14-26 blocks long
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_FILTER, params={"cuto": 3000.0})
        g.add_voice(m, workloads.tone_buffer(9, 48000, 0.2), 2, 48000, volume=0.4)
        g.add_voice(0, workloads.tone_buffer(20, 48000, 0.1), 2, 48000, volume=0.5, start_time=(9 * per_call + 3) * N + 5)     # late: wakes the chain up
        if bus == "limiter":
            return [g.add_effect(0, _capi.FX_COMPRESSOR, params={"thrs": -32.0, "rato": 20.0, "knee": 0.0, "gain": 0.0, "look": 0.01, "rels": 0.1})]
        return [g.add_effect(0, _capi.FX_EQ5, params={"gan2": 3.0}), g.add_effect(0, _capi.FX_REVERB, params={"room": 0.15}, reverb_seeds=workloads.reverb_seeds(5))]

    outs, stats = [], []
    for mode in ("single", "super", "oracle"):
        g = oracle.OracleGraph(SR, 2, N) if mode == "oracle" else Graph(SR, 2, N, 0)
        if mode == "super":
            g.set_max_blocks_per_launch(per_call)
        if mode != "oracle":
            g.set_timing_period(1)
        ids = build(g)
        chunks, pos = [], 0
        warm = np.zeros(2 * 2 * N, np.float32)
        assert g.write(warm, pos) == warm.size
        chunks.append(warm)
        pos += 2 * N
        if mode != "oracle":
            g.kernel_stats(reset=True)
        for c in range(calls):
            if c == 1:
                g.schedule_param(ids[0], "thrs" if bus == "limiter" else "gan4", -9.0, pos + 2 * N)      # inside the call, on a block boundary
            o = np.zeros(per_call * 2 * N, np.float32)
            assert g.write(o, pos) in (0, o.size)     # (oracle and device in the same calls: both walk them in the reference's 4096-frame chunks)
            chunks.append(o)
            pos += per_call * N
        outs.append(np.concatenate(chunks))
        if mode != "oracle":
            _, launches, blocks = g.kernel_stats(reset=True)
            stats.append((launches, blocks))
            assert g.device_errors() == 0
    single, sup, ref = outs
    assert np.array_equal(single, sup), int(np.count_nonzero(single != sup))
    compare(sup, ref)
    assert stats[0][1] == stats[0][0]                 # one block per launch
    assert stats[1][1] > 2 * stats[1][0]              # super-block launches carried most blocks
    per_block = np.abs(ref.reshape(-1, 2 * N)).max(axis=1)
    assert per_block[5] > 1e-2 and per_block[60:75].max() < 1e-5 and per_block[76] > 1e-3      # audible, rung out, woken up again by the late voice
    if bus == "limiter":
        assert (per_block[60:75] == 0.0).all()                                                    # (the limiter's known tail is over: the chain is bypassed)


def test_write_allocates_nothing_and_never_blocks_on_a_callers_stream():
    """The reference runs its audio callback under assert_no_alloc (src/output/cpal.rs:712-715). Here: all device / pinned allocations
    happen in the graph-changing calls (grow-by-doubling in add_*), the topology tables travel with asynchronous copies from pinned
    staging inside the first write after a change, command lists go through a pre-allocated ring — so the library's own HIP call
    counters (pg_debug_hip_calls) must not move across writes: no allocation, no release, and on a caller's stream no host wait and no
    blocking copy either — including the FIRST write after add_voice / add_effect and writes that carry parameter automation."""
    import gc

    import torch
    from phonic_amd.graph import Graph, hip_calls

    g = Graph(SR, 2, 1024, 0)
    ids = []
    for i in range(5):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_FILTER, params={"cuto": 3000.0})
        ids.append(g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i)))
        g.add_voice(m, workloads.tone_buffer(i, 44100, 0.2), 2, 44100, volume=0.4, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    stream = torch.cuda.Stream()
    buf = torch.zeros(8 * 2048, dtype=torch.float32, device="cuda:0")
    pos = 0

    def write(n_blocks=1):
        nonlocal pos
        assert g.write_device(buf.data_ptr(), n_blocks * 2048, pos, stream.cuda_stream) == n_blocks * 2048
        pos += n_blocks * 1024

    gc.collect()   # (the counters are process-wide: graphs of earlier tests that sit in reference cycles are released here, not by a collection inside the window)
    before = hip_calls()
    write()                                    # first write after construction: topology upload + patch kernel, all asynchronous
    for _ in range(4):
        write()
    g.schedule_param(ids[0], "room", 0.9, pos + 100)      # automation: command ring, generic kernel
    g.set_voice_volume(0, 0.2, pos + 700)
    write()
    write(4)
    assert hip_calls() == before, (before, hip_calls())
    # a graph change allocates (in add_voice, not in write) ...
    m = g.add_mixer()
    g.add_effect(m, _capi.FX_CHORUS)
    g.add_voice(m, workloads.tone_buffer(9, 48000, 0.2), 2, 48000, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
    after_change = hip_calls()
    assert after_change["alloc"] > before["alloc"]
    # ... and the first write after it again moves no counter
    write()
    write()
    assert hip_calls() == after_change
    stream.synchronize()
    assert g.device_errors() == 0
    host = buf.cpu().numpy()
    assert np.isfinite(host).all() and np.abs(host[:2048]).max() > 1e-3
    # the host-buffer variant waits for its result (one stream wait per call) but allocates nothing
    out = np.zeros(2048, np.float32)
    c0 = hip_calls()
    assert g.write(out, pos) == 2048
    c1 = hip_calls()
    assert c1["alloc"] == c0["alloc"] and c1["free"] == c0["free"] and c1["blocking_copy"] == c0["blocking_copy"]


def test_control_calls_from_another_thread_while_rendering():
    """EffectHandle::set_parameter / FilePlaybackHandle::set_volume ... push into the mixer's lock-free message queue from any thread
    while the audio thread renders (src/player/handles/effect.rs:67-95, src/source/mixed.rs:113-194,294-499). Same contract here: a
    producer thread schedules 100 000 sample-time-tagged events (parameter changes on 8 per-voice Gain / Filter effects, voice volume
    and panning moves) while this thread pulls blocks; the producer only has to stay ahead of the render position (a watermark the
    render loop waits for), so every event takes effect at its sample time and the result must equal the oracle fed the same events
    from one thread. Also: a full queue reports PG_ERR_QUEUE_FULL and loses nothing that was accepted."""
    import threading

    import phonic_amd
    from phonic_amd.graph import Graph

    N, blocks, n_units, n_events = 1024, 100, 8, 100_000
    rng = np.random.default_rng(7)
    times = np.sort(rng.integers(N, blocks * N, n_events)).astype(np.uint64)
    kinds = rng.integers(0, 4, n_events)
    units = rng.integers(0, n_units, n_events)
    vals = rng.random(n_events).astype(np.float32)

    def build(g):
        ids = []
        for i in range(n_units):
            m = g.add_mixer()
            ga = g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.8})
            fi = g.add_effect(m, _capi.FX_FILTER, params={"cuto": 4000.0})
            v = g.add_voice(m, workloads.tone_buffer(i, 44100, 0.2), 2, 44100, volume=0.3, panning=workloads.voice_pan(i), has_repeat=1,
                            repeat=_capi.PG_REPEAT_FOREVER)
            ids.append((ga, fi, v))
        return ids

    def send(g, ids, k):
        ga, fi, v = ids[units[k]]
        t = int(times[k])
        if kinds[k] == 0:
            g.schedule_param(ga, "gain", 0.2 + 0.6 * float(vals[k]), t)
        elif kinds[k] == 1:
            g.schedule_param(fi, "cuto", float(vals[k]), t, normalized=True)
        elif kinds[k] == 2:
            g.set_voice_volume(v, 0.1 + 0.4 * float(vals[k]), t)
        else:
            g.set_voice_panning(v, 2.0 * float(vals[k]) - 1.0, t)

    # oracle: one thread, every block's events sent right before the block
    gc = oracle.OracleGraph(SR, 2, N)
    ids_c = build(gc)
    ref = np.zeros((blocks, 2 * N), np.float32)
    k = 0
    for b in range(blocks):
        while k < n_events and times[k] < (b + 1) * N:
            send(gc, ids_c, k)
            k += 1
        assert gc.write(ref[b], b * N) == 2 * N
    # GPU: producer thread runs ahead of the render loop
    g = Graph(SR, 2, N, 0)
    ids_g = build(g)
    sent_until = [0]          # every event with sample time < sent_until[0] has been pushed
    cond = threading.Condition()
    errors = []

    def producer():
        try:
            k = 0
            for b in range(blocks):
                while k < n_events and times[k] < (b + 1) * N:
                    while True:
                        try:
                            send(g, ids_g, k)
                            break
                        except phonic_amd.PhonicError as e:   # queue full: the renderer has to drain first
                            if e.code != _capi.PG_ERR_QUEUE_FULL:
                                raise
                    k += 1
                with cond:
                    sent_until[0] = (b + 1) * N
                    cond.notify_all()
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            with cond:
                sent_until[0] = blocks * N
                cond.notify_all()

    th = threading.Thread(target=producer)
    out = np.zeros((blocks, 2 * N), np.float32)
    th.start()
    for b in range(blocks):
        with cond:
            cond.wait_for(lambda: sent_until[0] >= (b + 1) * N, timeout=120)
        assert g.write(out[b], b * N) == 2 * N
    th.join(timeout=120)
    assert not errors, errors
    assert g.device_errors() == 0
    compare(out.reshape(-1), ref.reshape(-1))
    assert np.abs(out).max() > 1e-3
    # queue capacity: 65536 records; the 65537th push without a write in between is refused, the next write takes all accepted ones
    accepted = 0
    with pytest.raises(phonic_amd.PhonicError) as ei:
        for _ in range(70000):
            g.set_voice_volume(ids_g[0][2], 0.3, blocks * N + 10)
            accepted += 1
    assert ei.value.code == _capi.PG_ERR_QUEUE_FULL and accepted == 65536
    tail = np.zeros(2 * N, np.float32)
    assert g.write(tail, blocks * N) == 2 * N                 # 65536 commands on one sample of one unit: still rendered
    g.set_voice_volume(ids_g[0][2], 0.3, blocks * N + 2000)   # accepted again after the drain
    for k in range(70000):                                     # more than the command ring holds in one round: the degenerate path
        if k == 65000:
            assert g.write(tail, (blocks + 1) * N) == 2 * N
        g.set_voice_panning(ids_g[1][2], 0.1, (blocks + 2) * N + 5)
    assert g.write(tail, (blocks + 2) * N) == 2 * N and np.isfinite(tail).all()


@pytest.mark.parametrize("n_shards", [1, 3])
def test_sharded_graph_object_matches_the_single_graph(n_shards):
    """pg_sharded_*: ONE handle that owns a graph per device and renders the main mixer as n partial buses + a sum on the root + the
    bus chain (the C-ABI form of the multi-GPU path; with 1-GPU boxes every shard sits on device 0). The handle takes every call the
    plain graph takes (the reference's MixerMessage set, src/source/mixed.rs:124-145,163-178,422-462): per-voice chains on sub-mixers
    (placed on the least loaded shard), plain main-mixer sources, a nested sub-mixer (must land on its parent's shard), a bus chain with
    a limiter (non-linear: the sum must happen before it), parameter events on a sub-mixer effect, on a bus effect and on voices, a stop,
    set_speed with a glide, seek, move_effect on a sub-mixer chain and on the bus chain, remove_effect, remove_mixer (with the ids under
    it). Main-mixer events of one shard must cut the chunks of ALL shards (the per-call logic of the other shards' sub-mixers sees the
    same calls as in the one mixer). Checked against the oracle and against the unsharded graph (f32 order of the voice sum differs)."""
    from phonic_amd.graph import Graph, ShardedGraph
    import phonic_amd

    N, blocks = 1024, 14

    def build(g):
        ids = {"fx": [], "rv": [], "v": [], "m": []}
        for i in range(7):
            m = g.add_mixer()
            ids["m"].append(m)
            ids["fx"].append(g.add_effect(m, _capi.FX_FILTER, params={"cuto": 1500.0 + 300 * i}))
            ids["rv"].append(g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i)))
            ids["v"].append(g.add_voice(m, workloads.tone_buffer(i, 44100, 0.2), 2, 44100, volume=0.3, panning=workloads.voice_pan(i), has_repeat=1,
                                        repeat=_capi.PG_REPEAT_FOREVER))
            if i == 2:
                child = g.add_mixer(m)
                g.add_effect(child, _capi.FX_CHORUS)
                g.add_voice(child, workloads.tone_buffer(30, 48000, 0.2), 2, 48000, volume=0.2, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
                ids["nested"] = (m, child)
        for i in range(4):
            ids["v"].append(g.add_voice(0, workloads.tone_buffer(10 + i, 48000, 0.2), 2, 48000, volume=0.2, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER))
        ids["eq"] = g.add_effect(0, _capi.FX_EQ5, params={"gan2": 4.0})
        ids["lim"] = g.add_effect(0, _capi.FX_COMPRESSOR, params={"thrs": -20.0, "rato": 20.0, "knee": 0.0, "gain": 0.0, "look": 0.02})
        return ids

    def automate(g, ids, b, pos):
        if b == 3:
            g.schedule_param(ids["fx"][1], "cuto", 500.0, pos + 300)
            g.schedule_param(ids["eq"], "gan4", -9.0, pos + 600)
            g.set_voice_volume(ids["v"][8], 0.05, pos + 100)      # a main-mixer source: its event cuts every shard's chunk
            g.set_voice_panning(ids["v"][0], 0.9, pos + 900)
        if b == 5:
            g.set_voice_speed(ids["v"][1], 1.5, pos + 128, glide=24.0)
            g.set_voice_speed(ids["v"][7], 0.75, pos + 700)          # a main-mixer source, immediate
            g.seek_voice(ids["v"][3], 0.05, pos + 512)
        if b == 6:
            g.stop_voice(ids["v"][9], pos + 200)
        if b == 7:
            g.move_effect(ids["rv"][4], ids["m"][4], _capi.MOVE_START)       # Reverb in front of the Filter
            g.move_effect(ids["lim"], 0, _capi.MOVE_DIRECTION, -1)           # the bus chain: limiter in front of the Eq5
        if b == 9:
            g.remove_effect(ids["fx"][5])
            g.remove_mixer(ids["nested"][0])                                  # with its nested sub-mixer
        if b == 11:
            g.remove_effect(ids["eq"])

    outs = []
    for mode in ("sharded", "single", "oracle"):
        g = ShardedGraph([0] * n_shards, SR, 2, N) if mode == "sharded" else (Graph(SR, 2, N, 0) if mode == "single" else oracle.OracleGraph(SR, 2, N))
        ids = build(g)
        if mode == "sharded":
            assert g.shard_count() == n_shards
            assert g.shard_of_mixer(ids["nested"][0]) == g.shard_of_mixer(ids["nested"][1])
            if n_shards == 3:
                assert len({g.shard_of_mixer(m) for m in range(1, 5)}) == 3     # placement spreads the sub-mixers
        o = np.zeros((blocks, 2 * N), np.float32)
        for b in range(blocks):
            automate(g, ids, b, b * N)
            assert g.write(o[b], b * N) == 2 * N
        outs.append(o.reshape(-1))
        if mode == "sharded":
            assert g.device_errors() == 0
            assert g.is_voice_playing(ids["v"][0]) and not g.is_voice_playing(ids["v"][9])
            for call in (lambda: g.schedule_param(9999, "cuto", 100.0, 0), lambda: g.remove_mixer(ids["nested"][0]), lambda: g.remove_mixer(ids["nested"][1]),
                         lambda: g.remove_effect(ids["fx"][5]), lambda: g.add_effect(ids["nested"][1], _capi.FX_GAIN), lambda: g.set_voice_speed(9999, 1.0, 0),
                         lambda: g.seek_voice(9999, 0.0, 0)):
                with pytest.raises(phonic_amd.PhonicError) as ei:
                    call()
                assert ei.value.code == _capi.PG_ERR_NOT_FOUND
            with pytest.raises(phonic_amd.PhonicError) as ei:
                g.remove_mixer(0)
            assert ei.value.code == _capi.PG_ERR_PARAMETER
            with pytest.raises(phonic_amd.PhonicError) as ei:      # an effect of another mixer
                g.move_effect(ids["rv"][0], ids["m"][1], _capi.MOVE_END)
            assert ei.value.code == _capi.PG_ERR_PARAMETER
    compare(outs[0], outs[2])
    compare(outs[1], outs[2])
    assert float(np.abs(outs[0] - outs[1]).max()) <= 2e-5
    assert np.abs(outs[0]).max() > 1e-2


@pytest.mark.parametrize("n_shards", [1, 3])
def test_sharded_superblock_write_takes_the_bus_decisions_per_block(n_shards):
    """A sharded write that spans several blocks (pg_sharded_set_max_blocks_per_launch): the bus chain behind the sum must see ONE
    `audible_input` per block (process_effects, src/source/mixed.rs:627-655,696-706), OR-ed over the shards — not one word for the whole
    call. One-shot voices end in the second block of a four-block call; the bus chain (Gain -> Delay with a known tail) must run over
    the audible blocks, count its tail down from the first silent one and bypass itself when the tail is over, exactly as the oracle
    rendering the same calls. An empty shard must contribute silence and a clear flag, not what an earlier call left in its buffers."""
    from phonic_amd.graph import ShardedGraph

    N, per_call, calls = 1024, 4, 15

    def build(g):
        ids = []
        for i in range(4):   # main-mixer one-shots, spread over the shards: ~1.4 blocks long, starting in call 2 (a source's `audible` ends with it; a
            ids.append(g.add_voice(0, workloads.tone_buffer(i, 48000, 0.03), 2, 48000, volume=0.5, start_time=2 * per_call * N))   # sub-mixer's only 2 s later)
        g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.8})
        g.add_effect(0, _capi.FX_DELAY, params={"dlay": 30.0, "fdbk": 0.3, "wet_": 0.6})
        return ids

    outs = []
    for mode in ("sharded", "oracle"):
        g = ShardedGraph([0] * n_shards, SR, 2, N) if mode == "sharded" else oracle.OracleGraph(SR, 2, N)
        if mode == "sharded":
            g.set_max_blocks_per_launch(per_call)
        build(g)
        o = np.zeros((calls, per_call * 2 * N), np.float32)
        for c in range(calls):   # (oracle and device in the same calls: both walk them in the reference's 4096-frame chunks)
            assert g.write(o[c], c * per_call * N) == o[c].size
        outs.append(o.reshape(-1))
        if mode == "sharded":
            assert g.device_errors() == 0
    compare(outs[0], outs[1])
    audible = outs[1].reshape(calls * per_call, -1)
    assert np.abs(audible[2 * per_call + 1]).max() > 1e-2          # the voices play in blocks 8-9 ...
    assert np.abs(audible[2 * per_call + 3]).max() > 1e-4          # ... the delay's repeats ring on in the silent blocks of the same call
    assert np.abs(audible[-1]).max() == 0.0                        # ... and the chain has bypassed itself at the end


@pytest.mark.parametrize("mf", [1024, 256])
def test_sharded_host_write_longer_than_its_staging_is_one_call_on_the_chunk_grid(mf):
    """pg_sharded_write with a host buffer of MORE than max_blocks x max_frames frames (round-4 advisor finding): it used to be cut into separate
    write calls of max_blocks x max_frames frames, each with its own process_messages, call end and chunk grid — per-chunk decisions (bypass and
    tail counters, the chorus' per-call phase bookkeeping under a rate ramp, Eq5's per-call ramp branch, one-shots that end inside the call) then
    differed from the single graph and the reference for the same call. Calls of 5000 and 9000 frames (max_blocks = 1: the staging holds one
    chunk), events anywhere inside them; against the single graph (same calls) and the oracle (same calls)."""
    from phonic_amd.graph import Graph, ShardedGraph

    calls = [5000, 9000, 4096, 700, 8192, 6000]

    def build(g):
        ids = {}
        for i in range(5):
            m = g.add_mixer()
            if i == 0:
                ids["ch"] = g.add_effect(m, _capi.FX_CHORUS, params={"rate": 2.0})
            elif i == 1:
                ids["eq"] = g.add_effect(m, _capi.FX_EQ5, params={"gan2": 3.0})
            else:
                g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.2), 2, 44100, volume=0.3, panning=workloads.voice_pan(i), has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        for i in range(3):   # one-shots on the main mixer: they end inside the second call, the bus Delay rings on and bypasses itself later
            ids.setdefault("v", []).append(g.add_voice(0, workloads.tone_buffer(10 + i, 48000, 0.05), 2, 48000, volume=0.4, start_time=5000 + 100 * i))
        g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.8})
        ids["dl"] = g.add_effect(0, _capi.FX_DELAY, params={"dlay": 30.0, "fdbk": 0.3, "wet_": 0.6})
        return ids

    def automate(g, ids, c, pos):
        if c == 0:
            g.schedule_param(ids["ch"], "rate", 6.0, pos + 1500)     # a rate ramp across a piece and a chunk boundary
            g.schedule_param(ids["eq"], "gan4", -6.0, pos + 4000)    # a gain ramp that starts just in front of the first chunk's end
        if c == 1:
            g.set_voice_volume(ids["v"][1], 0.1, pos + 4500)         # a main-mixer source: cuts every shard's chunk, restarts the grid
            g.schedule_param(ids["dl"], "fdbk", 0.5, pos + 6000)     # a bus event
        if c == 4:
            g.schedule_param(ids["ch"], "rate", 0.5, pos + 8000)

    outs = []
    for mode in ("sharded", "single", "oracle"):
        g = ShardedGraph([0, 0, 0], SR, 2, mf) if mode == "sharded" else (Graph(SR, 2, mf, 0) if mode == "single" else oracle.OracleGraph(SR, 2, mf))
        ids = build(g)
        chunks, pos = [], 0
        for c, n in enumerate(calls):
            automate(g, ids, c, pos)
            o = np.zeros(2 * n, np.float32)
            assert g.write(o, pos) == 2 * n
            chunks.append(o)
            pos += n
        outs.append(np.concatenate(chunks))
        if mode == "sharded":
            assert g.device_errors() == 0
    compare(outs[0], outs[2])
    compare(outs[1], outs[2])
    assert float(np.abs(outs[0] - outs[1]).max()) <= 2e-5
    assert np.abs(outs[0]).max() > 1e-2


def test_sharded_write_returns_zero_when_the_main_mixer_has_nothing_left():
    """MixedSource::write returns 0 without touching the buffer when there is no playing source, no effect, no sub-mixer and no event
    (src/source/mixed.rs:664-670); exhausted transient sources are dropped after the write they ended in (:715). The sharded handle
    must do the same as the plain graph, call for call: main-mixer one-shot sources spread over three shards, then a sub-mixer that is
    removed again."""
    from phonic_amd.graph import Graph, ShardedGraph

    N = 512
    rets = []
    for mode in ("sharded", "single", "oracle"):
        g = ShardedGraph([0, 0, 0], SR, 2, N) if mode == "sharded" else (Graph(SR, 2, N, 0) if mode == "single" else oracle.OracleGraph(SR, 2, N))
        r, pos = [], 0
        buf = np.full(2 * N, 7.0, np.float32)
        r.append(g.write(buf, pos)); assert buf[0] == 7.0      # empty graph: 0, buffer untouched
        for i in range(4):
            g.add_voice(0, workloads.tone_buffer(i, 48000, 0.01 + 0.004 * i), 2, 48000, volume=0.4, fade_out_seconds=-1.0)
        for b in range(6):
            buf[:] = 7.0
            r.append(g.write(buf, pos)); pos += N
        assert buf[0] == 7.0                                    # the last call found nothing to do
        m = g.add_mixer()
        r.append(g.write(buf, pos)); pos += N                  # a sub-mixer: the main mixer is not empty
        g.remove_mixer(m)
        buf[:] = 7.0
        r.append(g.write(buf, pos)); pos += N
        assert buf[0] == 7.0
        rets.append(r)
    assert rets[0] == rets[1] == rets[2], rets
    assert rets[2][0] == 0 and rets[2][1] == 2 * N and rets[2][6] == 0 and rets[2][7] == 2 * N and rets[2][8] == 0


def test_sharded_asynchronous_writes_back_to_back():
    """pg_sharded_write_device is asynchronous: several calls may be enqueued before one pg_sharded_synchronize. The peers' copies of
    call k + 1 into the root's gather buffers must wait for the root's sum of call k (round-2 advisor finding: a write-after-read race
    on d_gather / d_flags). 40 calls in flight on three shards against the same render taken one synchronous call at a time."""
    import torch
    from phonic_amd.graph import ShardedGraph

    N, per_call, calls = 1024, 2, 40

    def build(g):
        for i in range(9):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.1), 2, 44100, volume=0.3, panning=workloads.voice_pan(i), has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        g.add_effect(0, _capi.FX_COMPRESSOR, params={"thrs": -24.0, "rato": 20.0, "knee": 0.0, "gain": 0.0})

    a = ShardedGraph([0, 0, 0], SR, 2, N); a.set_max_blocks_per_launch(per_call); build(a)
    b = ShardedGraph([0, 0, 0], SR, 2, N); b.set_max_blocks_per_launch(per_call); build(b)
    d = torch.zeros((calls, per_call * 2 * N), dtype=torch.float32, device="cuda:0")
    for c in range(calls):
        assert a.write_device(d[c].data_ptr(), per_call * 2 * N, c * per_call * N) == per_call * 2 * N
    a.synchronize()
    ref = np.zeros((calls, per_call * 2 * N), np.float32)
    for c in range(calls):
        assert b.write(ref[c], c * per_call * N) == per_call * 2 * N
    assert a.device_errors() == 0 and b.device_errors() == 0
    assert np.array_equal(d.cpu().numpy(), ref)
    assert np.abs(ref).max() > 1e-2


def test_sharded_rccl_reduce_on_a_one_device_communicator():
    """PG_REDUCE_RCCL: the partial buses meet by ncclReduce(sum) (and the `audible` words by ncclReduce(max)) on the shards' streams
    instead of peer copies + the sum kernel. A 1-GPU box can only hold a one-rank communicator (ncclCommInitAll over one device), which
    still runs every RCCL call of the path; two shards on ONE device must be refused with RCCL / parameter error text, leaving the mode as
    it was — no silent fallback."""
    from phonic_amd.graph import ShardedGraph
    import phonic_amd

    N, blocks = 1024, 8

    def build(g):
        for i in range(5):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.1), 2, 44100, volume=0.3, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        eq = g.add_effect(0, _capi.FX_EQ5, params={"gan3": 5.0})
        g.add_effect(0, _capi.FX_COMPRESSOR, params={"thrs": -20.0, "rato": 20.0, "knee": 0.0, "gain": 0.0})
        return eq

    outs = []
    for mode in ("rccl", "oracle"):
        g = ShardedGraph([0], SR, 2, N) if mode == "rccl" else oracle.OracleGraph(SR, 2, N)
        if mode == "rccl":
            g.set_max_blocks_per_launch(2)
            g.set_reduce(_capi.REDUCE_RCCL)
            assert g.reduce_mode() == _capi.REDUCE_RCCL
        eq = build(g)
        o = np.zeros((blocks // 2, 2 * 2 * N), np.float32)
        for c in range(blocks // 2):
            if c == 2:
                g.schedule_param(eq, "gan1", -6.0, (c * 2 + 1) * N)     # a bus event inside a call (on its second block): the call is rendered as two segments
            if mode == "rccl":
                assert g.write(o[c], c * 2 * N) == o[c].size
            else:
                for k in range(2):
                    assert g.write(o[c][k * 2 * N:(k + 1) * 2 * N], (c * 2 + k) * N) == 2 * N
        outs.append(o.reshape(-1))
        if mode == "rccl":
            assert g.device_errors() == 0
    compare(outs[0], outs[1])
    assert np.abs(outs[0]).max() > 1e-2
    g2 = ShardedGraph([0, 0], SR, 2, N)
    with pytest.raises(phonic_amd.PhonicError) as ei:
        g2.set_reduce(_capi.REDUCE_RCCL)
    assert "device 0 is listed twice" in str(ei.value)
    assert g2.reduce_mode() == _capi.REDUCE_PEER_COPY


@pytest.mark.parametrize("file_rate,source_rate,channels", [(44100, 32000, 2), (48000, 96000, 2), (22050, 22050, 1), (44100, 44100, 2)])
def test_resampled_source_behind_the_file_source(file_rate, source_rate, channels):
    """ResampledSource::write + TempBuffer (src/source/resampled.rs:101-152, src/utils/buffer.rs:499-610). A file source
    created with an output rate other than the mixer's (pg_voice_options::source_rate) gets ConvertedSource's cubic ResampledSource
    behind it (converted.rs:15-45): 512-frame input and output staging, ranges carried across write calls, (consumed, produced) of the
    last channel, the ratio < 1 and >= 1 branches (96 kHz -> 48 kHz), mono sources mapped AFTER the resampler. Ragged block sizes move
    the staging ranges through every alignment; a looping voice on the main mixer is compared bit for bit, a one-shot voice into a
    sub-mixer with a Filter (the reference keeps resampling the stale tail of its input buffer once the source has ended) within tolerance."""
    sizes = [1, 7, 511, 512, 513, 1024, 100, 1023, 2, 640, 1024, 333] * 2

    def render(g):
        g.add_voice(0, workloads.tone_buffer(3, file_rate, 0.11, channels=channels), channels, file_rate, volume=1.0, panning=0.0, has_repeat=1,
                    repeat=_capi.PG_REPEAT_FOREVER, source_rate=source_rate)
        chunks, pos = [], 0
        for n in sizes:
            o = np.zeros(2 * n, np.float32)
            assert g.write(o, pos) == 2 * n
            chunks.append(o)
            pos += n
        return np.concatenate(chunks)

    gg, gc = graphs(1024)
    a, b = render(gg), render(gc)
    assert np.array_equal(a, b)
    assert np.abs(a).max() > 1e-2

    def render2(g):
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_FILTER, params={"cuto": 3000.0})
        g.add_voice(m, workloads.tone_buffer(5, file_rate, 0.09, channels=channels), channels, file_rate, volume=0.7, panning=-0.3, source_rate=source_rate,
                    fade_in_seconds=0.01, speed=1.25)
        g.add_voice(m, workloads.tone_buffer(6, 48000, 0.3), 2, 48000, volume=0.2, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        chunks, pos = [], 0
        for n in sizes:
            o = np.zeros(2 * n, np.float32)
            assert g.write(o, pos) == 2 * n
            chunks.append(o)
            pos += n
        return np.concatenate(chunks)

    gg, gc = graphs(1024)
    a, b = render2(gg), render2(gc)
    compare(a, b, 1e-6, 1e-5)
    assert gg.device_errors() == 0


def test_eq5_compressor_delay_and_chorus_ramps_stay_on_the_time_parallel_kernels():
    """While a smoother moves, FilterEffect (round 1), Eq5Effect and the Compressor's makeup gain (round 2) keep a time-parallel path: the
    smoothers' f32 value sequences are laid out by single lanes, the per-frame coefficients / gains are computed by all lanes, the
    recurrence runs as the time-varying blocked scan. A sub-mixer Eq5 -> Compressor gets gain / frequency / bandwidth / makeup updates;
    only the block that carries the commands goes to the generic kernel, the ramping blocks behind it are rendered by the fast kernel
    (pg_graph_deferred_units() == 0) and match the oracle."""
    from phonic_amd.graph import Graph

    def build(g):
        ids = []
        for i in range(3):
            m = g.add_mixer()
            eq = g.add_effect(m, _capi.FX_EQ5, params={"gan2": 3.0})
            cp = g.add_effect(m, _capi.FX_COMPRESSOR, params={"thrs": -24.0, "rato": 4.0, "gain": 3.0})
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.3), 2, 44100, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
            ids.append((eq, cp))
        m = g.add_mixer()   # DelayEffect: delay time (spring smoother), feedback, wet, filter cutoff and the LFO rate ramp together
        dl = g.add_effect(m, _capi.FX_DELAY, params={"dlay": 25.0, "fdbk": 0.6, "lfdt": 0.05, "lfdf": 0.3, "lfor": 3.0})
        g.add_voice(m, workloads.tone_buffer(7, 48000, 0.3), 2, 48000, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        ids.append((dl, dl))
        m = g.add_mixer()   # ChorusEffect: rate + phase (update_lfos per frame), delay (spring), depth, pre-filter frequency ramp together
        ch = g.add_effect(m, _capi.FX_CHORUS, params={"rate": 2.0, "dlay": 15.0, "fltf": 8000.0})
        g.add_voice(m, workloads.tone_buffer(9, 48000, 0.3), 2, 48000, volume=0.6, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        ids.append((ch, ch))
        return ids

    def act(g, ids, pos):
        g.schedule_param(ids[4][0], "rate", 6.0, pos + 20)
        g.schedule_param(ids[4][0], "phas", 0.4, pos + 20)
        g.schedule_param(ids[4][0], "dlay", 40.0, pos + 500)
        g.schedule_param(ids[4][0], "dpth", 0.7, pos + 500)
        g.schedule_param(ids[4][0], "fltf", 1200.0, pos + 800)
        g.schedule_param(ids[3][0], "dlay", 60.0, pos + 50)
        g.schedule_param(ids[3][0], "fdbk", 0.2, pos + 50)
        g.schedule_param(ids[3][0], "wet_", 0.9, pos + 400)
        g.schedule_param(ids[3][0], "cuto", 900.0, pos + 400)
        g.schedule_param(ids[3][0], "lfor", 7.0, pos + 900)
        g.schedule_param(ids[0][0], "gan2", -9.0, pos + 100)
        g.schedule_param(ids[0][0], "frq3", 900.0, pos + 100)
        g.schedule_param(ids[1][0], "bw_2", 0.5, pos + 700)
        g.schedule_param(ids[2][1], "gain", -12.0, pos + 300)

    gg, gc = Graph(SR, 2, 1024, 0), oracle.OracleGraph(SR, 2, 1024)
    outs, deferred = [], []
    for g in (gg, gc):
        ids = build(g)
        o = np.zeros((12, 2048), np.float32)
        for b in range(12):
            if b == 3:
                act(g, ids, b * 1024)
            assert g.write(o[b], b * 1024) == 2048
            if g is gg:
                deferred.append(g.deferred_units())
        outs.append(o.reshape(-1))
    compare(outs[0], outs[1])
    assert deferred[3] == 5          # the block with the commands: exact generic kernel
    assert deferred[4] == 0 and deferred[5] == 0, deferred   # still ramping (Eq5 gain: ~0.1 s; the delay time's spring: ~0.4 s), yet on the fast kernel
    assert gg.device_errors() == 0


def test_every_pair_of_effect_kinds_keeps_the_routing_and_the_kernels_consistent():
    """The fast kernels carry no serial effect code: which variant renders a unit (lean / wide / mid / staged lean / staged wide) is decided on
    the host from the effect kinds of its chain, and whether a unit may stay there from the eligibility the generic kernel computed a block
    earlier. Every ordered pair of the ten stock effects as a two-effect sub-mixer chain (100 units), rendered for 8 blocks with a parameter
    command in the middle: no kernel may meet an effect state its time-parallel path declines (pg_graph_device_errors() == 0 — round-1
    advisor finding), and everything matches the oracle."""
    from phonic_amd.graph import Graph

    some_param = {0: ("gain", 0.5), 1: ("pan ", 0.4), 2: ("cuto", 900.0), 3: ("gan3", 6.0), 4: ("fdbk", 0.3), 5: ("wet ", 0.6), 6: ("dpth", 0.6), 7: ("gain", -3.0),
                  8: ("thrs", -40.0), 9: ("driv", 1.5)}

    def build(g):
        ids = []
        n = 0
        for a in range(10):
            for b in range(10):
                m = g.add_mixer()
                fa = g.add_effect(m, a, reverb_seeds=workloads.reverb_seeds(n) if a == _capi.FX_REVERB else None)
                fb = g.add_effect(m, b, reverb_seeds=workloads.reverb_seeds(n + 500) if b == _capi.FX_REVERB else None)
                g.add_voice(m, workloads.tone_buffer(n % 50, 44100, 0.15), 2, 44100, volume=0.08, panning=workloads.voice_pan(n), has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
                ids.append((fa, a, fb, b))
                n += 1
        return ids

    outs = []
    for g in (Graph(SR, 2, 1024, 0), oracle.OracleGraph(SR, 2, 1024)):
        ids = build(g)
        o = np.zeros((8, 2048), np.float32)
        for blk in range(8):
            if blk == 3:
                for k, (fa, a, fb, b) in enumerate(ids):
                    if k % 3 == 0:
                        g.schedule_param(fa, some_param[a][0], some_param[a][1], blk * 1024 + 100 + k)
                    elif k % 3 == 1:
                        g.schedule_param(fb, some_param[b][0], some_param[b][1], blk * 1024 + 900 - k)
            assert g.write(o[blk], blk * 1024) == 2048
        outs.append(o.reshape(-1))
        if isinstance(g, Graph):
            assert g.device_errors() == 0
    compare(outs[0], outs[1])
    assert np.abs(outs[0]).max() > 1e-2


def test_multi_gpu_sized_run_stays_audible_past_the_silence_gate():
    """A shard of an 8192-voice job (the 8 x 1024 weak-scaling run): with the plain 1 / sqrt(V) voice level every per-voice sub-mixer would sit
    below SILENCE_THRESHOLD = 0.001 and be dropped from the sum after 2 s (submixer.rs:47-77) — the bench would measure silence. The workloads
    hold the level at 1 / 32 from 1024 voices on: block 110 (2.3 s) of such a shard is as loud as block 10 (round-1 advisor finding)."""
    from phonic_amd.graph import Graph

    g = Graph(SR, 2, 1024, 0)
    g.set_max_blocks_per_launch(10)
    workloads.build_headline(g, 32, 4096, 8192, seconds=0.5)
    peaks = []
    for c in range(11):
        o = np.zeros(10 * 2048, np.float32)
        assert g.write(o, c * 10240) == o.size
        peaks.append(float(np.abs(o[-2048:]).max()))
    assert peaks[0] > 1e-3 and peaks[-1] > 0.5 * peaks[0], peaks
    assert g.device_errors() == 0


def test_reverb_wet_ramp_stays_on_the_time_parallel_kernels():
    """ReverbEffect while `wet` moves (its exponential smoother needs 2-3 blocks): the ring geometry stands still, the wet gain, the dry share and
    the three low-pass cutoffs move per frame — reverb_wet_ramp_fast lays the smoother's sequence out on one lane and runs the biquads as
    time-varying blocked scans. Two sub-mixers Eq5 -> Reverb -> Gain (fused wide kernel: it carries the ramp paths) and one plain Reverb
    sub-mixer (staged kernel: no ramp paths, the generic kernel takes the unit while it ramps — with the same time-parallel path). Only the
    block with the commands is rendered serially; a room-size change (ring lengths change per frame) keeps its unit on the serial lane for the
    frames of its linear ramp (next test)."""
    from phonic_amd.graph import Graph

    def build(g):
        ids = []
        for i in range(2):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_EQ5, params={"gan3": 2.0})
            rv = g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(40 + i))
            g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.8})
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.3), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
            ids.append(rv)
        m = g.add_mixer()
        ids.append(g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(50)))
        g.add_voice(m, workloads.tone_buffer(5, 48000, 0.3), 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return ids

    gg, gc = Graph(SR, 2, 1024, 0), oracle.OracleGraph(SR, 2, 1024)
    outs, deferred = [], []
    for g in (gg, gc):
        ids = build(g)
        o = np.zeros((14, 2048), np.float32)
        for b in range(14):
            if b == 3:
                g.schedule_param(ids[0], "wet ", 0.9, b * 1024 + 100)
                g.schedule_param(ids[1], "wet ", 0.05, b * 1024 + 700)
                g.schedule_param(ids[2], "wet ", 0.8, b * 1024 + 300)
            if b == 9:
                g.schedule_param(ids[0], "room", 0.3, b * 1024 + 50)   # shrinking rooms: ring positions may sit above the new ring end
                g.schedule_param(ids[2], "room", 0.2, b * 1024 + 50)
            assert g.write(o[b], b * 1024) == 2048
            if g is gg:
                deferred.append(g.deferred_units())
        outs.append(o.reshape(-1))
    compare(outs[0], outs[1])
    assert deferred[3] == 3                      # the block with the commands
    assert deferred[4] == 1 and deferred[5] <= 1, deferred   # wet still ramping: only the staged unit is with the generic kernel
    assert deferred[8] == 0 and deferred[9] == 2 and deferred[13] == 0, deferred
    assert gg.device_errors() == 0


def test_reverb_wet_ramp_in_a_graph_of_lean_kernels():
    """The same ramp in a graph that holds nothing but Gain / Panning / Reverb: its fused fast kernel (`pg_unit_kernel_fast`, lean) carries no
    ramp paths, so a ramping unit must stay with the generic kernel (which takes the time-parallel ramp path itself) until the smoother rests —
    no kernel may meet a state it declines (pg_graph_device_errors() == 0), and the output matches the oracle."""
    from phonic_amd.graph import Graph

    def build(g):
        ids = []
        m = g.add_mixer()
        ids.append(g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(70)))
        g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.7})     # reverb not last: a fused (lean) unit, not a staged one
        g.add_voice(m, workloads.tone_buffer(2, 44100, 0.3), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m = g.add_mixer()
        ids.append(g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(71)))
        g.add_voice(m, workloads.tone_buffer(3, 48000, 0.3), 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return ids

    gg, gc = Graph(SR, 2, 1024, 0), oracle.OracleGraph(SR, 2, 1024)
    outs, deferred = [], []
    for g in (gg, gc):
        ids = build(g)
        o = np.zeros((10, 2048), np.float32)
        for b in range(10):
            if b == 3:
                g.schedule_param(ids[0], "wet ", 0.85, b * 1024 + 200)
                g.schedule_param(ids[1], "wet ", 0.1, b * 1024 + 600)
            assert g.write(o[b], b * 1024) == 2048
            if g is gg:
                deferred.append(g.deferred_units())
        outs.append(o.reshape(-1))
    compare(outs[0], outs[1])
    assert gg.dominant_kernel().startswith("pg_stage_fused_kernel") or "pg_unit_kernel_fast" in gg.dominant_kernel()
    assert deferred[3] == 2 and deferred[4] == 2 and deferred[9] == 0, deferred   # both units wait out the ramp on the generic kernel
    assert gg.device_errors() == 0


def test_gain_panning_and_distortion_ramps_stay_on_the_time_parallel_kernels():
    """The memoryless effects while their smoothers move — and the Distortion at a steady partial mix, whose reference loop steps both smoothers per
    frame: single lanes lay the smoothers' value sequences out, all lanes apply them. Sub-mixers Gain -> Filter, Panning -> Filter and
    Distortion (mix 0.5) -> Filter (a graph of wide kernels): only the block with the commands goes to the generic kernel."""
    from phonic_amd.graph import Graph

    def build(g):
        ids = {}
        for name, kind, params in (("gain", _capi.FX_GAIN, {"gain": 0.8}), ("pan", _capi.FX_PANNING, {"pan ": -0.2, "wdth": 1.2}),
                                   ("dist", _capi.FX_DISTORTION, {"driv": 1.0, "mix ": 0.5}), ("dcgain", _capi.FX_GAIN, {"gain": 0.7, "dcfm": 2})):
            m = g.add_mixer()
            ids[name] = g.add_effect(m, kind, params=params)
            g.add_effect(m, _capi.FX_FILTER, params={"cuto": 6000.0})
            g.add_voice(m, workloads.tone_buffer(len(ids), 44100, 0.3), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return ids

    gg, gc = Graph(SR, 2, 1024, 0), oracle.OracleGraph(SR, 2, 1024)
    outs, deferred = [], []
    for g in (gg, gc):
        ids = build(g)
        o = np.zeros((10, 2048), np.float32)
        for b in range(10):
            if b == 3:
                g.schedule_param(ids["gain"], "gain", 0.2, b * 1024 + 100)
                g.schedule_param(ids["pan"], "pan ", 0.7, b * 1024 + 300)
                g.schedule_param(ids["pan"], "wdth", 0.4, b * 1024 + 300)
                g.schedule_param(ids["dist"], "driv", 3.0, b * 1024 + 500)
                g.schedule_param(ids["dist"], "mix ", 0.9, b * 1024 + 700)
                g.schedule_param(ids["dcgain"], "gain", 1.5, b * 1024 + 900)
            assert g.write(o[b], b * 1024) == 2048
            if g is gg:
                deferred.append(g.deferred_units())
        outs.append(o.reshape(-1))
    compare(outs[0], outs[1])
    assert deferred[2] == 0 and deferred[3] == 4 and deferred[4] == 0 and deferred[5] == 0, deferred   # (block 2: the steady partial mix is on the fast kernel too)
    assert gg.device_errors() == 0


def test_long_run_past_every_ring_wrap_without_drift():
    """1100 blocks of 1024 frames (1 126 400 frames, 23 s): the Delay's 262 144-frame f64 lines wrap four times (the other rings — chorus line,
    predelay, reverb combs and allpasses — many times), the f32 LFO phases and the vibrato phases of the reverb lines pass thousands of
    periods, the looping sources wrap hundreds of times. The difference to the oracle must not grow: the last 32 blocks are held to the
    same tolerance as the first 32."""
    def build(g):
        workloads.build_c5(g, 2, 0, 2, seconds=0.37)
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_CHORUS)
        g.add_effect(m, _capi.FX_DELAY, params={"mode": 1, "dlay": 3900.0, "fdbk": 0.55, "lfor": 0.31, "lfos": 1, "lfdt": 0.02, "ldfb": 0.2})
        g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.8})
        g.add_voice(m, workloads.tone_buffer(9, 44100, 0.41), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_DELAY, params={"dlay": 2600.0, "fdbk": 0.7, "ftyp": 2, "cuto": 2500.0, "driv": 0.2})
        g.add_effect(m, _capi.FX_REVERB, params={"room": 0.8, "wet ": 0.6}, reverb_seeds=workloads.reverb_seeds(77))
        g.add_voice(m, workloads.tone_buffer(15, 44100, 0.29, channels=1), 1, 44100, volume=0.6, speed=0.83, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return {}
    n_blocks = 1100
    a, b = both(build, n_blocks, 1024, max_frames=1024)
    compare(a, b)
    first = compare(a[:32 * 2048], b[:32 * 2048])
    last = compare(a[-32 * 2048:], b[-32 * 2048:])
    assert np.abs(a[-32 * 2048:]).max() > 1e-2
    assert last <= max(4.0 * first, 2e-6), (first, last)
    from phonic_amd.graph import Graph

    g = Graph(SR, 2, 1024, 0)
    build(g)
    out = np.zeros(2048, np.float32)
    for i in range(5):
        g.write(out, i * 1024)
    assert g.deferred_units() == 0


def test_reverb_room_size_ramp_hands_the_rest_of_the_block_back_to_the_time_parallel_path():
    """ReverbEffect while its room size moves (LinearSmoothedValue, 0.01 x 44100 / fs per frame: <= 109 frames; the ring lengths change per frame):
    the generic kernel runs the smoother's pending frames on the serial lane and offers the rest of the block to the time-parallel paths (steady
    state, or the wet ramp when `wet` moves too). Commands at a block start, in mid-block, 40 frames before a block end (the ramp crosses into the
    next block), growing and shrinking rooms (a shrunk ring may leave a position above its new end: that unit stays serial a block longer), with and
    without a simultaneous wet change, ragged block sizes, lean / wide / staged units."""
    from phonic_amd.graph import Graph

    def build(g):
        ids = []
        for i in range(2):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_EQ5, params={"gan2": -3.0})
            ids.append(g.add_effect(m, _capi.FX_REVERB, params={"room": 0.3 + 0.4 * i}, reverb_seeds=workloads.reverb_seeds(60 + i)))
            g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.9})
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.3), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        for i in range(2):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.7})
            ids.append(g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(70 + i)))
            g.add_voice(m, workloads.tone_buffer(5 + i, 48000, 0.3), 2, 48000, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return ids

    sizes = [1024, 1024, 1024, 700, 1024, 333, 1024, 1024, 1024, 1024, 1024, 1024]
    gg, gc = Graph(SR, 2, 1024, 0), oracle.OracleGraph(SR, 2, 1024)
    outs = []
    for g in (gg, gc):
        ids = build(g)
        chunks, pos = [], 0
        for b, n in enumerate(sizes):
            if b == 2:
                g.schedule_param(ids[0], "room", 0.95, pos)             # at the block start, growing
                g.schedule_param(ids[2], "room", 0.1, pos + 500)        # mid-block, shrinking
            if b == 4:
                g.schedule_param(ids[1], "room", 0.2, pos + n - 40)     # the ramp crosses the block end
                g.schedule_param(ids[3], "room", 1.0, pos + 17)
                g.schedule_param(ids[3], "wet ", 0.9, pos + 17)         # room and wet together: the wet ramp takes over behind the room ramp
            if b == 7:
                g.schedule_param(ids[0], "room", 0.5, pos + 1000)
                g.schedule_param(ids[0], "wet ", 0.1, pos + 1010)       # a second command inside the room ramp
                g.schedule_param(ids[2], "room", 0.6, pos + 1023)
            o = np.zeros(2 * n, np.float32)
            assert g.write(o, pos) == 2 * n
            chunks.append(o)
            pos += n
        outs.append(np.concatenate(chunks))
    compare(outs[0], outs[1])
    assert np.abs(outs[0][-2048:]).max() > 1e-3
    assert gg.device_errors() == 0 and gg.deferred_units() == 0


def test_device_failure_makes_the_graph_silent_for_good():
    """SURVEY §8b error convention: `write` is infallible in the reference — a panic inside it is caught once by GuardedSource, which returns 0
    from then on (src/source/guarded.rs:87-107). Here a device failure inside write plays the panic's part: the failing call returns 0, the handle
    stays failed (every later write returns 0 at once, nothing is launched), pg_last_error_message names the cause, and the control calls are
    still accepted (a handle may outlive its source). Injected with pg_debug_fail_launch_round; the sharded handle fails as a whole when one
    of its shards does; other graphs of the process are untouched."""
    import gc

    from phonic_amd.graph import Graph, ShardedGraph, hip_calls

    lib = _capi.load()
    N = 512

    def build(g):
        m = g.add_mixer()
        fx = g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(9))
        v = g.add_voice(m, workloads.tone_buffer(2, 44100, 0.2), 2, 44100, volume=0.5, has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)
        return fx, v

    g, healthy = Graph(SR, 2, N, 0), Graph(SR, 2, N, 0)
    fx, v = build(g)
    build(healthy)
    out = np.zeros(2 * N, np.float32)
    assert g.write(out, 0) == 2 * N and healthy.write(out, 0) == 2 * N
    lib.pg_debug_fail_launch_round(2)
    assert g.write(out, N) == 2 * N                          # the first round from now still runs
    out[:] = 3.0
    assert g.write(out, 2 * N) == 0                          # the second fails: 0, like a panicked GuardedSource
    assert b"injected device failure" in lib.pg_last_error_message()
    gc.collect()   # (the counters are process-wide: graphs of earlier tests that sit in reference cycles are released here, not by a collection inside the window)
    launches_before = hip_calls()
    for b in range(3, 6):
        assert g.write(out, b * N) == 0                      # ... and stays silent
    assert hip_calls() == launches_before
    g.schedule_param(fx, "room", 0.3, 10 * N)                 # handles keep working (messages are queued, never applied)
    g.set_voice_volume(v, 0.1, 10 * N)
    assert healthy.write(out, N) == 2 * N and np.abs(out).max() > 1e-4      # another graph is not affected
    s = ShardedGraph([0, 0], SR, 2, N)
    for _ in range(2):
        build(s)
    assert s.write(out, 0) == 2 * N
    lib.pg_debug_fail_launch_round(2)                         # the second shard's round of the next write
    assert s.write(out, N) == 0 and s.write(out, 2 * N) == 0
    lib.pg_debug_fail_launch_round(0)

@pytest.mark.parametrize("feed", ["resampled", "host_fed"])
def test_adapter_backed_reverb_units_render_on_their_staged_kernel(feed):
    """Round 5: a reverb-terminated sub-mixer whose voice sits behind a ResampledSource
    (src/source/resampled.rs:27-152) or is fed by the host (pg_graph_add_stream_voice) is a staged unit of level 3 — pg_stage_fused_adapt_kernel,
    the wide staged kernel with the source adapters in its source stage — instead of a unit of the fused fast kernel at two workgroups per CU.
    Ragged call sizes walk the 512-frame staging ranges through every alignment; single launches and super-block launches; a one-shot voice runs
    out inside a call (the ResampledSource is asked again and plays its stale input range: PgVoice::zombie_end). Against the oracle, and the
    staged render against the same graph with the staged kernels off."""
    from phonic_amd.graph import Graph

    sizes = [1024, 1024, 700, 1024, 324, 1024, 1024, 512, 2048, 1024, 3072, 1024]

    def build(g):
        fed = []
        for i in range(6):
            m = g.add_mixer()
            if i % 2:
                g.add_effect(m, _capi.FX_FILTER, params={"cuto": 2500.0 + 300.0 * i})
            g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
            if feed == "resampled":
                g.add_voice(m, workloads.tone_buffer(i, 44100, 0.25 if i == 4 else 0.12), 2, 44100, volume=0.25, panning=workloads.voice_pan(i), source_rate=32000,
                            **({} if i == 4 else dict(has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER)))
            else:
                fed.append(g.add_stream_voice(m, 2, SR, 65536, volume=0.25, panning=workloads.voice_pan(i)))   # (the whole render fits: the host feeds ahead of every call)
        return fed

    def render(g, fed):
        rng = np.random.default_rng(7)
        chunks, pos = [], 0
        for n in sizes:
            for k, v in enumerate(fed):
                g.feed_voice(v, (0.3 * rng.standard_normal((n, 2))).astype(np.float32))
            o = np.zeros(2 * n, np.float32)
            assert g.write(o, pos) == 2 * n
            chunks.append(o)
            pos += n
        return np.concatenate(chunks)

    gg = Graph(SR, 2, 1024, 0)
    gg.set_max_blocks_per_launch(4)
    a = render(gg, build(gg))
    assert "pg_stage_fused_adapt_kernel" in gg.dominant_kernel(), gg.dominant_kernel()
    assert np.abs(a).max() > 1e-3 and gg.device_errors() == 0
    if feed == "resampled":   # (the oracle has no host-fed sources: those are held against the preloaded voice, tests/test_gpu_stream_voices.py)
        go = oracle.OracleGraph(SR, 2, 1024)
        b = render(go, build(go))
        compare(a, b, 1e-5, 1e-4)
    g0 = Graph(SR, 2, 1024, 0)
    g0.set_staged(0)
    f0 = build(g0)
    c = render(g0, f0)
    assert "pg_stage" not in g0.dominant_kernel()
    compare(a, c, 1e-6, 1e-5)


def test_sharded_direct_delivery_equals_the_copies(monkeypatch):
    """Round 5: in the peer-copy mode a shard's mixer sum writes its partial bus and its `audible` words straight into the root's gather ring /
    word banks (pg_sharded.hip: direct delivery; regions and banks rotate over four segments). Bit-identical to the copies (PHONIC_SHARD_DIRECT=0)
    over one-block calls issued back to back without a host wait (the ring comes round many times), a long call (one region, the last sum awaited)
    and voices that end under a bus Delay (silent shards: their words must be this call's)."""
    import torch
    from phonic_amd.graph import ShardedGraph

    N = 1024

    def build(g):
        for i in range(7):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_REVERB, reverb_seeds=workloads.reverb_seeds(i))
            g.add_voice(m, workloads.tone_buffer(i, 44100, 0.1 if i < 5 else 0.35), 2, 44100, volume=0.3, panning=workloads.voice_pan(i),
                        **(dict(has_repeat=1, repeat=_capi.PG_REPEAT_FOREVER) if i < 5 else {}))
        g.add_effect(0, _capi.FX_DELAY)

    def run(direct):
        monkeypatch.setenv("PHONIC_SHARD_DIRECT", "1" if direct else "0")
        g = ShardedGraph([0, 0, 0], SR, 2, N)
        g.set_max_blocks_per_launch(4)
        build(g)
        calls = 30
        d = torch.zeros((calls + 1, 8 * N), dtype=torch.float32, device="cuda:0")
        pos = 0
        for c in range(calls):   # one-block calls in flight
            assert g.write_device(d[c].data_ptr(), 2 * N, pos) == 2 * N
            pos += N
        assert g.write_device(d[calls].data_ptr(), 8 * N, pos) == 8 * N   # a four-block call behind them
        g.synchronize()
        assert g.device_errors() == 0
        out = d.cpu().numpy().copy()
        g.close()
        return out

    a, b = run(True), run(False)
    assert np.array_equal(a, b)
    assert np.abs(a).max() > 1e-2


def test_voice_commands_do_not_end_the_steady_state_of_offline_calls():
    """Round 5 (pg_host.hip: cmd may_ramp / feedback word 3): source volume / panning / stop commands leave no smoother of an EFFECT moving, so a
    unit deferred for those alone is back on its time-parallel kernel in the next block and the host keeps rendering super-block launches between
    such commands WITHOUT waiting for the device to report the steady state — here: eight-block calls enqueued back to back on a caller's stream
    (no host wait: the feedback of a commanded round has not arrived when the next span is planned), notes that stop and restart at random sample
    times plus volume / panning commands. Bit for bit the render of the same calls piece by piece (max_blocks 1), within tolerance of the oracle,
    no consistency flag, and most blocks in launches of several blocks; a reverb `wet` command in the middle (it CAN start a ramp) must take the
    graph off the super-block path until the device says the ramp has ended."""
    import torch
    from phonic_amd.graph import Graph

    N, per_call, calls = 1024, 8, 12
    stream = torch.cuda.Stream()

    def run(g, async_calls):
        plan = workloads.build_dyn(g, 24, calls * per_call * N / SR, churn_pct_per_s=12.0, silent_pct=0.0, first_frame=2 * per_call * N, seed=5, sample_rate=SR)
        drv = workloads.DynDriver(plan, 5.0, 11, sample_rate=SR, kinds=(1, 2))
        d = torch.zeros((calls, per_call * 2 * N), dtype=torch.float32, device="cuda:0") if async_calls else None
        o = np.zeros((calls, per_call * 2 * N), np.float32)
        n_cmds = 0
        for c in range(calls):
            pos = c * per_call * N
            if c >= 2:
                n_cmds += drv.schedule(g, pos, pos + per_call * N)
            if c == calls - 2:
                g.schedule_param(plan["reverbs"][3], "wet ", 0.45, pos + 3 * N + 17)
            if async_calls:
                if c == calls - 2:   # what the calls with voice commands alone took: most of their blocks rode in launches of several blocks
                    torch.cuda.synchronize()
                    _, launches, blocks = g.kernel_stats(reset=True)
                    stats.append((launches, blocks))
                assert g.write_device(d[c].data_ptr(), per_call * 2 * N, pos, stream.cuda_stream) == per_call * 2 * N
                if c < 2:
                    torch.cuda.synchronize()   # (the graph has played for a while: the device has reported its steady state once)
                    g.kernel_stats(reset=True)
            else:
                assert g.write(o[c], pos) == o[c].size
        if async_calls:
            torch.cuda.synchronize()
            o = d.cpu().numpy()
        assert n_cmds >= 8 and len(plan["restarts"]) >= 3
        return o.reshape(-1)

    stats = []
    ga = Graph(SR, 2, N, 0)
    ga.set_max_blocks_per_launch(per_call)
    ga.set_timing_period(1)
    a = run(ga, True)
    assert ga.device_errors() == 0
    launches, blocks = stats[0]
    # (a launch of several blocks covers whole chunks of four blocks or runs to the call's end, and a block with a command goes piece by piece with
    # the rest of its chunk: ~1.6 blocks per launch at one command every few blocks; it was 1.0 from the first command on while any command ended
    # the steady state — the host plans these calls before the device has rendered the first of them)
    assert blocks == (calls - 4) * per_call and blocks / max(1, launches) > 1.3, (launches, blocks)
    _, launches, blocks = ga.kernel_stats()
    assert blocks == 2 * per_call and launches >= per_call + 4, (launches, blocks)   # behind the `wet` command: block by block (the host has no word from the device yet)
    g1 = Graph(SR, 2, N, 0)
    b = run(g1, False)
    assert np.array_equal(a, b), f"{int(np.count_nonzero(a != b))} samples differ from the piece-by-piece render"
    c = run(oracle.OracleGraph(SR, 2, N), False)
    compare(a, c)
    assert np.abs(a).max() > 1e-2


def test_add_voice_that_fails_its_argument_checks_keeps_no_device_memory():
    """pg_graph_add_voice checks the resampling ratio and the loop range in front of its first allocation: a call that fails there with a
    ParameterError leaves the library's allocation and release counters (pg_debug_hip_calls) grown by the same amount, and the graph takes the
    next voice and renders it."""
    import gc

    import phonic_amd
    from phonic_amd.graph import Graph, hip_calls
    g = Graph(48000, 2, 256)
    pcm = (0.5 * np.sin(np.arange(64) * 0.3)).astype(np.float32)
    gc.collect()   # (the counters are process-wide: graphs of earlier tests are released here, not inside the window)
    before = hip_calls()
    for opts in (dict(has_loop_range=1, loop_start=5, loop_end=5),     # loop_start >= loop_end
                 dict(speed=64.0)):                                     # 192 kHz at 64x: a resampling ratio above 64
        with pytest.raises(phonic_amd.PhonicError) as ei:
            g.add_voice(0, pcm, 1, 192000, **opts)
        assert ei.value.code == _capi.PG_ERR_PARAMETER, ei.value
    after = hip_calls()
    assert after["alloc"] - before["alloc"] == after["free"] - before["free"], (before, after)
    assert g.add_voice(0, pcm, 1, 48000) == 0
    assert g.write(np.zeros(512, np.float32), 0) == 512
    assert g.device_errors() == 0
