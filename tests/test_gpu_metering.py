"""Per-mixer peak / RMS level metering on the GPU (pg_graph_set_metering / pg_graph_mixer_audio_level) against tests/metering_model.py, the
numpy restatement of the reference's AudioLevelState::record (src/source/metered.rs:75-143), fed with the samples the GPU itself returned.

Tolerances (derived, not measured): the peak is BIT-EQUAL — a maximum does not depend on the order. The RMS is within ONE f32 ulp: squares of
f32 values are exact in f64, any summation order of n <= 2^22 non-negative f64 terms is within n * 2^-53 relative of the exact sum, and
that leaves the two results at most one f32 rounding apart."""
import gc

import numpy as np
import pytest

from metering_model import AudioLevelState, interval_frames, ulp_distance
from phonic_amd import _capi
from phonic_amd._wrap import PhonicError
from phonic_amd.graph import Graph, ShardedGraph, hip_calls

pytestmark = pytest.mark.gpu

SR = 48000
ZERO = ((0.0, 0.0), (0.0, 0.0))


def noise(seed, frames, amp=0.4):
    """Seeded stereo noise + the zero frame a decoded file ends with."""
    rng = np.random.default_rng(seed)
    x = (amp * rng.uniform(-1.0, 1.0, 2 * frames)).astype(np.float32)
    return np.concatenate([x, np.zeros(2, np.float32)])


def lv(g, mixer=0):
    l = g.audio_level(mixer)
    return (l.peak, l.rms)


def assert_level(got, model, what=""):
    (gp, gr), (mp, mr) = got, model.level()
    print(what, "gpu", gp, gr, "model", mp, mr, "rms ulps", [ulp_distance(gr[c], mr[c]) for c in range(2)])
    assert gp == mp, (what, gp, mp)
    for c in range(2):
        assert ulp_distance(gr[c], mr[c]) <= 1, (what, c, gr[c], mr[c])


def write(g, pos, frames):
    buf = np.zeros(2 * frames, dtype=np.float32)
    n = g.write(buf, pos)
    return n, buf


def records(bus, pos, grid):
    """The bus of one call cut on a record grid: [(samples, start)] for chunk lengths `grid`."""
    out, off = [], 0
    for n in grid:
        out.append((bus[2 * off : 2 * (off + n)], pos + off))
        off += n
    assert 2 * off == bus.size
    return out


def chunks(frames):
    return [4096] * (frames // 4096) + ([frames % 4096] if frames % 4096 else [])


def sub_graph(max_frames=1024, interval=0.0, seed=3, frames=20000, main_gain=False):
    """Mixer 0 empty (or a unity Gain), one sub-mixer: voice -> Filter -> Reverb. The master bus is 0 + the sub-mixer's row."""
    g = Graph(SR, 2, max_frames, 0)
    fx0 = g.add_effect(0, _capi.FX_GAIN) if main_gain else None
    m = g.add_mixer()
    g.add_effect(m, _capi.FX_FILTER)
    g.add_effect(m, _capi.FX_REVERB, reverb_seeds=(16386, 16386, [0.1 * i for i in range(16)]))
    g.add_voice(m, noise(seed, frames), 2, SR)
    g.set_metering(interval)
    return g, m, fx0


# ---- 1: main mixer ------------------------------------------------------------------------------------------------------------------
def test_main_mixer_every_write():
    g = Graph(SR, 2, 1024, 0)
    g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.7})
    g.add_voice(0, noise(1, 4000), 2, SR)
    g.set_metering(0.0)
    assert lv(g) == ZERO
    model = AudioLevelState(0.0, SR)
    for k in range(8):
        n, buf = write(g, k * 256, 256)
        assert n == 512
        assert model.record(buf, k * 256)
        assert_level(lv(g), model, f"write {k}")
    assert max(lv(g)[0]) > 0.0
    g.close()


# ---- 2: publish timing --------------------------------------------------------------------------------------------------------------
def test_publish_timing():
    g = Graph(SR, 2, 1024, 0)
    g.add_effect(0, _capi.FX_GAIN)
    g.add_voice(0, noise(2, 8000), 2, SR)
    g.set_metering(0.025)
    assert interval_frames(0.025, SR) == 1200
    model = AudioLevelState(0.025, SR)
    published, last = [], ZERO
    for k in range(10):
        n, buf = write(g, k * 512, 512)
        assert n == 1024
        pub = model.record(buf, k * 512)
        published.append(pub)
        now = lv(g)
        if pub:
            assert_level(now, model, f"write {k}")
            assert now != last
        else:
            assert now == last, (k, now, last)   # unchanged between publishes; 0 before the first
        last = now
    assert published == [False, False, False, True, False, False, True, False, False, True]
    g.close()


# ---- 3: shapes that can break the kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_frames,frames", [(1024, 333), (1024, 4097), (128, 1000)], ids=["odd_333", "two_chunks_4097", "pieces_128x1000"])
def test_shapes_host_write(max_frames, frames):
    g = Graph(SR, 2, max_frames, 0)
    g.add_effect(0, _capi.FX_GAIN, params={"gain": 1.3})
    g.add_voice(0, noise(4, 12000), 2, SR)
    g.set_metering(0.0)
    model = AudioLevelState(0.0, SR)
    pos = 0
    for k in range(2):
        n, buf = write(g, pos, frames)
        assert n == 2 * frames
        model.record(buf, pos)          # ONE record per call, however many chunks or pieces
        assert_level(lv(g), model, f"call {k}")
        pos += frames
    g.close()


def test_super_block_launch_on_a_device_buffer():
    """max_frames 2048, four blocks per launch: a call of 8192 frames is two chunks — two records of the sub-mixer in one launch, one of the main mixer."""
    import torch

    mf, calls = 2048, 6
    g = Graph(SR, 2, mf, 0)
    g.set_max_blocks_per_launch(4)
    m = g.add_mixer()
    g.add_effect(m, _capi.FX_GAIN, params={"gain": 0.9})
    g.add_voice(m, noise(5, 4 * mf * calls + 100), 2, SR)
    g.set_metering(0.0)
    main, sub = AudioLevelState(0.0, SR), AudioLevelState(0.0, SR)
    d = torch.zeros(2 * 4 * mf, dtype=torch.float32, device="cuda")
    for k in range(calls):
        pos = k * 4 * mf
        assert g.write_device(d.data_ptr(), 2 * 4 * mf, pos) == 2 * 4 * mf
        bus = d.cpu().numpy()
        main.record(bus, pos)
        for x, t in records(bus, pos, [4096, 4096]):
            sub.record(x, t)
        assert_level(lv(g), main, f"main, call {k}")
        assert_level(lv(g, m), sub, f"sub-mixer, call {k}")
    assert g.device_errors() == 0
    g.close()


# ---- 4: sub-mixer equals bus --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [256, 333, 1000], ids=lambda n: f"{n}_frames")
def test_sub_mixer_equals_bus(frames):
    g, m, _ = sub_graph()
    model = AudioLevelState(0.0, SR)
    for k in range(4):
        n, bus = write(g, k * frames, frames)
        assert n == 2 * frames
        model.record(bus, k * frames)
        assert_level(lv(g, m), model, f"call {k}")
    assert max(lv(g, m)[0]) > 0.0
    g.close()


def test_sub_mixer_two_records_in_a_4097_frame_write():
    """4096 + 1: the second record starts at 4096. With an interval of 4096 frames it publishes what BOTH records collected; a single record of
    4097 frames starting at 0 would publish nothing."""
    interval = 4096 / SR
    assert interval_frames(interval, SR) == 4096
    g, m, _ = sub_graph(interval=interval)
    n, bus = write(g, 0, 4097)
    assert n == 2 * 4097
    model = AudioLevelState(interval, SR)
    pubs = [model.record(x, t) for x, t in records(bus, 0, [4096, 1])]
    assert pubs == [False, True]
    assert_level(lv(g, m), model, "two records")
    assert max(lv(g, m)[0]) > 0.0
    assert lv(g) == ZERO      # the main mixer: one record starting at 0
    g.close()


# ---- 5: a parent event cuts the sub-mixer's record ----------------------------------------------------------------------------------
def test_parent_event_cuts_the_record():
    cut, frames = 700, 1500
    interval = 600 / SR
    assert interval_frames(interval, SR) == 600
    g, m, fx0 = sub_graph(interval=interval, main_gain=True)
    g.schedule_param(fx0, "gain", 1.0, cut)
    n, bus = write(g, 0, frames)
    assert n == 2 * frames
    two = AudioLevelState(interval, SR)
    pubs = [two.record(x, t) for x, t in records(bus, 0, [cut, frames - cut])]
    assert pubs == [False, True]
    one = AudioLevelState(interval, SR)
    assert not one.record(bus, 0)
    got = lv(g, m)
    assert_level(got, two, "two-chunk grid")
    assert got != one.level()          # the uncut grid publishes nothing here
    g.close()


# ---- 6: several mixers, nested ------------------------------------------------------------------------------------------------------
def _nested(which):
    """main -> A (own voice) -> B (own voice), plus a sibling C; `which`: the mixers to build (B alone hangs off the main mixer)."""
    g = Graph(SR, 2, 1024, 0)
    ids = {}
    if "A" in which:
        ids["A"] = g.add_mixer()
        g.add_effect(ids["A"], _capi.FX_GAIN, params={"gain": 0.8})
        g.add_voice(ids["A"], noise(11, 6000), 2, SR)
    if "B" in which:
        ids["B"] = g.add_mixer(ids.get("A"))
        g.add_effect(ids["B"], _capi.FX_GAIN, params={"gain": 0.6})
        g.add_voice(ids["B"], noise(12, 6000), 2, SR)
    if "C" in which:
        ids["C"] = g.add_mixer()
        g.add_effect(ids["C"], _capi.FX_GAIN, params={"gain": 0.5})
        g.add_voice(ids["C"], noise(13, 6000), 2, SR)
    g.set_metering(0.0)
    return g, ids


def test_nested_mixers_equal_their_solo_graphs():
    sizes = [256, 333, 1000, 256]
    full, ids = _nested("ABC")
    levels = {k: [] for k in ids}
    pos = 0
    for n in sizes:
        assert write(full, pos, n)[0] == 2 * n
        for k, m in ids.items():
            levels[k].append(lv(full, m))
        pos += n
    full.close()
    for name, which in (("A", "AB"), ("B", "B"), ("C", "C")):
        solo, sid = _nested(which)
        model = AudioLevelState(0.0, SR)
        pos = 0
        for i, n in enumerate(sizes):
            w, bus = write(solo, pos, n)
            assert w == 2 * n
            model.record(bus, pos)
            got = lv(solo, sid[name])
            assert_level(got, model, f"solo {name}, call {i}")
            assert got == levels[name][i], (name, i, got, levels[name][i])     # bit-equal: the same kernel over the same row
            pos += n
        solo.close()


# ---- 7: an empty mixer freezes ------------------------------------------------------------------------------------------------------
def test_empty_main_mixer_freezes():
    g = Graph(SR, 2, 1024, 0)
    g.add_voice(0, noise(21, 300), 2, SR)
    g.set_metering(0.0)
    model = AudioLevelState(0.0, SR)
    last, zero_calls = None, 0
    for k in range(8):
        n, buf = write(g, k * 256, 256)
        if n:
            assert zero_calls == 0
            model.record(buf, k * 256)
            assert_level(lv(g), model, f"write {k}")
            last = lv(g)
        else:
            zero_calls += 1
            assert lv(g) == last and max(last[0]) > 0.0, (k, lv(g), last)
    assert zero_calls >= 3
    g.close()


def _ab(with_a, with_b):
    g = Graph(SR, 2, 1024, 0)
    a = b = None
    if with_a:
        a = g.add_mixer()
        g.add_voice(a, noise(22, 8000), 2, SR)
    if with_b:
        b = g.add_mixer()
        g.add_voice(b, noise(23, 300), 2, SR)      # no effects: the mixer returns 0 once its source is gone
    g.set_metering(0.0)
    return g, a, b


def test_empty_sub_mixer_freezes():
    calls = 8
    solo, _, sb = _ab(False, True)
    model, ended_at, expected = AudioLevelState(0.0, SR), None, None
    outs = [write(solo, k * 256, 256)[1] for k in range(calls)]
    solo.close()
    for k, bus in enumerate(outs):
        if np.any(bus != 0.0):
            ended_at = k
    assert ended_at == 1, ended_at      # 300 frames: the voice ends inside the second call
    for k in range(ended_at + 1):
        model.record(outs[k], k * 256)
    expected = model.level()
    g, a, b = _ab(True, True)
    la = []
    for k in range(calls):
        assert write(g, k * 256, 256)[0] == 512
        la.append(lv(g, a))
        print("call", k, "B", lv(g, b))
    got = lv(g, b)
    assert max(got[0]) > 0.0
    assert_level(got, model, "B, frozen")
    assert len(set(la[-4:])) == 4        # A's level keeps moving
    g.close()


# ---- 8: on and off ------------------------------------------------------------------------------------------------------------------
def test_on_and_off():
    def build():
        g = Graph(SR, 2, 1024, 0)
        g.add_effect(0, _capi.FX_GAIN)
        m = g.add_mixer()
        g.add_effect(m, _capi.FX_REVERB, reverb_seeds=(16386, 16386, [0.1 * i for i in range(16)]))
        g.add_voice(m, noise(31, 6000), 2, SR)
        return g, m

    off, m = build()
    with pytest.raises(PhonicError) as e:
        off.audio_level(0)
    assert e.value.code == _capi.PG_ERR_STATE
    on, _ = build()
    on.set_metering(0.0)
    a = np.concatenate([write(off, k * 256, 256)[1] for k in range(20)])
    b = np.concatenate([write(on, k * 256, 256)[1] for k in range(20)])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert max(lv(on)[0]) > 0.0 and max(lv(on, m)[0]) > 0.0
    on.set_metering(0.0)                       # enabling (again) mid-run: AudioLevelState::new
    assert lv(on) == ZERO and lv(on, m) == ZERO
    late = on.add_mixer()                      # added after enabling: metered too
    on.add_voice(late, noise(32, 2000), 2, SR, start_time=20 * 256)
    n, _ = write(on, 20 * 256, 256)
    assert n == 512 and max(lv(on, late)[0]) > 0.0
    on.remove_mixer(late)
    with pytest.raises(PhonicError) as e:
        on.audio_level(late)
    assert e.value.code == _capi.PG_ERR_NOT_FOUND
    with pytest.raises(PhonicError) as e:
        on.audio_level(99)
    assert e.value.code == _capi.PG_ERR_NOT_FOUND
    on.set_metering(None)
    with pytest.raises(PhonicError) as e:
        on.audio_level(0)
    assert e.value.code == _capi.PG_ERR_STATE
    off.close()
    on.close()


# ---- 9: real-time rules -------------------------------------------------------------------------------------------------------------
def test_no_allocation_no_wait_with_metering_on():
    import torch

    g, m, _ = sub_graph(interval=0.0, frames=40000)
    stream = torch.cuda.Stream()
    d = torch.zeros(2 * 1024, dtype=torch.float32, device="cuda")
    for k in range(4):       # warm-up: topology upload, first launches
        assert g.write_device(d.data_ptr(), 2048, k * 1024, stream.cuda_stream) == 2048
    stream.synchronize()
    gc.collect()   # (the counters are process-wide: graphs of earlier tests that sit in reference cycles are released here, not by a collection inside the window)
    before = hip_calls()
    for k in range(4, 24):
        assert g.write_device(d.data_ptr(), 2048, k * 1024, stream.cuda_stream) == 2048
        lv(g), lv(g, m)
    assert hip_calls() == before, (before, hip_calls())
    stream.synchronize()
    assert max(lv(g, m)[0]) > 0.0
    g.close()


# ---- 10: sharded --------------------------------------------------------------------------------------------------------------------
def test_sharded_levels():
    def build(g):
        g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.9})
        ms = []
        for i in range(2):
            m = g.add_mixer()
            g.add_effect(m, _capi.FX_FILTER)
            g.add_voice(m, noise(40 + i, 6000), 2, SR)
            ms.append(m)
        g.set_metering(0.0)
        return ms

    single = Graph(SR, 2, 1024, 0)
    ms = build(single)
    sharded = ShardedGraph([0, 0], SR, 2, 1024)
    mss = build(sharded)
    assert sorted(sharded.shard_of_mixer(m) for m in mss) == [0, 1]
    model = AudioLevelState(0.0, SR)
    for k in range(5):
        assert write(single, k * 333, 333)[0] == 666
        n, bus = write(sharded, k * 333, 333)
        assert n == 666
        model.record(bus, k * 333)
        assert_level(lv(sharded), model, f"mixer 0, call {k}")
        for a, b in zip(ms, mss):
            assert lv(sharded, b) == lv(single, a), (k, a)
            assert max(lv(sharded, b)[0]) > 0.0
    single.close()
    sharded.close()


# ---- 11: deferred bus ---------------------------------------------------------------------------------------------------------------
def test_deferred_bus_records_in_process_bus():
    import torch

    g = Graph(SR, 2, 1024, 0)
    g.add_effect(0, _capi.FX_GAIN, params={"gain": 0.5})
    m = g.add_mixer()
    g.add_effect(m, _capi.FX_FILTER)
    g.add_voice(m, noise(50, 6000), 2, SR)
    g.set_defer_bus(True)
    g.set_metering(0.0)
    model = AudioLevelState(0.0, SR)
    d = torch.zeros(2 * 512, dtype=torch.float32, device="cuda")
    for k in range(3):
        before = lv(g)
        assert g.write_device(d.data_ptr(), 1024, k * 512) == 1024
        assert lv(g) == before                           # the write leaves mixer 0's level alone
        assert max(lv(g, m)[0]) > 0.0                    # ... the sub-mixer's record is taken there
        g.process_bus_device(d.data_ptr(), 1024, k * 512)
        g.synchronize()
        model.record(d.cpu().numpy(), k * 512)
        assert_level(lv(g), model, f"call {k}")
    assert max(lv(g)[0]) > 0.0
    g.close()
