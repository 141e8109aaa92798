"""The Sampler's note layer on the GPU where tests/test_gpu_sampler.py does not reach: pools of 9 to 64 voices (the wave-wide allocation beyond
lane 7 and across the 32-lane boundary), sample times beyond 2^32, mono / 44.1 kHz / looping buffers, messages out of time order, a start time,
removal with notes sounding, two samplers in one sub-mixer and a sampler in a nested sub-mixer. 48 kHz, pieces of 1024 frames, the sampler
alone in an effect-less sub-mixer unless a case says otherwise; the rig, the model and the expected audio are tests/sampler_rig.py's.

Where the sampler is alone in its mixer the slot table after EVERY write equals the model's, field by field, and the audio equals the
expected audio under np.array_equal. Two samplers in one mixer (H) are summed voice by voice here and sum by sum in the reference: the bound of
tests/test_gpu_ahdsr.py for shared mixers, RMS <= 1e-5 and max <= 1e-4.

What every scripted case expects of the allocation is written down by hand and asserted on the model first: the model is pinned by
tests/test_sampler_model.py, the device must then agree with it."""
import numpy as np
import pytest

from phonic_amd import _capi, workloads
from phonic_amd._wrap import PhonicError
from phonic_amd.graph import Graph
from sampler_rig import (ENV, LONG, MF, POOL_CASES, POOL_MESSAGES, POOL_PIECES, SHORT, SR, Rig, _assert_equal, _run, _single,
                         assert_pool_script_conditions, pool_rng, pool_script)

pytestmark = pytest.mark.gpu

POOLS = [9, 32, 33, 64]
ENVS = [False, True]


def _env(on):
    return ENV if on else None


def _fill(r, n, notes=None, step=10):
    """One note per slot, slot i at frame step * i of the first piece."""
    return [r.on(step * i, 60 if notes is None else notes[i], 0.5 + 0.004 * i, -0.6 + 0.015 * i) for i in range(n)]


def _slot_of(r, k):
    return r.m.notes[r.ids[k]].slot


# ---- A. large pools, scripted ----
@pytest.mark.parametrize("envelope", ENVS)
@pytest.mark.parametrize("n", POOLS)
def test_a1_steal_by_oldest_id(n, envelope):
    g, r = _single(LONG, n, envelope=_env(envelope))
    first = _fill(r, n)
    a, b = r.on(1500, 67, 0.7, 0.1), r.on(1600, 69, 0.6, -0.1)
    got = _run(g, [r], [MF] * 3)
    assert [_slot_of(r, k) for k in first] == list(range(n))
    assert (_slot_of(r, a), _slot_of(r, b)) == (0, 1)
    assert r.m.notes[r.ids[a]].stole == r.ids[first[0]] and r.m.notes[r.ids[b]].stole == r.ids[first[1]]
    _assert_equal(got, r.expected(3 * MF))


@pytest.mark.parametrize("envelope", ENVS)
@pytest.mark.parametrize("n,free", [(9, (8,)), (32, (31,)), (33, (32,)), (64, (63,)), (64, (47,)), (9, (2, 8)), (32, (8, 31)), (33, (8, 32)), (64, (16, 63))])
def test_a2_free_slot_in_the_upper_half(n, free, envelope):
    """The slots of `free` play the 6001-frame buffer at speed 2 (note 72) and end inside the fourth piece; the others last beyond the fifth. The
    next note-ons land exactly there, the lower slot first."""
    g, r = _single(SHORT, n, envelope=_env(envelope))
    _fill(r, n, notes=[72 if i in free else 60 for i in range(n)])
    late = [r.on(4200 + 100 * j, 62, 0.8, 0.2) for j in range(len(free))]
    got = _run(g, [r], [MF] * 6)
    assert [_slot_of(r, k) for k in late] == sorted(free)
    assert all(r.m.notes[r.ids[k]].stole is None for k in late)
    _assert_equal(got, r.expected(6 * MF))


@pytest.mark.parametrize("n,pair", [(9, (5, 7)), (32, (17, 30)), (33, (31, 32)), (64, (35, 50))])
def test_a3_earliest_release_beyond_lane_31(n, pair):
    g, r = _single(LONG, n, envelope=ENV)
    occ = _fill(r, n)                                # occ[slot]: the note that lives there
    victims = []

    def on(t, note, expect):
        k = r.on(t, note)
        victims.append((occ[expect], k, expect))
        occ[expect] = k

    r.off(2000, occ[n - 1])
    r.off(2001, occ[3])
    on(2100, 62, n - 1)                              # the earliest release: the last slot ...
    on(2200, 64, 3)                                  # ... then slot 3
    r.off(2500, occ[pair[1]])
    r.off(2500, occ[pair[0]])                        # one frame, the higher slot sent first: the lower one goes first
    on(2600, 65, pair[0])
    on(2700, 67, pair[1])
    r.all_off(3000)                                  # every slot releases from 3000: a tie of the whole pool
    on(3100, 69, 0)
    got = _run(g, [r], [MF] * 4)
    for old, new, slot in victims:
        assert _slot_of(r, new) == slot and r.m.notes[r.ids[new]].stole == r.ids[old] and r.m.notes[r.ids[old]].stolen_releasing, (slot, _slot_of(r, new))
    _assert_equal(got, r.expected(4 * MF))


@pytest.mark.parametrize("n,slot", [(33, 32), (64, 33)])
def test_a4_oldest_id_above_lane_31(n, slot):
    g, r = _single(LONG, n)
    first = _fill(r, n)
    again = [r.on(1100 + 20 * j, 62, 0.6, 0.3) for j in range(slot)]     # each steals the lowest id: slots 0 .. slot - 1 in turn
    a = r.on(1100 + 20 * slot + 50, 64)
    got = _run(g, [r], [MF] * 3)
    assert [_slot_of(r, k) for k in again] == list(range(slot))
    assert _slot_of(r, a) == slot and r.m.notes[r.ids[a]].stole == r.ids[first[slot]]
    _assert_equal(got, r.expected(3 * MF))


# ---- B. large pools, random ----
@pytest.mark.parametrize("voice_count,envelope,seed", POOL_CASES)
def test_b_random_scripts(voice_count, envelope, seed):
    g, r = _single(LONG, voice_count, envelope=_env(envelope))
    pool_script(r, pool_rng(voice_count, envelope, seed), POOL_PIECES * MF, POOL_MESSAGES)
    got = _run(g, [r], [MF] * POOL_PIECES)
    assert_pool_script_conditions(r.m, envelope)
    _assert_equal(got, r.expected(POOL_PIECES * MF))


# ---- C. sample times beyond 2^32 ----
def test_c_release_start_frames_on_both_sides_of_2_32():
    """Slot 1 releases at 2^32 - 100, slot 0 at 2^32 + 50: the smaller low word belongs to the LATER release. The next note-on steals slot 1."""
    top = 1 << 32
    p0 = top - 3 * MF
    g, r = _single(LONG, 4, envelope=ENV)
    first = [r.on(p0 + 10 * i, 60 + i, 0.8, -0.3 + 0.2 * i) for i in range(4)]
    r.off(top - 100, first[1])
    r.off(top + 50, first[0])
    a = r.on(top + 500, 67)
    b = r.on(top + 600, 69)
    got = _run(g, [r], [MF] * 6, pos=p0)
    assert (_slot_of(r, a), _slot_of(r, b)) == (1, 0)
    st = r.m.state()
    assert r.m.notes[r.ids[a]].start == top + 500 and st["slots"][2]["release_start_frame"] is None
    _assert_equal(got, r.expected(6 * MF, origin=p0))


# ---- D. what the pool plays ----
def _d_script(r):
    a, b, c = r.on(0, 60, 0.9, -0.2), r.on(300, 64, 0.8, 0.3), r.on(700, 55, 1.0, 0.0)
    d = r.on(1500, 67, 0.7, 0.1)                     # a steal: a, the lowest id
    r.off(2500, b)
    r.param(3500, "transpose", 5)
    r.speed(4500, c, 1.5, glide=12.0)
    e = r.on(5200, 62, 0.6, -0.4)                    # where nothing ends by itself b still fades (about 4800 frames to 1e-4) and goes: the lowest id
    return a, b, c, d, e


MONO = workloads.tone_buffer(1, SR, 6000 / SR, channels=1)


@pytest.mark.parametrize("what", ["mono", "stereo_44100", "mono_44100", "sampler_loop", "embedded_loop", "sampler_loop_over_embedded"])
def test_d_buffers_and_loops(what):
    kw = dict(mono=dict(channels=1), stereo_44100=dict(rate=44100), mono_44100=dict(channels=1, rate=44100), sampler_loop=dict(loop_range=(500, 4000)),
              embedded_loop=dict(buffer_loop=(1000, 5000)), sampler_loop_over_embedded=dict(loop_range=(500, 4000), buffer_loop=(1000, 5000)))[what]
    pcm = MONO if kw.get("channels") == 1 else SHORT
    g, r = _single(pcm, 3, **kw)
    a, b, c, d, e = _d_script(r)
    n = 12
    counts = []
    out, pos = [], 0
    for k in range(n):
        out.append(_run(g, [r], [MF], pos=pos))
        pos += MF
        counts.append(r.m.state()["active_voices"])
    got = np.concatenate(out)
    notes = r.m.notes
    assert notes[r.ids[a]].stolen and notes[r.ids[a]].end == 1500 and _slot_of(r, d) == 0
    if "loop" in what:
        assert r.loop == ((500, 4000) if "sampler" in what else (1000, 5000))
        assert g.sample_buffer_info(r.buf)["loop_range"] == kw.get("buffer_loop")
        # nothing ends by itself: three notes sound behind every piece, b goes to e while it fades
        assert counts == [3] * n and _slot_of(r, e) == 1 and notes[r.ids[e]].stole == r.ids[b] and notes[r.ids[b]].stop_frames == [2500]
        assert notes[r.ids[c]].end is None and notes[r.ids[d]].end is None and notes[r.ids[e]].end is None
    else:
        assert counts[-1] < 3                        # the 6001 frames end by themselves
    _assert_equal(got, r.expected(n * MF))


# ---- E. message order ----
def test_e_out_of_order_base_pitch():
    g, r = _single(LONG, 3)
    r.param(4000, "transpose", 7)
    r.param(2000, "finetune", -40)
    a, b = r.on(1000, 60), r.on(3000, 64)
    got = _run(g, [r], [MF] * 6)
    pf = lambda tr, ft: 2.0 ** (tr / 12.0 + ft / 1200.0)
    ea, eb = r.m.notes[r.ids[a]].speed_events, r.m.notes[r.ids[b]].speed_events
    assert [t for t, _, _ in ea] == [1000, 2000, 4000] and [t for t, _, _ in eb] == [3000, 4000]
    assert ea[0][1] == 1.0 and abs(ea[1][1] - pf(0, -40)) < 1e-12 and abs(ea[2][1] - pf(7, -40)) < 1e-12
    assert abs(eb[0][1] - 2.0 ** (4 / 12.0) * pf(0, -40)) < 1e-12
    st = g.sampler_state(r.s)
    assert (st["transpose"], st["finetune"]) == (7, -40)
    _assert_equal(got, r.expected(6 * MF))


@pytest.mark.parametrize("note_first", [True, False])
def test_e_same_frame_send_order(note_first):
    g, r = _single(LONG, 3)
    r.on(0, 57, 0.9, 0.1)
    if note_first:
        a = r.on(1500, 60, 0.8, -0.2)
        r.param(1500, "volume", 0.5)
    else:
        r.param(1500, "volume", 0.5)
        a = r.on(1500, 60, 0.8, -0.2)
    got = _run(g, [r], [MF] * 4)
    ev = r.m.notes[r.ids[a]].volume_events
    assert [float(x) for _, x in ev] == ([float(np.float32(0.8)), float(np.float32(0.5) * np.float32(0.8))] if note_first else [float(np.float32(0.5) * np.float32(0.8))])
    _assert_equal(got, r.expected(4 * MF))


def test_e_late_messages():
    g, r = _single(LONG, 3, envelope=ENV)
    a, b = r.on(0, 60, 0.9, -0.2), r.on(400, 64, 0.8, 0.3)
    got = [_run(g, [r], [MF] * 3)]
    r.off(500, a)                                    # stamped with a frame that is over: both apply at the next write's first frame
    c = r.on(500, 67, 0.7, 0.1)
    got.append(_run(g, [r], [MF] * 3, pos=3 * MF))
    assert r.m.notes[r.ids[c]].start == 3 * MF and r.m.notes[r.ids[a]].release_frames == [3 * MF]
    _assert_equal(np.concatenate(got), r.expected(6 * MF))


# ---- F. start_time ----
@pytest.mark.parametrize("start,in_order", [(1500, True), (1024, False)])
def test_f_start_time(start, in_order):
    """Messages that come due before the sampler's start time wait in its queue (mixed.rs:565-576, :902-918) and apply at the top of its first
    write, by sample time and then by sending order; nothing sounds before it."""
    g, r = _single(LONG, 3, envelope=ENV, start_time=start)
    sends = [lambda: r.on(100, 60, 0.8, -0.2), lambda: r.param(200, "volume", 0.5), lambda: r.off(300, None), lambda: r.on(start, 64, 1.0, 0.3)]
    for k in ((0, 1, 2, 3) if in_order else (1, 3, 2, 0)):
        sends[k]()
    a, b = (0, 1) if in_order else (1, 0)            # positions in r.ids: the note of frame 100, the note of the start time
    got = _run(g, [r], [MF] * 5)
    na, nb = r.m.notes[r.ids[a]], r.m.notes[r.ids[b]]
    assert (na.start, nb.start, na.slot, nb.slot) == (start, start, 0, 1)
    assert [float(x) for _, x in na.volume_events] == [float(np.float32(0.8)), float(np.float32(0.5) * np.float32(0.8))] and [t for t, _ in na.volume_events] == [start, start]
    assert [float(x) for _, x in nb.volume_events] == [0.5]
    assert not got[:2 * start].any() and got[2 * start:2 * (start + 600)].any()
    _assert_equal(got, r.expected(5 * MF))


# ---- G. removal ----
def test_g_remove_sampler_with_notes_sounding():
    g = Graph(SR, 2, MF, 0)
    ids = [0]
    r0, r1 = Rig(g, g.add_mixer(), LONG, ids, 3, envelope=ENV), Rig(g, g.add_mixer(), SHORT, ids, 3)
    r0.on(0, 60, 0.9, -0.2), r1.on(100, 64, 0.8, 0.3), r0.on(700, 55), r1.on(1300, 59, 0.7, -0.5)
    r0.off(2000, 0)
    r1.on(3500, 62), r1.off(5000, 1), r1.param(6000, "transpose", -3)
    r0.on(4000, 67)                                  # still queued when the sampler goes ...
    r0.param(5000, "volume", 0.5)                    # ... and this one
    n0, n = 3, 9
    got = [_run(g, [r0, r1], [MF] * n0)]
    assert r0.m.state()["active_voices"] == 2 and g.sample_buffer_info(r0.buf)["use_count"] == 3
    g.remove_sampler(r0.s)
    got.append(_run(g, [r1], [MF] * (n - n0), pos=n0 * MF))
    got = np.concatenate(got)
    with pytest.raises(PhonicError) as e:
        g.sampler_state(r0.s)
    assert e.value.code == _capi.PG_ERR_NOT_FOUND
    with pytest.raises(PhonicError) as e:
        g.sampler_note_on(r0.s, 60)
    assert e.value.code == _capi.PG_ERR_NOT_FOUND
    g.add_mixer()                                    # a graph-changing call: the removed pool's buffer references return
    assert g.sample_buffer_info(r0.buf)["use_count"] == 0 and g.sample_buffer_info(r1.buf)["use_count"] == 3
    assert g.device_errors() == 0
    e0 = np.concatenate([r0.expected(n0 * MF), np.zeros(2 * (n - n0) * MF, np.float32)])   # exact up to the third write's end, absent after
    e1 = r1.expected(n * MF)
    assert np.abs(e0).max() > 1e-3 and np.abs(e0[2 * (n0 - 1) * MF:2 * n0 * MF]).max() > 1e-3
    _assert_equal(got, (e0 + e1).astype(np.float32))   # the main mixer's sum of two sub-mixers: one f32 addition per sample
    assert np.array_equal(got[2 * n0 * MF:], e1[2 * n0 * MF:])


# ---- H. shared and nested mixers ----
def test_h_two_enveloped_samplers_in_one_sub_mixer():
    """Each sampler's messages cut the other's chunks (the mixer cuts at all of its events): each model gets the other's message times as
    extra_cuts, and the slot tables are exact after every write. The audio's twin: the CPU oracle has no envelope, so the models' notes cannot
    stand in ONE oracle graph as test_gpu_sampler.py's case 10 puts them; every note is rendered as an oracle voice of its own and multiplied by
    the model's envelope gains (expected_audio), per sampler in slot order, and the mixer adds the two samplers' sums (mixed.rs:578-609).
    The device adds voice by voice: the bound for shared mixers of tests/test_gpu_ahdsr.py."""
    g = Graph(SR, 2, MF, 0)
    mg = g.add_mixer()
    ids = [0]
    r0, r1 = Rig(g, mg, SHORT, ids, 4, envelope=ENV), Rig(g, mg, LONG, ids, 4, envelope=ENV)
    r0.on(0, 60, 0.8, -0.3), r1.on(150, 64, 0.7, 0.4)
    r0.on(900, 67, 0.6, 0.2), r1.on(1700, 55, 0.9, -0.1)
    r0.off(2300, 0), r1.off(3100, 0)
    r1.param(4000, "volume", 0.6), r0.param(4700, "transpose", 2)
    r0.on(5800, 62, 0.7, 0.0), r1.off(5900, 1)       # r0's first note (6001 frames, faster from 4700) ends in a write that these two cut
    r0.speed(7000, 1, 1.25), r1.on(7900, 59, 0.5, 0.5), r0.all_off(9000), r1.vol(9500, 2, 0.3)
    r0.m.extra_cuts, r1.m.extra_cuts = sorted(set(r1.times)), sorted(set(r0.times))
    n = 12
    got = _run(g, [r0, r1], [MF] * n)
    assert all(not rec.stolen for rig in (r0, r1) for rec in rig.m.notes.values())
    assert r0.m.notes[r0.ids[0]].end not in (None,) and r0.m.notes[r0.ids[0]].end % MF != 0      # freed behind a write that another event ended
    exp = (r0.expected(n * MF) + r1.expected(n * MF)).astype(np.float32)
    d = got.astype(np.float64) - exp.astype(np.float64)
    rms, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"two samplers in one mixer: rms {rms:.3e} max {mx:.3e} (signal peak {np.abs(exp).max():.3f})")
    assert np.abs(exp).max() > 1e-2
    assert rms <= 1e-5 and mx <= 1e-4


@pytest.mark.parametrize("plain", [True, False])
def test_h_sampler_in_a_nested_sub_mixer(plain):
    """A sampler alone in a sub-mixer of a sub-mixer, a plain voice with a volume event in the outer one: the outer mixer's event is a call
    boundary of the inner one (mixed.rs:679-712), so the model cuts there too. Without the plain voice the audio is the sampler's alone: exact."""
    g = Graph(SR, 2, MF, 0)
    outer = g.add_mixer()
    inner = g.add_mixer(outer)
    r = Rig(g, inner, SHORT, [0], 3, envelope=ENV)
    if plain:
        v = g.add_voice(outer, workloads.tone_buffer(5, SR, 0.2), 2, SR, start_time=200, volume=0.5)
        g.set_voice_volume(v, 0.25, 6050)            # an event of the outer mixer: one more call of the inner one begins there
        r.m.extra_cuts = [6050]
    a, b, c = r.on(0, 60, 0.9, -0.2), r.on(300, 64, 0.8, 0.3), r.on(700, 55)
    d = r.on(1500, 67, 0.7, 0.1)
    r.off(2500, b)
    r.param(3500, "finetune", 30)
    r.speed(4500, c, 1.5, glide=12.0)
    n = 10
    got = _run(g, [r], [MF] * n)
    assert r.m.notes[r.ids[a]].stolen and _slot_of(r, d) == 0
    if plain:
        assert np.abs(got).max() > 1e-3
    else:
        _assert_equal(got, r.expected(n * MF))
