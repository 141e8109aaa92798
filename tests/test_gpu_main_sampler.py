"""Samplers on the MAIN mixer on the GPU (pg_graph_add_sampler_to_main, pg_graph_add_granular_sampler_to_main, pg_graph_sampler_set_volume /
_set_panning, pg_graph_sampler_output_state) against tests/main_sampler_model.py and the CPU oracle. 48 kHz, pieces of 1024 frames (granular
cases: 256). After EVERY write the slot table, the envelope read-back, a granular sampler's grain, matrix and parameter state and the output
stage's two smoothers equal the model's, the smoothers bit for bit (tests/main_sampler_rig.py).

Audio. A lone file sampler: the bus is 0 + the unit's row, so it must equal — as values; an all-zero sample may carry the other zero's sign —
the rig's expected audio: every note rendered through the CPU oracle, cut and enveloped as the model says, summed in slot order, then passed
through the model's output stage in f32. A lone granular sampler: the existing granular-sampler test's bar, equality as values with the model's
frames. Beside other sources the sum is re-associated: the project's bound for that, RMS <= 1e-5 and max <= 1e-4, figures printed.
Every test ends with a device-error count of 0 (the rigs' run functions assert it)."""
import numpy as np
import pytest

import granular_sampler_rig as GR
import main_sampler_rig as MR
import oracle
import sampler_live_rig as LR
from main_sampler_rig import FileRig, GranularRig, assert_values_equal, run_file
from phonic_amd import _capi, workloads
from phonic_amd._wrap import PhonicError
from phonic_amd.graph import Graph
from sampler_rig import ENV, LONG, MF, SHORT, SR
from test_main_sampler_model import GRID_ENV, GRID_SIZES, grid_script, ramp_stands_still_script

pytestmark = pytest.mark.gpu
F32 = np.float32
GMF = GR.MF


def _bound(got, exp, what):
    d = np.asarray(got, np.float64).reshape(-1) - np.asarray(exp, np.float64).reshape(-1)
    rms, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"{what}: rms {rms:.3e} max {mx:.3e} (signal peak {np.abs(exp).max():.3f})")
    assert np.abs(exp).max() > 1e-2
    assert rms <= 1e-5 and mx <= 1e-4


# ---- 1. a file sampler alone on the main mixer ----
POOL_SIZES = [1024, 1500, 7, 3000, 1024, 4096, 1024, 2000]   # 14675 frames; writes across pieces, of 7 frames, of a whole chunk


def pool_script(r, n, envelope):
    """Fills the pool, steals, releases, glides, moves the base parameters (and the envelope's), starts a note behind all that, lets go of every
    note and stops the — transient — sampler, which then leaves the mixer."""
    for i in range(n):
        r.on(10 * i, 60 + i % 12, 0.5 + 0.4 * (i % 3) / 2.0, -0.5 + (i % 5) / 4.0)
    steal = r.on(700, 67, 0.8, 0.2)                      # the pool is full: the lowest id goes
    r.off(900, steal)
    r.speed(1200, n - 1 if n > 1 else steal, 1.3, glide=24.0)
    r.param(1500, "volume", 0.7)
    r.param(1700, "transpose", 3)
    r.param(1900, "panning", -0.4)
    if envelope:
        r.env(2100, "ASTN", 0.5)
        r.env(2200, "AREL", 0.02)
    r.on(2531, 55, 0.9, 0.1)
    r.all_off(5000)
    r.stop(6000)


def _pool_run(n, envelope, max_blocks=None):
    g = Graph(SR, 2, MF, 0)
    if max_blocks is not None:
        g.set_max_blocks_per_launch(max_blocks)
    r = FileRig(g, LONG, [0], n, envelope=ENV if envelope else None, transient=True)
    pool_script(r, n, envelope)
    got = run_file(g, [r], POOL_SIZES)
    return g, r, got


@pytest.mark.parametrize("envelope", [False, True])
@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_1_file_sampler_alone(n, envelope):
    g, r, got = _pool_run(n, envelope)
    notes = list(r.m.notes.values())
    assert any(rec.stolen for rec in notes) and len(notes) == n + 2
    st = r.m.state()
    assert st["stopped"] and st["active_voices"] == 0           # stopped inside the run: the sampler left the mixer behind that write
    assert_values_equal(got, r.expected(sum(POOL_SIZES)))
    with pytest.raises(PhonicError):                            # the id takes no message any more; its read-backs stay (run_file read them)
        g.sampler_set_volume(r.s, 0.5, 0)
    tail = np.ones(2 * 64, F32)
    g.write(tail, sum(POOL_SIZES))
    assert (not tail.any() or (tail == 1.0).all()) and g.device_errors() == 0   # silence, or a write that found nothing to do: the mixer is empty


# ---- 2. the grid ----
def test_2_the_main_grid_and_the_sub_mixer_grid_side_by_side():
    """Model script (a) on a granular sampler with explicit generator states: on the main mixer the message at frame 1000 begins a chunk, the
    released slot's write ends at 5096; in a sub-mixer (the existing entry point) it ends at 6000. Each placement equals ITS model after every
    write, and the later note in that slot plays other grains."""
    states = [[tuple(1000 * (k + 1) + 10 * j + i for i in range(1, 5)) for j in range(3)] for k in range(2)]
    g1 = Graph(SR, 2, GMF, 0)
    main = GranularRig(g1, [0], 2, envelope=GRID_ENV, rng_states=states)
    grid_script(main)
    out_main = []
    pos = 0
    for k, n in enumerate(GRID_SIZES):
        buf = np.zeros(2 * n, F32)
        g1.write(buf, pos)
        exp = main.m.write(n, pos)
        main.check_state((k, pos + n))
        GR.assert_audio(buf, exp, (k, pos))
        out_main.append(buf)
        pos += n
    assert g1.device_errors() == 0
    assert main.m.span_log[:3] == [(0, 1000), (1000, 4096), (5096, 904)]
    g2 = Graph(SR, 2, GMF, 0)
    sub = GR.Rig(g2, g2.add_mixer(), [0], 2, envelope=GRID_ENV, rng_states=states)
    grid_script(sub)
    out_sub, _ = GR.run(g2, [sub], list(GRID_SIZES))
    assert sub.m.span_log[:3] == [(0, 1000), (1000, 3096), (4096, 1904)]
    assert np.array_equal(out_main[0].reshape(-1, 2), out_sub[:GRID_SIZES[0]])
    assert not np.array_equal(out_main[1].reshape(-1, 2), out_sub[GRID_SIZES[0]:])
    # both placements in ONE graph (short writes: a chunk is a write, and the main sampler's messages cut the sub-mixer's call too)
    g3 = Graph(SR, 2, GMF, 0)
    ids = [0]
    a = GranularRig(g3, ids, 2, envelope=GRID_ENV, rng_states=states, volume=0.5)
    b = LR.GRig(g3, g3.add_mixer(), ids, 2, envelope=GRID_ENV, rng_states=states)
    a.on(0, 60), b.on(40, 62)
    a.off(300, 0), b.off(500, 0)
    a.on(900, 64), b.on(1100, 65)
    pos = 0
    for k, n in enumerate([700, 7, 1000]):
        buf = np.zeros(2 * n, F32)
        g3.write(buf, pos)
        # (b's messages are its sub-mixer's events: they do not cut the main mixer's chunk; a's are the main mixer's and cut every call under it)
        ea, eb = a.m.write(n, pos), b.m.write(n, pos, cuts=set(a.times))
        a.check_state((k, "main")), b.check_state((k, "sub"))
        if n > 7:
            _bound(buf, ea.astype(np.float64) + eb.astype(np.float64), f"main and sub-mixer granular samplers, write {k}")
        pos += n
    assert g3.device_errors() == 0


# ---- 3. the output stage ----
def _stage_rig(kind, g, **kw):
    if kind == "file":
        return FileRig(g, LONG, [0], 3, **kw)
    return GranularRig(g, [0], 3, **kw)


def _stage_check(kind, r, got, n):
    if kind == "file":
        assert_values_equal(got, r.expected(n))


def _run_stage(kind, g, r, sizes):
    """run_file, with a granular sampler's audio compared write by write against the model's frames (equal as values)."""
    if kind == "file":
        return run_file(g, [r], sizes)
    out, pos = [], 0
    for k, n in enumerate(sizes):
        buf = np.zeros(2 * n, F32)
        g.write(buf, pos)
        exp = r.m.write(n, pos)
        r.check_state((k, pos + n))
        GR.assert_audio(buf, exp, (k, pos))
        out.append(buf)
        pos += n
    assert g.device_errors() == 0
    return np.concatenate(out)


@pytest.mark.parametrize("kind", ["file", "granular"])
def test_3_output_stage_messages_at_every_kind_of_edge(kind):
    """Constant non-default options; set_volume / set_panning inside a piece, on a piece edge, on a chunk edge and on a write's frame 0; two
    messages of a kind on one frame in both sending orders."""
    mf = MF if kind == "file" else GMF
    g = Graph(SR, 2, mf, 0)
    r = _stage_rig(kind, g, volume=0.6, panning=0.3)
    sizes = [3 * mf, 4096 + 2 * mf, 7, 2 * mf]
    w1 = sizes[0]                                  # the second write's first frame
    r.on(0, 60, 0.9, -0.2)
    r.on(50, 64, 0.8, 0.4)
    r.out_volume(300, 0.9)                         # inside a piece
    r.out_pan(mf, -0.5)                            # on a piece edge
    r.out_volume(w1, 0.3)                          # frame 0 of a write
    r.out_pan(w1 + 4096, 0.7)                      # on the edge of that write's first chunk
    t = w1 + 4096 + mf + 11
    r.out_volume(t, 0.5), r.out_volume(t, 1.2)     # one frame, two volumes: the last one sent counts ...
    r.out_pan(t, 0.2), r.out_pan(t, -0.9)
    t2 = sum(sizes[:3]) + 100
    r.out_volume(t2, 1.2), r.out_volume(t2, 0.25)  # ... in either order
    got = _run_stage(kind, g, r, sizes)
    assert r.m.output_state()["volume_target"] == F32(0.25) and r.m.output_state()["panning_target"] == F32(-0.9)
    assert any(isinstance(w[2], np.ndarray) for w in r.m.out.log) and any(isinstance(w[3], tuple) and isinstance(w[3][0], np.ndarray) for w in r.m.out.log)
    _stage_check(kind, r, got, sum(sizes))


@pytest.mark.parametrize("what", ["volume", "panning"])
@pytest.mark.parametrize("kind", ["file", "granular"])
def test_3_a_ramp_ends_inside_a_seven_frame_write(kind, what):
    import main_sampler_model as MM

    probe = MM.OutputStage(SR, 1.0, 0.0)
    probe.message(what, 0.25 if what == "volume" else 0.8)
    sm, steps = (probe.volume if what == "volume" else probe.panning), 0
    while sm.need_ramp():
        sm.next()
        steps += 1
    end = (steps + 1) // 2 if what == "volume" else steps      # the frame (behind the message) in which the last step is taken
    assert end > 100
    mf = MF if kind == "file" else GMF
    g = Graph(SR, 2, mf, 0)
    r = _stage_rig(kind, g)
    r.on(0, 60)
    t = 40
    (r.out_volume if what == "volume" else r.out_pan)(t, 0.25 if what == "volume" else 0.8)
    sizes = [t + end - 4, 7, 300]                                # the 7-frame write holds the ramp's last step
    got = _run_stage(kind, g, r, sizes)
    key = what + "_ramping"
    log = r.m.out.log
    assert len(log) == 4 and log[2][1] == 7                      # [0, t), [t, ..), the 7 frames, the rest
    seq = log[2][2] if what == "volume" else log[2][3][0]
    assert isinstance(seq, np.ndarray) and not r.m.output_state()[key]
    _stage_check(kind, r, got, sum(sizes))


@pytest.mark.parametrize("kind", ["file", "granular"])
def test_3_a_ramp_waits_for_the_next_note(kind):
    """Model script (c): the target is set at the message, the ramp's first step is the next note's first sample."""
    mf = MF if kind == "file" else GMF
    g = Graph(SR, 2, mf, 0)
    r = _stage_rig(kind, g)
    ramp_stands_still_script(r)
    got = _run_stage(kind, g, r, [2000, 2000])
    assert [w[2] for w in r.m.write_log[:2]] == [False, False] and r.m.out.log[0][0] == 3000
    assert not got[:2 * 3000].any() and got[2 * 3000:].any()
    _stage_check(kind, r, got, 4000)


@pytest.mark.parametrize("kind", ["file", "granular"])
def test_3_the_skip_branches(kind):
    """A volume within 1e-6 of 1 and a panning within 1e-6 of 0 leave the samples alone; just outside they do not."""
    outs = []
    for volume, panning in ((1.0 + 5e-7, 5e-7), (1.0, 0.0), (1.0 + 5e-6, 5e-6)):
        mf = MF if kind == "file" else GMF
        g = Graph(SR, 2, mf, 0)
        r = _stage_rig(kind, g, volume=volume, panning=panning)
        r.on(0, 60, 0.9, 0.3)
        got = _run_stage(kind, g, r, [700, 7])
        log = r.m.out.log
        assert all((w[2] is None and w[3] is None) == (volume < 1.000004) for w in log)
        _stage_check(kind, r, got, 707)
        outs.append(got)
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])


# ---- 4. beside other things ----
def test_4_between_plain_voices_a_sub_mixer_and_a_second_main_sampler():
    g = Graph(SR, 2, MF, 0)
    o = oracle.OracleGraph(SR, 2, MF)
    plain = workloads.tone_buffer(5, SR, 0.2)
    ids = [0]
    for h in (g, o):
        h.add_voice(0, plain, 2, SR, start_time=0, volume=0.5, panning=-0.3)            # added earlier: behind the pool in the mixer's sum
    a = FileRig(g, SHORT, ids, 4, volume=0.7, panning=0.2)
    for h in (g, o):
        h.add_voice(0, plain, 2, SR, start_time=0, volume=0.4, panning=0.6, speed=1.5)  # added later, same start time: in front of the pool
        m = h.add_mixer()
        h.add_effect(m, _capi.FX_GAIN, params={"gain": 0.5})
        h.add_voice(m, plain, 2, SR, start_time=100, volume=0.8)
    b = FileRig(g, LONG, ids, 2, envelope=ENV, volume=0.9, panning=-0.6)
    a.on(0, 60, 0.8, -0.3), b.on(200, 64, 0.7, 0.4)
    a.out_volume(900, 0.3), b.out_pan(1500, 0.5)
    a.on(2000, 67), b.off(3000, 0)
    n = 6
    got = run_file(g, [a, b], [MF] * n)
    exp = o.render(n, MF).astype(np.float64) + a.expected(n * MF).astype(np.float64) + b.expected(n * MF).astype(np.float64)
    _bound(got, exp, "two main-mixer samplers, two plain voices, a sub-mixer with a Gain")
    # the order of the main mixer's sources: the later plain voice, sampler a's pool, the earlier plain voice, ...
    assert g.device_errors() == 0


# ---- 5. a Delay on the main bus ----
def test_5_main_bus_delay_across_a_silent_gap():
    """The silent gap is longer than the Delay's tail: the sampler returns nothing over it (sampler.rs:974-981), the bus chain goes to sleep
    and wakes with the next note. Notes start on write edges, where the oracle's chunk grid and the main mixer's event grid coincide."""
    params = {"dlay": 5.0, "fdbk": 0.2}
    g = Graph(SR, 2, MF, 0)
    g.add_effect(0, _capi.FX_DELAY, params=params)
    r = FileRig(g, SHORT, [0], 2)
    r.on(0, 72, 0.9, -0.2)                 # an octave up: ~3000 frames
    r.on(28 * MF, 67, 0.8, 0.3)            # 25000 silent frames later
    n = 32
    got = run_file(g, [r], [MF] * n)
    assert [w[2] for w in r.m.write_log].count(False) >= 20
    o = oracle.OracleGraph(SR, 2, MF)
    o.add_effect(0, _capi.FX_DELAY, params=params)
    for rec in r.m.notes.values():
        v = o.add_voice(0, SHORT, 2, SR, volume=float(rec.inherited_volume), panning=float(rec.inherited_panning), speed=rec.speed_events[0][1], start_time=rec.start)
        for t, x in rec.volume_events:
            o.set_voice_volume(v, float(x), t)
        for t, x in rec.panning_events:
            o.set_voice_panning(v, float(x), t)
    exp = o.render(n, MF)
    assert np.abs(exp[2 * 28 * MF:]).max() > 1e-2 and exp[2 * 10 * MF:2 * 12 * MF].any() and not exp[2 * 24 * MF:2 * 28 * MF].any()   # the tail outlasts the note and ends inside the gap
    _bound(got, exp, "main-bus Delay behind a lone file sampler")


# ---- 6. the launch count ----
def test_6_blocks_per_launch_change_nothing():
    _, r1, got1 = _pool_run(8, True, max_blocks=1)
    _, r4, got4 = _pool_run(8, True, max_blocks=4)
    assert got1.tobytes() == got4.tobytes()
    assert r1.m.state()["slots"] == r4.m.state()["slots"]      # (both runs matched the model's slot table after every write)


# ---- 7. small checks ----
def test_7_removal_while_notes_sound():
    g = Graph(SR, 2, MF, 0)
    r = FileRig(g, LONG, [0], 3, volume=0.8)
    r.on(0, 60), r.on(100, 64)
    r.out_volume(5000, 0.1)                 # still queued when the sampler goes
    got = run_file(g, [r], [MF, 700])
    assert got[-200:].any()
    g.remove_sampler(r.s)
    tail = np.ones(2 * MF, F32)
    g.write(tail, MF + 700)
    assert not tail.any() or (tail == 1.0).all()   # silence, or a write that found nothing to do and left the buffer alone
    with pytest.raises(PhonicError):
        g.sampler_output_state(r.s)
    more = np.zeros(2 * 6000, F32)
    g.write(more, 2 * MF + 700)             # across frame 5000: the queued event finds no sampler
    assert not more.any() and g.device_errors() == 0


@pytest.mark.parametrize("kind", ["file", "granular"])
def test_7_a_start_time_inside_a_later_write(kind):
    mf = MF if kind == "file" else GMF
    g = Graph(SR, 2, mf, 0)
    r = _stage_rig(kind, g, start_time=1500, volume=0.5, panning=-0.4)
    r.on(200, 60)                           # held: it acts at the start time
    r.out_volume(300, 0.9)                  # held too: the ramp's first step is frame 1500
    r.on(1800, 64, 0.7, 0.3)
    got = _run_stage(kind, g, r, [1000, 1000, 500])
    assert r.m.write_log[0][:2] == (1500, 300) and r.m.out.log[0][0] == 1500
    assert not got[:2 * 1500].any() and got[2 * 1500:].any()
    _stage_check(kind, r, got, 2500)
