"""What the GPU scripts of tests/test_gpu_main_sampler.py discriminate, decided on the model alone (tests/main_sampler_model.py): the two write
grids end a granular slot's write at different frames, a volume ramp steps per interleaved sample, and a ramp stands still while the sampler
returns nothing. The scripts themselves live here so that the GPU tests run the very same ones."""
import numpy as np

import granular_sampler_rig as GR
import main_sampler_model as MM
import sampler_rig as FR

SR = 48000
F32 = np.float32
# the release ends ~3497 frames behind the note-off at frame 1000: Idle between frames 4096 and 5096
GRID_ENV = dict(attack_s=0.0, hold_s=0.0, decay_s=0.0, sustain_level=1.0, release_s=3500.0 / SR)
GRID_SIZES = (6000, 1000)


def grid_script(r):
    """(a) One slot's note, released by the message at frame 1000 of a 6000-frame write; a later note in the same slot. `r`: anything with
    on(t, note) -> k and off(t, k) that sends in this order (a rig, or _ModelCalls below)."""
    a = r.on(0, 60)
    r.off(1000, a)
    r.on(6000, 64)


class _ModelCalls:
    def __init__(self, m):
        self.m, self.ids = m, []

    def on(self, t, note, volume=1.0, panning=0.0):
        self.ids.append(self.m.note_on(note, volume, panning, t))
        return len(self.ids) - 1

    def off(self, t, k):
        self.m.note_off(self.ids[k], t)


def _granular(grid, **kw):
    return MM.MainGranularSamplerModel(SR, GR.BUF, GR.model_params(GR.SHORT), voice_count=2, envelope=GRID_ENV, grid=grid, **kw)


def test_a_the_two_grids_end_the_released_slots_write_at_different_frames():
    got = {}
    for grid in ("main", "sub"):
        m = _granular(grid)
        grid_script(_ModelCalls(m))
        audio = [m.write(n) for n in GRID_SIZES]
        got[grid] = (m, audio)
    main, sub = got["main"][0], got["sub"][0]
    # the message at frame 1000 begins a chunk of the main mixer: 4096 frames from THERE; the sub-mixer's parent keeps its chunk of 4096 from 0
    assert main.span_log[:3] == [(0, 1000), (1000, 4096), (5096, 904)]
    assert sub.span_log[:3] == [(0, 1000), (1000, 3096), (4096, 1904)]
    # the envelope is Idle inside (4096, 5096): the slot is freed — and its scheduler stops drawing — at 5096 here, at 6000 there
    assert [a[2] for a in main.allocations] == [0, 0] and [a[2] for a in sub.allocations] == [0, 0]
    assert np.array_equal(got["main"][1][0], got["sub"][1][0])        # the first note sounds the same: it is silent behind Idle
    assert main.grain_state(0)["rng"] != sub.grain_state(0)["rng"]    # the slot's generator drew a different number of times ...
    assert not np.array_equal(got["main"][1][1], got["sub"][1][1])    # ... and the later note in that slot plays other grains


def test_a_file_pool_is_written_on_the_main_grid():
    """The file model on the main grid: the message at frame 1000 begins a chunk of 4096 frames. (A file slot is freed at the end of the write
    that holds its end, and the next message ends that write on either grid: which slot a note gets does not depend on the grid — what
    differs is what the read-backs show between two messages, and where a granular slot's generator stops, above.)"""
    m = MM.MainSamplerModel(SR, FR._frames(FR.SHORT), 2, SR, voice_count=1)
    a = m.note_on(64, 1.0, 0.0, 0)            # four semitones up: the 6001 frames end near frame 4763
    m.set_note_volume(a, 0.5, 1000)
    m.write(6000, 0)
    assert m.write_log == [(0, 1000, True), (1000, 4096, True), (5096, 904, False)]   # the last write finds no active slot: it returns nothing
    assert m.notes[a].end == 5096


def test_b_a_volume_ramp_steps_per_interleaved_sample():
    o = MM.OutputStage(SR, volume=1.0)
    o.message("volume", 0.25)
    o.write(0, 64)
    gains = o.log[0][2]
    assert isinstance(gains, np.ndarray) and gains.shape == (128,)
    assert (np.diff(gains) < 0).all()                      # every SAMPLE takes a step: left and right of one frame differ
    assert gains[0] != gains[1]
    x = np.ones((64, 2), F32)
    y = o.apply(x)
    assert (y[:, 0] != y[:, 1]).all()                      # per-frame stepping would give both channels of a frame one gain
    # the panning steps per FRAME
    p = MM.OutputStage(SR, panning=0.0)
    p.message("panning", 0.8)
    p.write(0, 64)
    left, right = p.log[0][3]
    assert left.shape == (64,) and (np.diff(left) < 0).all() and (np.diff(right) > 0).all()


def ramp_stands_still_script(r):
    """(c) set_volume at frame 100 with no note sounding; the first note at frame 3000. `r`: on / out_volume."""
    r.out_volume(100, 0.25)
    r.on(3000, 60)


def test_c_a_ramp_waits_for_the_next_note():
    class Calls(_ModelCalls):
        def out_volume(self, t, v):
            self.m.set_volume(v, t)

    m = MM.MainSamplerModel(SR, FR._frames(FR.LONG), 2, SR, voice_count=2)
    ramp_stands_still_script(Calls(m))
    m.write(2000, 0)
    st = m.output_state()
    assert st["volume_target"] == F32(0.25) and st["volume_current"] == F32(1.0) and st["volume_ramping"]   # set at the message, not moved since
    assert [w[2] for w in m.write_log] == [False, False]     # [0, 100) and [100, 2000): the sampler returned nothing
    m.write(2000, 2000)
    assert m.out.log[0][0] == 3000                           # the ramp's first step is the note's first sample
    first = m.out.log[0][2][0]
    assert F32(0.99) < first < F32(1.0)
    assert m.output_state()["volume_current"] < F32(0.5)


def test_two_messages_on_one_frame_the_last_one_sent_counts():
    for order in ((0.5, 0.25), (0.25, 0.5)):
        m = MM.MainSamplerModel(SR, FR._frames(FR.LONG), 2, SR, voice_count=1)
        m.note_on(60, 1.0, 0.0, 0)
        for v in order:
            m.set_volume(v, 500)
        m.write(1000, 0)
        assert m.output_state()["volume_target"] == F32(order[1])


def test_skip_branches_leave_the_samples_alone():
    o = MM.OutputStage(SR, volume=1.0 + 5e-7, panning=5e-7)
    o.write(0, 8)
    assert o.log[0][2] is None and o.log[0][3] is None
    o = MM.OutputStage(SR, volume=1.0 + 5e-6, panning=5e-6)
    o.write(0, 8)
    assert o.log[0][2] is not None and o.log[0][3] is not None


def test_a_held_message_acts_at_the_start_time():
    m = MM.MainSamplerModel(SR, FR._frames(FR.LONG), 2, SR, voice_count=2, start_time=1500)
    m.note_on(60, 1.0, 0.0, 200)
    m.set_volume(0.5, 300)
    m.write(3000, 0)
    assert m.notes[1].start == 1500
    assert m.write_log == [(1500, 1500, True)]
    assert m.out.log[0][0] == 1500 and isinstance(m.out.log[0][2], np.ndarray)
