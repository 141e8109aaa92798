"""tests/sampler_model.py pinned with hand-derived cases taken straight from Sampler::next_free_voice_index (reference
src/generator/sampler.rs:826-860), SamplerVoice::stop / reset (sampler/voice.rs:196-236) and the end of SamplerVoice::process (:488-502).
No GPU, no library: the model is plain Python."""
import pytest

import sampler_model as M
import sampler_rig as R

SR = 48000
LONG = 200001     # frames of a buffer that does not end inside these cases
ENV = dict(attack_s=0.01, hold_s=0.5, decay_s=0.5, sustain_level=0.75, release_s=1.0)   # the release outlasts every case: 48000 frames


def _slots(st):
    return [s["note_id"] for s in st["slots"]]


def test_first_free_slot():
    m = M.SamplerModel(SR, LONG, 2, SR, voice_count=3)
    ids = [m.note_on(60, t=t) for t in (0, 100, 200)]
    st = m.write(1024)
    assert ids == [1, 2, 3]
    assert _slots(st) == ids                                     # slots 0, 1, 2 in the order of the notes
    assert [m.notes[i].start for i in ids] == [0, 100, 200]
    assert [m.notes[i].slot for i in ids] == [0, 1, 2]
    assert st["active_voices"] == 3 and all(s["envelope_stage"] == -1 and s["release_start_frame"] is None for s in st["slots"])


def test_a_fresh_slot_reports_the_constructor_values():
    st = M.SamplerModel(SR, LONG, 2, SR, voice_count=2, envelope=ENV).state()
    assert [(s["note_id"], s["note"], float(s["note_volume"]), float(s["note_panning"]), s["envelope_stage"]) for s in st["slots"]] == [(0, 60, 1.0, 0.0, 0)] * 2


def test_releasing_beats_active():
    m = M.SamplerModel(SR, LONG, 2, SR, voice_count=3, envelope=ENV)
    a, b, c = (m.note_on(60, t=t) for t in (0, 10, 20))
    m.note_off(c, t=1000)
    d = m.note_on(62, t=2000)
    st = m.write(3072)
    assert _slots(st) == [a, b, d]                               # slot 2 was the only one in Release; the oldest id (slot 0) stays
    assert m.notes[c].stolen and m.notes[c].end == 2000 and m.notes[d].slot == 2


def test_earliest_release_wins():
    m = M.SamplerModel(SR, LONG, 2, SR, voice_count=3, envelope=ENV)
    a, b, c = (m.note_on(60, t=t) for t in (0, 10, 20))
    m.note_off(b, t=1000)
    m.note_off(a, t=1500)
    d = m.note_on(62, t=2000)
    st = m.write(3072)
    assert _slots(st) == [a, d, c]                               # b released first (1000 < 1500): not the oldest id
    assert st["slots"][0]["release_start_frame"] == 1500 and st["slots"][1]["release_start_frame"] is None and st["slots"][0]["envelope_stage"] == 5


def test_second_all_notes_off_moves_the_release_start():
    def run(second):
        m = M.SamplerModel(SR, LONG, 2, SR, voice_count=3, envelope=ENV)
        a, b, c = (m.note_on(60, t=t) for t in (0, 10, 20))
        m.all_notes_off(t=600)                                   # a, b, c release from 600
        m.note_off(a, t=800)                                     # a again: its release start moves to 800 (voice.rs:202 runs for a releasing voice too)
        if second:
            m.all_notes_off(t=1000)                              # all three move to 1000
        d = m.note_on(62, t=2000)
        return m, m.write(3072), (a, b, c, d)

    m, st, (a, b, c, d) = run(False)
    assert _slots(st) == [a, d, c]                               # b and c tie at 600 < 800: the strict `<` keeps the first, slot 1
    assert [s["release_start_frame"] for s in st["slots"]] == [800, None, 600]
    m, st, (a, b, c, d) = run(True)
    assert _slots(st) == [d, b, c]                               # all tie at 1000: slot 0
    assert [s["release_start_frame"] for s in st["slots"]] == [None, 1000, 1000]
    assert m.notes[a].stolen and m.notes[a].end == 2000


def test_fading_voice_without_envelope_is_stolen_by_note_id():
    m = M.SamplerModel(SR, LONG, 2, SR, voice_count=2)
    a, b = m.note_on(60, t=0), m.note_on(60, t=10)
    m.note_off(b, t=500)                                         # b fades for 50 ms = 2400 frames: still active at 1000
    c = m.note_on(62, t=1000)
    st = m.write(2048)
    assert _slots(st) == [c, b]                                  # a, the lowest id, goes: a fading voice is not "releasing"
    assert m.notes[a].stolen and m.notes[a].end == 1000 and m.notes[b].stop_frames == [500]
    assert st["slots"][1]["release_start_frame"] == 500


def test_slot_frees_in_the_write_that_exhausts_it():
    m = M.SamplerModel(SR, 6001, 2, SR, voice_count=1)           # at speed 1 the file's 6001 frames end inside the sixth write: 5120 < 6001 <= 6144
    a = m.note_on(60, t=0)
    states = [m.write(1024) for _ in range(6)]
    assert [_slots(s) for s in states] == [[a]] * 5 + [[0]]
    assert not m.notes[a].stolen and m.notes[a].end == 6144
    b = m.note_on(60, t=6144)
    assert _slots(m.write(1024)) == [b] and m.notes[b].slot == 0 and not m.notes[a].stolen


# ---- a 64-slot pool: next_free_voice_index (sampler.rs:826-860) where the winner lies beyond slot 31 ----
def _full_pool(n=64, envelope=ENV, frames=LONG, notes=None):
    m = M.SamplerModel(SR, frames, 2, SR, voice_count=n, envelope=envelope)
    ids = [m.note_on(60 if notes is None else notes[i], t=i) for i in range(n)]    # slot i gets id i + 1 at frame i
    return m, ids


def test_pool64_first_free_slot_at_47():
    m, ids = _full_pool(envelope=None, frames=6001, notes=[72 if i == 47 else 60 for i in range(64)])
    st = m.write(4096)
    # slot 47 plays at speed 2: 6001 source frames are 3001 output frames from frame 47, over inside this write (one chunk of the mixer from
    # the last message, frame 63, to 4096: freed behind it); the others last to 6001 + i
    assert [i for i, s in enumerate(st["slots"]) if s["note_id"] == 0] == [47] and m.notes[ids[47]].end == 4096
    a = m.note_on(60, t=4200)
    st = m.write(1024)
    assert m.notes[a].slot == 47 and m.notes[a].stole is None and st["active_voices"] == 64


def test_pool64_earliest_release_in_slot_40_against_slot_3():
    m, ids = _full_pool()
    m.note_off(ids[40], t=2000)
    m.note_off(ids[3], t=2001)
    a, b = m.note_on(62, t=2100), m.note_on(62, t=2200)
    m.write(3072)
    assert (m.notes[a].slot, m.notes[b].slot) == (40, 3)          # 2000 < 2001: the release start decides, not the slot and not the id
    assert m.notes[ids[40]].stolen_releasing and m.notes[ids[40]].end == 2100 and m.notes[ids[3]].end == 2200


def test_pool64_equal_release_frames_in_35_and_50_give_35():
    m, ids = _full_pool()
    m.note_off(ids[50], t=2000)
    m.note_off(ids[35], t=2000)
    a, b = m.note_on(62, t=2100), m.note_on(62, t=2200)
    m.write(3072)
    assert (m.notes[a].slot, m.notes[b].slot) == (35, 50)         # the strict `<` keeps the first of equals (sampler.rs:843-849)


def test_pool64_lowest_note_id_in_slot_33():
    m, ids = _full_pool(envelope=None)
    again = [m.note_on(62, t=1000 + 10 * j) for j in range(33)]   # each takes the lowest id: slots 0..32 in turn
    a = m.note_on(64, t=2000)
    m.write(3072)
    assert [m.notes[i].slot for i in again] == list(range(33))
    assert m.notes[a].slot == 33 and m.notes[a].stole == ids[33] == 34


# ---- start_time: the mixer does not call a source before it (mixed.rs:565-576) and a TriggerGeneratorEvent that comes due earlier only goes
# into the generator's queue (mixed.rs:902-918); the sampler drains the queue at the top of its first write (sampler.rs:656-731) ----
def _start_time_script(m, order):
    sent = {}
    for k in order:
        if k == "on100":
            sent[k] = m.note_on(60, 0.8, 0.0, t=100)
        elif k == "vol200":
            m.set_parameter("volume", M.F32(0.5), t=200)
        elif k == "off300":
            m.note_off(999999, t=300)
        else:
            sent[k] = m.note_on(64, 1.0, 0.0, t=1500)
    return sent["on100"], sent["on1500"]


def test_start_time_holds_earlier_messages_until_the_first_write():
    for order in (("on100", "vol200", "off300", "on1500"), ("on1500", "vol200", "off300", "on100")):
        m = M.SamplerModel(SR, LONG, 2, SR, voice_count=3, envelope=ENV, start_time=1500)
        a, b = _start_time_script(m, order)
        st = m.write(1024)
        assert _slots(st) == [0, 0, 0] and float(st["volume"]) == 1.0 and not m.notes          # nothing was applied: the messages wait
        st = m.write(1024)
        # the mixer's first call of the sampler begins at its start time, inside the chunk (mixed.rs:574-582): everything applies at 1500, by
        # sample time and then by sending order — the note of frame 100 first, with the base volume still 1.0
        assert _slots(st) == [a, b, 0] and float(st["volume"]) == 0.5
        assert (m.notes[a].start, m.notes[b].start) == (1500, 1500)
        assert m.notes[a].volume_events == [(1500, M.F32(0.8)), (1500, M.F32(M.F32(0.5) * M.F32(0.8)))]
        assert m.notes[b].volume_events == [(1500, M.F32(0.5))]
        assert len(m.notes[a].gains) == len(m.notes[b].gains) == 2048 - 1500


def test_start_time_equal_sample_times_keep_the_sending_order():
    m = M.SamplerModel(SR, LONG, 2, SR, voice_count=2, start_time=1024)
    m.set_parameter("volume", M.F32(0.5), t=100)
    a = m.note_on(60, 1.0, 0.0, t=100)
    assert _slots(m.write(1024)) == [0, 0]
    st = m.write(1024)                                             # a start time on a piece boundary: the second write is the first one
    assert _slots(st) == [a, 0] and m.notes[a].start == 1024 and m.notes[a].volume_events == [(1024, M.F32(0.5))]


def test_start_time_in_the_past_changes_nothing():
    def run(**kw):
        m = M.SamplerModel(SR, LONG, 2, SR, voice_count=2, **kw)
        a = m.note_on(60, t=100)
        m.write(1024, 2048)
        return m.notes[a].start
    assert run() == run(start_time=2048) == run(start_time=7) == 2048   # a late message applies at the write's first frame


# ---- extra_cuts: the owning mixer cuts its chunk at ALL of its events (mixed.rs:679-712); the sampler's write ends there ----
def test_extra_cuts_end_the_write_that_exhausts_a_slot():
    def end_of_note(cuts):
        m = M.SamplerModel(SR, 6001, 2, SR, voice_count=1, extra_cuts=cuts)
        a = m.note_on(60, t=0)
        for _ in range(6):
            m.write(1024)
        return m.notes[a].end
    assert end_of_note(()) == 6144                                 # the file's 6001 frames end inside the sixth piece: freed behind it
    assert end_of_note((6050,)) == 6050                            # another source's event at 6050: the write that exhausts the slot ends there
    assert end_of_note((5990,)) == 6144                            # a cut in front of the end: the next write, 5990..6144, exhausts it
    assert end_of_note((6001, 6100)) == 6001                       # the write 5120..6001 consumes the file's last frame: end of file in that write (preloaded.rs:270-332)
    assert end_of_note((0, 5120, 99999)) == 6144                   # cuts on chunk borders and beyond the writes change nothing


def test_extra_cuts_move_the_fade_out_arrival():
    def run(cuts):
        m = M.SamplerModel(SR, LONG, 2, SR, voice_count=1, extra_cuts=cuts)
        a = m.note_on(60, t=0)
        m.note_off(a, t=100)                                       # the 50 ms fade-out: its arrival is tested behind every write (fader.rs:118-121)
        for _ in range(5):
            m.write(1024)
        return m.notes[a].end
    # the fader's value after k frames is exp(-4.605 k / 2400) (fader.rs:67-91): below 1e-4 from k = 2400 * ln(1e4) / 4.605 = 4800.2 on, frame 4901
    assert run(()) == 5120                                         # found behind the fifth piece
    assert run((4920,)) == 4920                                    # a write that ends at 4920 finds it arrived: the slot is free from there
    assert run((4880,)) == 5120                                    # one that ends at 4880 does not


# ---- the random scripts of the large pools (tests/test_gpu_sampler_pools.py, group B) against the model alone: what they must contain ----
@pytest.mark.parametrize("voice_count,envelope,seed", R.POOL_CASES)
def test_pool_scripts_contain_what_the_gpu_cases_need(voice_count, envelope, seed):
    r = R.ModelRig(R.LONG.size // 2, voice_count, envelope=R.ENV if envelope else None)
    R.pool_script(r, R.pool_rng(voice_count, envelope, seed), R.POOL_PIECES * R.MF, R.POOL_MESSAGES)
    for _ in range(R.POOL_PIECES):
        r.m.write(R.MF)
    R.assert_pool_script_conditions(r.m, envelope)
