"""tests/sampler_model.py pinned with hand-derived cases taken straight from Sampler::next_free_voice_index (reference
src/generator/sampler.rs:826-860), SamplerVoice::stop / reset (sampler/voice.rs:196-236) and the end of SamplerVoice::process (:488-502).
No GPU, no library: the model is plain Python."""
import sampler_model as M

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
