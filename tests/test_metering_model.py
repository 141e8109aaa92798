"""tests/metering_model.py against analytic answers (the reference's AudioLevelState has no known-answer test of its own)."""
import math

import numpy as np

from metering_model import AudioLevelState, interval_frames, ulp_distance

SR = 48000


def stereo(l, r=None):
    l = np.asarray(l, dtype=np.float32)
    r = l if r is None else np.asarray(r, dtype=np.float32)
    return np.stack([l, r], axis=1).reshape(-1)


def test_constant_gives_peak_equal_rms():
    a = np.float32(0.3125)
    st = AudioLevelState(0.0, SR)
    assert st.record(stereo(np.full(500, a), np.full(500, -a)), 0)
    assert st.level() == ((float(a), float(a)), (float(a), float(a)))


def test_full_scale_square_wave():
    x = np.where(np.arange(960) % 48 < 24, 1.0, -1.0)
    st = AudioLevelState(0.0, SR)
    st.record(stereo(x), 0)
    assert st.level() == ((1.0, 1.0), (1.0, 1.0))


def test_whole_periods_of_a_sine():
    a, n, periods = 0.5, 4800, 100
    x64 = a * np.sin(2.0 * np.pi * periods * np.arange(n) / n)
    x = x64.astype(np.float32)
    st = AudioLevelState(0.0, SR)
    st.record(stereo(x), 0)
    exact = math.sqrt(float(np.sum(x.astype(np.float64) ** 2)) / n)      # of the f32 samples themselves
    assert ulp_distance(st.rms[0], np.float32(exact)) <= 1
    assert abs(float(st.rms[0]) - a / math.sqrt(2.0)) < 1e-7              # f32 rounding of the samples and of the result
    assert st.peak[0] == np.abs(x).max()


def test_nan_is_ignored_by_the_peak():
    x = np.array([0.25, np.nan, -0.5, 0.125], dtype=np.float32)
    st = AudioLevelState(0.0, SR)
    st.record(stereo(x), 0)
    assert st.peak[0] == np.float32(0.5) and st.peak[1] == np.float32(0.5)
    assert math.isnan(st.rms[0])   # the sum of squares does take it, as in the reference


def test_interval_is_truncated():
    assert interval_frames(0.0249999, SR) == 1199
    assert interval_frames(0.025, SR) == 1200
    assert interval_frames(0.0, SR) == 0
    assert interval_frames(1e30, SR) == 2**64 - 1


def test_publish_at_the_first_record_whose_start_reaches_the_interval():
    st = AudioLevelState(0.025, SR)   # 1200 frames
    rng = np.random.default_rng(1)
    published = []
    for i in range(6):
        x = rng.uniform(-1, 1, 512 * 2).astype(np.float32)
        published.append(st.record(x, i * 512))
    # starts 0, 512, 1024 < 1200; 1536 >= 1200 publishes and moves the clock to 1536; 2048 - 1536 and 2560 - 1536 < 1200
    assert published == [False, False, False, True, False, False]
    assert st.clock_start == 1536


def test_interval_zero_publishes_every_record_and_resets():
    st = AudioLevelState(0.0, SR)
    assert st.record(stereo(np.full(10, 0.5)), 0)
    assert st.level() == ((0.5, 0.5), (0.5, 0.5))
    assert st.collected_frames == 0 and not st.peak_hold.any() and not st.sum_square.any()
    assert st.record(stereo(np.full(10, 0.25)), 10)
    assert st.level() == ((0.25, 0.25), (0.25, 0.25))     # nothing of the first record is left


def test_accumulation_across_records_until_publish():
    st = AudioLevelState(0.025, SR)
    st.record(stereo(np.full(600, 1.0)), 0)
    assert st.level() == ((0.0, 0.0), (0.0, 0.0))
    st.record(stereo(np.full(600, 0.0)), 600)
    assert st.level() == ((0.0, 0.0), (0.0, 0.0))
    assert st.record(stereo(np.full(600, 0.0)), 1200)
    assert st.peak[0] == 1.0 and ulp_distance(st.rms[0], np.float32(math.sqrt(1.0 / 3.0))) <= 1


def test_zero_length_record_is_a_no_op():
    st = AudioLevelState(0.0, SR)
    st.record(stereo(np.full(10, 0.5)), 0)
    before = (st.level(), st.clock_start, st.publishes)
    assert not st.record(np.zeros(0, dtype=np.float32), 5000)
    assert (st.level(), st.clock_start, st.publishes) == before
