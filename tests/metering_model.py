"""AudioLevelState::record (reference src/source/metered.rs:75-143) and the interval conversion (src/utils/time.rs:28-35), restated in numpy:
sequential f64 sums in the reference's order. The reference has no known-answer test for the meter, so tests/test_metering_model.py pins
this model against analytic answers; the GPU tests then compare the device against it."""
import numpy as np


def interval_frames(seconds, sample_rate):
    """(interval.as_secs_f64() * sample_rate as f64) as u64: truncated, saturating."""
    f = float(seconds) * float(sample_rate)
    return 2**64 - 1 if f >= 2.0**64 else int(f)


class AudioLevelState:
    def __init__(self, interval_seconds, sample_rate, channels=2):
        self.channels = channels
        self.update_interval = interval_frames(interval_seconds, sample_rate)
        self.peak_hold = np.zeros(channels, dtype=np.float32)
        self.sum_square = np.zeros(channels, dtype=np.float64)
        self.collected_frames = 0
        self.clock_start = 0                                  # SampleTimeClock::start_time
        self.peak = np.zeros(channels, dtype=np.float32)      # AudioLevel
        self.rms = np.zeros(channels, dtype=np.float32)
        self.publishes = 0

    def level(self):
        return (float(self.peak[0]), float(self.peak[1])), (float(self.rms[0]), float(self.rms[1]))

    def record(self, output, pos_in_frames):
        """One write call of the wrapped mixer that returned `output` (interleaved f32) and began at pos_in_frames. Returns True when it published."""
        output = np.asarray(output, dtype=np.float32).reshape(-1)
        if self.channels == 0 or output.size == 0:
            return False
        frames = output.reshape(-1, self.channels)
        for ch in range(self.channels):
            x = frames[:, ch]
            a = np.abs(x)
            a = a[~np.isnan(a)]                                # `if abs_sample > peak_hold`: a compare, a NaN never enters
            if a.size and a.max() > self.peak_hold[ch]:
                self.peak_hold[ch] = a.max()
            x64 = x.astype(np.float64)
            # sequential, in frame order, from the running sum (np.cumsum accumulates left to right; np.sum would add pairwise)
            self.sum_square[ch] = np.cumsum(np.concatenate([self.sum_square[ch : ch + 1], x64 * x64]))[-1]
        self.collected_frames += frames.shape[0]
        elapsed = max(0, int(pos_in_frames) - self.clock_start)   # saturating_sub
        if elapsed < self.update_interval:
            return False
        for ch in range(self.channels):
            self.peak[ch] = self.peak_hold[ch]
            self.rms[ch] = np.float32(np.sqrt(self.sum_square[ch] / np.float64(self.collected_frames))) if self.collected_frames > 0 else np.float32(0.0)
        self.clock_start = int(pos_in_frames)
        self.collected_frames = 0
        self.peak_hold[:] = 0.0
        self.sum_square[:] = 0.0
        self.publishes += 1
        return True


def ulp_distance(a, b):
    """Distance of two non-negative finite f32 values in units in the last place."""
    ia = int(np.float32(a).view(np.uint32))
    ib = int(np.float32(b).view(np.uint32))
    return abs(ia - ib)
