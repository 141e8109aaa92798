"""A numpy model of phonic::utils::waveform::{mixed_down, multi_channel} (reference src/utils/waveform.rs:95-199) on a slice of interleaved
f32 PCM, written from reading that file: every operation in f32, in the reference's order.

  upscale    (frames <= resolution) one point per frame, min == max == the frame's value (:105-116, :159-170);
  downscale  step = frames as f32 / resolution as f32 (:119); bucket i covers frames [b(i), b(i + 1)) with
             b(i) = min((i as f32 * step) as usize, frames) (:123-127): one rounded f32 product, truncated. The point's frame is b(i) BEFORE the
             clamp, its time b(i) as f32 / rate as f32 (:135) — the argument of Duration::from_secs_f32, which the model (like the C ABI) leaves
             as the f32. A bucket without frames keeps f32::MAX / f32::MIN (:121-122);
  mono value fold(0.0, |acc, x| acc + x / channels as f32) in channel order (:107-109): each sample is divided first;
  min / max  f32::min / f32::max (:132-133, :184-185) ignore a NaN operand: np.fmin / np.fmax, seeded with f32::MAX / f32::MIN.

Vectorised: np.fmin.reduceat / np.fmax.reduceat over the non-empty buckets. Both functions return a dict of frame (uint64), time, min, max
(float32): shape (P,) for mixed_down, (channels, P) for multi_channel."""
import numpy as np

F = np.float32
F32_MAX = np.finfo(np.float32).max
F32_MIN = np.finfo(np.float32).min   # Rust's f32::MIN: the most negative finite value


def boundaries(n_frames, resolution):
    """b(0) .. b(resolution) before the clamp, as uint64: (i as f32 * step) as usize."""
    step = F(n_frames) / F(resolution)
    i = np.arange(resolution + 1, dtype=np.uint64).astype(F)
    return (i * step).astype(F).astype(np.uint64)


def integer_boundaries(n_frames, resolution):
    """What exact integer arithmetic would give: i * n // resolution. NOT the reference's boundaries; tests count where the two differ."""
    return np.array([i * n_frames // resolution for i in range(resolution + 1)], dtype=np.uint64)


def mono_values(frames):
    """frames: (n, channels) f32 -> the fold of :107-109 per frame."""
    ch = frames.shape[1]
    with np.errstate(all="ignore"):
        acc = np.zeros(frames.shape[0], F)
        for c in range(ch):
            acc = (acc + (frames[:, c] / F(ch)).astype(F)).astype(F)
    return acc


def _points(values, rate, resolution):
    """values: (n,) f32 — one display row."""
    n = values.shape[0]
    with np.errstate(all="ignore"):
        if n <= resolution:
            frame = np.arange(n, dtype=np.uint64)
            return frame, (frame.astype(F) / F(rate)).astype(F), values.copy(), values.copy()
        b = boundaries(n, resolution)
        frame = b[:-1].copy()
        time = (frame.astype(F) / F(rate)).astype(F)
        lo, hi = np.minimum(b[:-1], n).astype(np.int64), np.minimum(b[1:], n).astype(np.int64)
        mn, mx = np.full(resolution, F32_MAX, F), np.full(resolution, F32_MIN, F)
        full = np.flatnonzero(hi > lo)
        if full.size:
            # reduceat over [lo0, hi0, lo1, hi1, ...]: the even results are the buckets, the odd ones the gaps between them (none, as b is monotone)
            idx = np.stack([lo[full], hi[full]], axis=1).reshape(-1)
            padded = np.concatenate([values, np.zeros(1, F)])   # an index == n must be valid for reduceat
            mn[full] = np.fmin(np.fmin.reduceat(padded, idx)[0::2], F32_MAX)
            mx[full] = np.fmax(np.fmax.reduceat(padded, idx)[0::2], F32_MIN)
        return frame, time, mn, mx


def mixed_down(pcm, channels, rate, resolution):
    frames = np.ascontiguousarray(pcm, dtype=F).reshape(-1, channels)
    frame, time, mn, mx = _points(mono_values(frames), rate, resolution)
    return dict(frame=frame, time=time, min=mn, max=mx)


def multi_channel(pcm, channels, rate, resolution):
    frames = np.ascontiguousarray(pcm, dtype=F).reshape(-1, channels)
    rows = [_points(np.ascontiguousarray(frames[:, c]), rate, resolution) for c in range(channels)]
    return {k: np.stack([r[j] for r in rows]) for j, k in enumerate(("frame", "time", "min", "max"))}


def waveform(pcm, channels, rate, resolution, mode="mixed_down", first_frame=0, n_frames=None):
    """The model on frames [first_frame, first_frame + n_frames) — the `&buffer[a * ch .. b * ch]` a caller of the reference passes."""
    frames = np.ascontiguousarray(pcm, dtype=F).reshape(-1, channels)
    end = frames.shape[0] if n_frames is None else first_frame + n_frames
    part = frames[first_frame:end]
    return (mixed_down if mode == "mixed_down" else multi_channel)(part, channels, rate, resolution)
