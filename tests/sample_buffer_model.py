"""A numpy model of Sampler::create_granular_sample_buffer (reference src/generator/sampler.rs:908-952): the mono buffer at the graph's rate that
a sampler's grain pool reads. A mono file at the graph's rate is its own granular buffer (:912-914); anything else goes through a temporary
PreloadedFileSource — the graph's rate, default options, repeat(0), the cubic resampler — pulled in writes of exactly 1024 frames until one
returns 0 (:932-945), each frame mixed down as _capi.mono_downmix does (:940-943); a single 0.0 if nothing came (:946-949).

Built on FileSource of tests/golden/numpy_restatement_graph.py, the restatement of PreloadedFileSource::write that tests/test_golden.py holds
against the C++ oracle. The 1024-frame writes matter: a source that reaches the end of its file in a write is finished after that write, so
the outputs the interpolator could still deliver without a new input frame appear only if that write has room for them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import numpy_restatement_graph as RG  # noqa: E402

from phonic_amd import _capi  # noqa: E402

F = np.float32
WRITE_FRAMES = 1024   # sampler.rs:932

# (channels, file rate, graph rate, frames in — with the decoder's zero frame —, frames out): the cases of the conversion, one per path of the
# resampler (bypass; ratio in [0.5, 1), at or above 1, below 0.5; a buffer too short to initialise the interpolator; the end of file on a write's
# last frame)
CASES = [
    (2, 48000, 48000, 701, 701),
    (2, 44100, 48000, 2301, 2503),
    (1, 96000, 48000, 4101, 2049),
    (2, 32000, 48000, 3, 2),
    (1, 44100, 48000, 2, 4),
    (2, 88200, 44100, 2051, 1024),
    (1, 22050, 48000, 1501, 3264),
    (2, 48000, 44100, 2501, 2295),
]


def make_pcm(channels, n_frames, seed=0):
    """Deterministic interleaved PCM in [-1, 1) whose last frame is the zero frame symphonia's decoding appends."""
    rng = np.random.default_rng(1000 * channels + n_frames + seed)
    t = np.arange(n_frames, dtype=np.float64)
    pcm = np.zeros((n_frames, channels), F)
    for c in range(channels):
        pcm[:, c] = (0.6 * np.sin(0.031 * (c + 1) * t + c) + 0.3 * rng.uniform(-1.0, 1.0, n_frames)).astype(F)
    pcm[-1, :] = 0.0
    return pcm.reshape(-1)


def granular_sample_buffer(pcm, channels, file_rate, graph_rate):
    pcm = np.ascontiguousarray(pcm, dtype=F).reshape(-1)
    if channels == 1 and file_rate == graph_rate:
        return pcm.copy()
    src = RG.FileSource(pcm, channels, file_rate, graph_rate, repeat=0)
    parts = []
    while True:
        out = np.zeros(WRITE_FRAMES * channels, F)
        n = src.write(out)
        if n == 0:
            break
        parts.append(_capi.mono_downmix(out[:n], channels))
    if not parts:
        return np.zeros(1, F)
    return np.concatenate(parts)


_CACHE = {}


def case_buffers(case):
    """(pcm, model output) of a row of CASES — computed once, shared by the tests that need it, never modified (the arrays are read-only)."""
    if case not in _CACHE:
        ch, fr, gr, n_in, _ = case
        pcm = make_pcm(ch, n_in)
        mono = granular_sample_buffer(pcm, ch, fr, gr)
        pcm.setflags(write=False)
        mono.setflags(write=False)
        _CACHE[case] = (pcm, mono)
    return _CACHE[case]
