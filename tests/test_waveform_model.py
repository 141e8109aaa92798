"""tests/waveform_model.py — the numpy model of waveform::mixed_down / multi_channel (reference src/utils/waveform.rs) — pinned on the CPU: the
claims of the reference's own test (waveform.rs:207-254), the branch edge, ramps whose every bucket shows its two ends, and the shapes at which
the reference's f32 bucket boundaries differ from exact integer ones — the shapes that let tests/test_gpu_waveform.py catch integer or f64
boundary arithmetic in the kernels. A scalar loop written from the same lines of the reference is the second opinion on small inputs."""
import numpy as np
import pytest

import waveform_model as W

F = np.float32


def _noise(n, ch, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n * ch).astype(F)


def _scalar_mixed_down(pcm, ch, rate, res):
    """waveform.rs:95-140, one frame at a time (min / max as f32::min / f32::max: a NaN operand is ignored)."""
    fr = np.asarray(pcm, F).reshape(-1, ch)
    n = fr.shape[0]

    def mono(f):
        acc = F(0.0)
        for x in f:
            acc = F(acc + F(x / F(ch)))
        return acc

    pts = []
    if n <= res:
        for k in range(n):
            v = mono(fr[k])
            pts.append((k, F(F(k) / F(rate)), v, v))
        return pts
    step = F(n) / F(res)
    for i in range(res):
        a, e = int(F(F(i) * step)), min(int(F(F(i + 1) * step)), n)
        mn, mx = W.F32_MAX, W.F32_MIN
        for k in range(a, e):
            v = mono(fr[k])
            mn, mx = np.fmin(mn, v), np.fmax(mx, v)
        pts.append((a, F(F(a) / F(rate)), mn, mx))
    return pts


def test_lengths_as_the_references_own_test_claims():
    long_st, short_st = _noise(5000, 2, 1), _noise(600, 2, 2)
    assert W.mixed_down(long_st, 2, 44100, 1024)["min"].shape == (1024,)            # downscale: length == resolution
    assert W.mixed_down(short_st, 2, 44100, 1024)["min"].shape == (600,)            # upscale: length == frames < resolution
    assert W.multi_channel(long_st, 2, 44100, 1024)["min"].shape == (2, 1024)
    assert W.multi_channel(short_st, 2, 44100, 1024)["min"].shape == (2, 600)


def test_frames_equal_to_the_resolution_take_the_upscale_branch():
    x = _noise(1024, 1, 3)
    w = W.mixed_down(x, 1, 48000, 1024)
    assert np.array_equal(w["min"], x) and np.array_equal(w["max"], x) and np.array_equal(w["frame"], np.arange(1024))
    assert np.array_equal(w["time"], (np.arange(1024).astype(F) / F(48000)).astype(F))
    d = W.mixed_down(_noise(1025, 1, 3), 1, 48000, 1024)   # one more frame: buckets, one of them with two frames
    assert d["min"].shape == (1024,) and int(np.count_nonzero(d["min"] != d["max"])) == 1


@pytest.mark.parametrize("n,res", [(65537, 1024), (100003, 1000), (240001, 1920), (5000, 7)])
def test_on_a_ramp_every_bucket_shows_its_first_and_last_frame(n, res):
    x = np.arange(n, dtype=F)
    w = W.mixed_down(x, 1, 48000, res)
    b = W.boundaries(n, res)
    lo, hi = np.minimum(b[:-1], n), np.minimum(b[1:], n)
    assert (hi > lo).all()
    assert np.array_equal(w["frame"], b[:-1])
    assert np.array_equal(w["min"], lo.astype(F)) and np.array_equal(w["max"], (hi - 1).astype(F))
    assert np.array_equal(w["time"], (b[:-1].astype(F) / F(48000)).astype(F))


@pytest.mark.parametrize("n,res,differ,where", [(65537, 1024, 2, None), (100003, 1000, 2, [333, 666]), (262147, 4096, 27, None), (240001, 1920, 7, None), (1000003, 4096, 83, None)])
def test_f32_boundaries_differ_from_integer_ones(n, res, differ, where):
    d = np.flatnonzero(W.boundaries(n, res) != W.integer_boundaries(n, res))
    assert d.size == differ, d
    if where is not None:
        assert d.tolist() == where


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n,res", [(37, 64), (64, 64), (65, 64), (127, 64), (1000, 7), (1003, 1)])
def test_the_vectorised_model_equals_the_scalar_loop(ch, n, res):
    pcm = _noise(n, ch, 10 * n + ch)
    pcm[3 * ch] = np.nan
    pcm[5 * ch:5 * ch + ch] = np.inf
    w = W.mixed_down(pcm, ch, 44100, res)
    pts = _scalar_mixed_down(pcm, ch, 44100, res)
    assert len(pts) == w["min"].size
    for k, key in enumerate(("frame", "time", "min", "max")):
        assert np.array_equal(np.array([p[k] for p in pts]).astype(w[key].dtype), w[key], equal_nan=True), key
    m = W.multi_channel(pcm, ch, 44100, res)
    for c in range(ch):   # a channel of multi_channel is mixed_down of that channel alone (the fold over one channel is the sample)
        one = W.mixed_down(pcm.reshape(-1, ch)[:, c].copy(), 1, 44100, res)
        for key in ("frame", "time", "min", "max"):
            assert np.array_equal(m[key][c], one[key], equal_nan=True), (c, key)


def test_special_values():
    big = np.finfo(F).max
    pcm = np.zeros((2048, 2), F)
    pcm[0] = (big, big)          # the fold divides first: the mono value stays finite
    pcm[8] = (1e-45, 1e-45)      # half the smallest denormal rounds to zero, twice
    pcm[16] = (np.nan, 0.5)
    pcm[24:32] = np.nan          # a whole bucket of NaN (resolution 256: buckets of 8 frames)
    pcm[32] = (np.inf, np.inf)
    w = W.mixed_down(pcm.reshape(-1), 2, 48000, 256)
    assert w["max"][0] == big and w["max"][1] == 0.0 and w["min"][1] == 0.0
    assert w["min"][2] == 0.0 and w["max"][2] == 0.0            # the NaN frame's mono value is NaN: skipped
    assert w["min"][3] == W.F32_MAX and w["max"][3] == W.F32_MIN
    assert w["max"][4] == np.inf and w["min"][4] == 0.0
    m = W.multi_channel(pcm.reshape(-1), 2, 48000, 256)
    assert m["max"][1][2] == 0.5 and m["max"][0][2] == 0.0 and m["max"][0][1] == F(1e-45)


def test_a_slice_counts_from_its_own_start():
    pcm = _noise(5000, 2, 9)
    w = W.waveform(pcm, 2, 44100, 100, "multi_channel", first_frame=1234, n_frames=3001)
    ref = W.multi_channel(pcm[2 * 1234:2 * (1234 + 3001)], 2, 44100, 100)
    assert w["frame"][0][0] == 0
    for key in ref:
        assert np.array_equal(w[key], ref[key])
