"""tests/sample_buffer_model.py — the numpy model of Sampler::create_granular_sample_buffer — against the second reference, the C++ oracle's graph:
a file voice with volume 1, panning 0, repeat 0 and no effects on the main mixer of a graph pulled in 1024-frame writes delivers the raw output
of the PreloadedFileSource the reference's function pulls. Mono files are compared with the left channel, stereo files with (L + R) / 2 in f32;
behind the model's length the oracle must be silent (the source is finished: nothing follows the write in which it met its end of file).
CPU only."""
import numpy as np
import pytest

import oracle
import sample_buffer_model as M

F = np.float32


def case_id(c):
    return f"{c[0]}ch-{c[1]}to{c[2]}-{c[3]}f"


@pytest.mark.parametrize("case", M.CASES, ids=case_id)
def test_model_equals_the_oracle_graph(case):
    ch, file_rate, graph_rate, n_in, n_out = case
    pcm, mono = M.case_buffers(case)
    assert pcm.size == n_in * ch
    assert mono.size == n_out, (mono.size, n_out)
    g = oracle.OracleGraph(graph_rate, 2, 1024)
    g.add_voice(0, pcm, ch, file_rate, volume=1.0, panning=0.0, has_repeat=1, repeat=0)
    blocks = n_out // 1024 + 2
    bus = g.render(blocks, 1024).reshape(-1, 2)
    g.close()
    ref = bus[:, 0] if ch == 1 else ((bus[:, 0] + bus[:, 1]).astype(F) / F(2.0)).astype(F)
    assert np.array_equal(ref[:n_out], mono)
    assert not ref[n_out:].any() and not bus[n_out:].any()


def test_mono_at_the_graph_rate_is_the_buffer_itself():
    pcm = M.make_pcm(1, 333)
    out = M.granular_sample_buffer(pcm, 1, 48000, 48000)
    assert out is not pcm and np.array_equal(out, pcm)


def test_nothing_written_gives_one_zero():
    # ratio 4: the first output needs four pushed frames behind the interpolator's three — a file of five frames delivers nothing
    out = M.granular_sample_buffer(M.make_pcm(1, 5), 1, 192000, 48000)
    assert out.size == 1 and out[0] == 0.0
