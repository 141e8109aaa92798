"""The host side of pg_graph_sample_buffer_waveform under AddressSanitizer + UndefinedBehaviorSanitizer + LeakSanitizer, without a GPU: the
library's translation units compiled host-only against the stub HIP runtime (tests/host_build.py) and linked with the stand-alone program
tests/host/waveform_host.cpp — a plain executable with its own main, nothing preloaded, no Python inside. It walks mono and stereo buffers, both
modes and sources, every grid, sub-slices, repeated calls between writes while voices play the buffer, release and destroy, and checks the
returned counts and error codes (the stub launches nothing, so the values are zeros and not checked) and that the allocation counters balance."""
import os
import subprocess

import host_build


def test_waveform_host_side_under_asan_and_ubsan(tmp_path):
    exe = host_build.build_host_program(tmp_path, "waveform_host")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **host_build.SANITIZER_ENV))
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-1000:], run.stderr[-4000:])
