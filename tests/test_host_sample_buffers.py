"""The host side of the sample buffers under AddressSanitizer + UndefinedBehaviorSanitizer + LeakSanitizer, without a GPU: the library's
translation units compiled host-only against the stub HIP runtime (tests/host_build.py, the recipe tests/test_sanitizers.py uses for
host_fuzz.cpp) and linked with the stand-alone program tests/host/sample_buffer_host.cpp, which walks the reference counts of both handles —
release while voices play, voices and mixers removed, destroy with buffers still held — and checks that the library's allocation and release
counters balance."""
import os
import subprocess

import host_build


def test_sample_buffer_reference_counts_under_asan_and_ubsan(tmp_path):
    exe = host_build.build_host_program(tmp_path, "sample_buffer_host")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **host_build.SANITIZER_ENV))
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-1000:], run.stderr[-4000:])
