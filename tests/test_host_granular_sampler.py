"""The host side of the granular-mode samplers under AddressSanitizer + UndefinedBehaviorSanitizer + LeakSanitizer, without a GPU: the library's
translation units compiled host-only against the stub HIP runtime (tests/host_build.py) and linked with the stand-alone program
tests/host/granular_sampler_host_trace.cpp, which drives add, messages in and out of time order, the refusals, remove with notes sounding, a mixer
removed with its sampler and destroy with live samplers, checks that the library's allocation and release counters balance, and reads from the
stub's observer the order of the launches per span of the sampler's source-write grid: close / open, grains, ..., closing, then the unit kernels —
for a piece with 0, 1 and 3 cuts, a cut on a piece edge and several messages on one frame (one boundary). A plain executable: nothing is preloaded."""
import os
import subprocess

import host_build


def test_granular_sampler_host_trace_under_asan_and_ubsan(tmp_path):
    exe = host_build.build_host_program(tmp_path, "granular_sampler_host_trace", hip_headers=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **host_build.SANITIZER_ENV))
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-1000:], run.stderr[-4000:])
