"""The host side of the samplers under AddressSanitizer + UndefinedBehaviorSanitizer + LeakSanitizer, without a GPU: the library's translation
units compiled host-only against the stub HIP runtime (tests/host_build.py) and linked with the stand-alone program
tests/host/sampler_host_trace.cpp, which drives every sampler entry point — add, messages in and out of time order, removed and unknown ids,
the main-mixer refusal, remove during pending events, short writes in between, a mixer removed with its sampler, destroy with live samplers —
and checks that the library's allocation and release counters balance. A plain executable: nothing is preloaded."""
import os
import subprocess

import host_build


def test_sampler_host_trace_under_asan_and_ubsan(tmp_path):
    exe = host_build.build_host_program(tmp_path, "sampler_host_trace")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **host_build.SANITIZER_ENV))
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-1000:], run.stderr[-4000:])
