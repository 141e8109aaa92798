"""The host side of samplers on the main mixer under AddressSanitizer + UndefinedBehaviorSanitizer + LeakSanitizer, without a GPU: the library's
translation units compiled host-only against the stub HIP runtime (tests/host_build.py) and linked with the stand-alone program
tests/host/main_sampler_host_trace.cpp. It drives both add calls and every refusal in its stated order, messages out of time order and in front of
the start time, a source added in front of and behind the pool, remove and destroy with events queued and the transient drop; from the records
the stub observes it checks the one source unit that holds the pool and its place in the order, the commands addressed to that unit, the chunk
grid begun again at every message, and that allocations and releases balance. A plain executable: nothing is preloaded."""
import os
import subprocess

import host_build


def test_main_sampler_host_trace_under_asan_and_ubsan(tmp_path):
    exe = host_build.build_host_program(tmp_path, "main_sampler_host_trace", hip_headers=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **host_build.SANITIZER_ENV))
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-1000:], run.stderr[-4000:])
