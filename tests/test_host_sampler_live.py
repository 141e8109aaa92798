"""The host side of the sampler messages that change every voice while notes sound, under AddressSanitizer + UndefinedBehaviorSanitizer +
LeakSanitizer, without a GPU: the library's translation units compiled host-only against the stub HIP runtime (tests/host_build.py) and linked
with the stand-alone program tests/host/sampler_live_host_trace.cpp. It drives every new call on a file sampler with and without an envelope and
on a granular sampler with and without a matrix, messages out of time order, in front of the start time and on removed ids, with events queued
at remove and destroy; it checks that allocations and releases balance and — from the command records the host wrote for the launches — that
the values sampler_stage_command resolved are those of the time-ordered sequence. A plain executable: nothing is preloaded."""
import os
import subprocess

import host_build


def test_sampler_live_host_trace_under_asan_and_ubsan(tmp_path):
    exe = host_build.build_host_program(tmp_path, "sampler_live_host_trace", hip_headers=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **host_build.SANITIZER_ENV))
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-1000:], run.stderr[-4000:])
