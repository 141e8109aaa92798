"""The host part of the playback status events — the ring and its drop count, the compaction of the kernel's slots, the order of a chunk's
records, the merge of several shards, polls smaller than what waits — as a stand-alone program (tests/host/status_host.cpp: its own main,
phonic_amd/csrc/pg_status_host.h and nothing else of the library) built with -fsanitize=address,undefined (the sanitizer's runtime linked in statically: the program needs nothing preloaded) and run in the
environment the test runs in, unchanged but for the sanitizers' options."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_status_host_header_under_asan_and_ubsan(tmp_path):
    rocm_clang = "/opt/rocm/lib/llvm/bin/clang++"   # (the compiler the library itself is built with)
    cxx = rocm_clang if os.path.exists(rocm_clang) else (shutil.which("clang++") or shutil.which("g++"))
    assert cxx, "no C++ compiler: the library cannot be built here either"
    static_runtime = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else ["-static-libsan"]
    exe = str(tmp_path / "status_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(ROOT, "tests", "host", "status_host.cpp"), "-o", exe] + static_runtime, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout[-1000:], run.stderr[-4000:])
