"""The host-only build of the library for stand-alone test programs (tests/host/*.cpp with a main of their own): the library's translation
units compiled `hipcc --cuda-host-only` (no device code) under a sanitizer, tests/host/hip_stub.cpp in place of the HIP runtime, empty symbols
for the absent device code objects, and one plain executable — the sanitizer's runtime is linked in, nothing is preloaded. The same recipe as
tests/test_sanitizers.py uses for host_fuzz.cpp."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SANITIZER_ENV = dict(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def build_host_program(tmp_path, program, sanitize="address,undefined", hip_headers=False, csrc=None):
    """Builds tests/host/<program>.cpp against the host side of the library under -fsanitize=<sanitize>; returns the executable's path.
    sanitize=None: a plain -O2 build (host-cost timing). hip_headers: the program includes HIP headers itself (the stub's observer, pg_dev.h) and
    is compiled like the library's units. csrc: another directory of library sources to build against (default: phonic_amd/csrc)."""
    if not (os.path.exists(HIPCC) and os.path.exists(CLANG)):
        pytest.skip("hipcc not available")
    csrc = csrc or os.path.join(ROOT, "phonic_amd", "csrc")
    san = (["-fsanitize=" + sanitize] + (["-fno-sanitize-recover=undefined"] if "undefined" in sanitize else [])) if sanitize else []
    opt = ["-O1", "-g"] if sanitize else ["-O2"]
    flags = ["--cuda-host-only", "-std=c++17"] + opt + ["-fPIC", "-ffp-contract=off", "-fno-omit-frame-pointer", "-DPG_FAST_WAVES=2", "-Wno-unused", "-Wno-unused-command-line-argument"] + san
    units = ["pg_host", "pg_sampler", "pg_fxstate", "pg_effect", "pg_sharded", "pg_kernels"] + sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(csrc, "pg_k_*.hip")))
    objs, jobs = [], []
    for tu in units:
        objs.append(str(tmp_path / (tu + ".o")))
        jobs.append(subprocess.Popen([HIPCC] + flags + ["-c", os.path.join(csrc, tu + ".hip"), "-o", objs[-1]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    stub = str(tmp_path / "hip_stub.o")
    jobs.append(subprocess.Popen([HIPCC] + flags + ["-c", os.path.join(ROOT, "tests", "host", "hip_stub.cpp"), "-x", "hip", "-o", stub], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    main = os.path.join(ROOT, "tests", "host", program + ".cpp")
    if hip_headers:
        jobs.append(subprocess.Popen([HIPCC] + flags + ["-x", "hip", "-c", main, "-o", str(tmp_path / (program + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        main = str(tmp_path / (program + ".o"))
    for j in jobs:
        out, _ = j.communicate(timeout=900)
        assert j.returncode == 0, out[-3000:]
    # the module constructors name the (absent) device code objects of their translation units: define those symbols, empty
    undefined = subprocess.run(["nm", "-u"] + objs, capture_output=True, text=True).stdout.split()
    fat = tmp_path / "fatbins.cpp"
    fat.write_text("".join(f"extern \"C\" const char {s}[16] = {{0}};\n" for s in sorted(set(u for u in undefined if u.startswith("__hip_fatbin_")))))
    exe = str(tmp_path / program)
    link = subprocess.run([CLANG, "-std=c++17"] + opt + san + [main, str(fat), stub] + objs + ["-o", exe, "-lpthread", "-ldl"],
                          capture_output=True, text=True, timeout=600)
    assert link.returncode == 0, link.stderr[-3000:]
    return exe
