"""What the sampler host code writes, as a transcript, without a GPU: the stand-alone program tests/host/sampler_records_trace.cpp drives the
constructors, timed calls, refusals and read-backs of phonic_amd/csrc/pg_sampler.hip against the stub HIP runtime (tests/host/hip_stub.cpp), whose
"device" memory is plain host memory, and prints every record they upload field by field — PgSamplerRec, PgSamplerTab, PgGSampler, PgGrainVoice
with its pool, grains and modulation matrix, PgEnv, PgEnvTable, the pool's PgVoice records, what the host keeps of each sampler — floats as bit
patterns, pointers as allocation ordinal + offset; the PgCmd records a write hands to the kernels for every timed sampler call (in order, out of
order, in front of a start time, on removed ids); the return code and message of every refusal, with and without a handle; and what the read-backs
return, a stopped transient sampler included. The transcript was recorded from the tree before the sampler host code was consolidated into one
builder per record and one message path (tests/golden/sampler_records_trace.txt); it must come out byte for byte, twice. Built with
-fsanitize=address,undefined (tests/host_build.py: a plain executable, nothing preloaded), LeakSanitizer on."""
import os
import subprocess

import host_build


def test_sampler_records_transcript_is_unchanged(tmp_path):
    exe = host_build.build_host_program(tmp_path, "sampler_records_trace", hip_headers=True)
    with open(os.path.join(host_build.ROOT, "tests", "golden", "sampler_records_trace.txt")) as f:
        golden = f.read()
    assert len(golden) < 256 * 1024
    outputs = []
    for _ in range(2):
        run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, **host_build.SANITIZER_ENV))
        assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-4000:])
        outputs.append(run.stdout)
    if outputs[0] != golden:
        a, b = outputs[0].splitlines(), golden.splitlines()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        header = next((l for l in reversed(a[:first + 1]) if l.startswith("== ")), "")
        raise AssertionError("the transcript differs from tests/golden/sampler_records_trace.txt at line %d (%s):\n  now:    %s\n  golden: %s" % (
            first + 1, header, a[first][:400] if first < len(a) else "<end>", b[first][:400] if first < len(b) else "<end>"))
    assert outputs[1] == outputs[0], "two runs of the program gave different transcripts"
