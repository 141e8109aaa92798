"""What the write path enqueues, as a transcript, without a GPU: the stand-alone program tests/host/write_launch_trace.cpp installs the observer
of the stub HIP runtime (tests/host/hip_stub.cpp) and drives pg_graph_write_device, pg_graph_write, pg_graph_process_bus_device and the sharded
handle's writes through small scripted scenarios — every call length and max_frames / max_blocks shape, staged sub-mixers leaving and regaining the
steady state, a bus chain with its overlap pipeline, nested mixers at the call budget, deferred-bus graphs, metering, status / granular / host-fed
voices, host writes longer than the staging, the command ring's overflow and wrap, an injected launch failure, handles of 1 to 3 shards — and
prints one line per launch, copy, fill, event record, wait, synchronisation and stream query, every launch decoded field by field, pointers as
allocation ordinal + offset. The program plays the words the host reads back from the device (the generic kernel's feedback, the status word),
so the super-block path is reached on a CPU. The transcript was recorded from the tree before the write path was split into named steps
(tests/golden/write_launch_trace.txt); it must come out byte for byte, twice. Built with -fsanitize=address,undefined (tests/host_build.py: a
plain executable, nothing preloaded)."""
import os
import subprocess

import host_build


def test_write_launch_transcript_is_unchanged(tmp_path):
    exe = host_build.build_host_program(tmp_path, "write_launch_trace", hip_headers=True)
    with open(os.path.join(host_build.ROOT, "tests", "golden", "write_launch_trace.txt")) as f:
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
        raise AssertionError("the transcript differs from tests/golden/write_launch_trace.txt at line %d (%s):\n  now:    %s\n  golden: %s" % (
            first + 1, header, a[first][:400] if first < len(a) else "<end>", b[first][:400] if first < len(b) else "<end>"))
    assert outputs[1] == outputs[0], "two runs of the program gave different transcripts"
