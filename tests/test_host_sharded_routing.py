"""The routing of the sharded handle (pg_sharded_* in phonic_amd/csrc/pg_sharded.hip) as a transcript, without a GPU: the stand-alone program
tests/host/sharded_routing_trace.cpp drives every pg_sharded_* entry point on handles of 1, 2 and 3 shards — nested sub-mixers, every kind of
voice, effects, shared sample buffers, ids that are negative, past the end, removed or of the wrong kind, every argument error that comes before
the handle, short writes in between — and prints one line per call: arguments, return value, error message, plus the shard of every new mixer
and the buffers' use counts after every new voice. The transcript was recorded from the tree before the routing was rewritten around one
resolver per id kind, one placement helper and one forwarder (tests/golden/sharded_routing_trace.txt); it must come out byte for byte, with the
shards' issuing threads on and off. Null handles: the entry points that always answered them are part of the transcript; for all the others the
program asserts the header's rule itself and reports how many it covered, which must be every remaining entry point of the header.
Built with -fsanitize=address,undefined (tests/host_build.py: a plain executable, nothing preloaded)."""
import os
import re
import subprocess

import host_build


def test_sharded_routing_transcript_is_unchanged(tmp_path):
    exe = host_build.build_host_program(tmp_path, "sharded_routing_trace")
    with open(os.path.join(host_build.ROOT, "tests", "golden", "sharded_routing_trace.txt")) as f:
        golden = f.read()
    assert len(golden) < 256 * 1024
    reports = []
    for threads in ("0", "1"):
        env = dict(os.environ, PHONIC_SHARD_THREADS=threads, **host_build.SANITIZER_ENV)
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-4000:])
        transcript, _, report = run.stdout.rstrip("\n").rpartition("\n")
        assert transcript + "\n" == golden, "the transcript differs from tests/golden/sharded_routing_trace.txt (PHONIC_SHARD_THREADS=%s)" % threads
        reports.append(report)
    # every entry point of the header that takes the handle is either in the transcript with a null handle or held to the null-handle rule
    with open(os.path.join(host_build.ROOT, "include", "phonic_gpu.h")) as f:
        with_handle = set(re.findall(r"\b(pg_sharded_\w+)\(pg_sharded_graph\* s\b", f.read()))
    in_golden = set(re.findall(r"^null (pg_sharded_\w+) ->", golden, flags=re.M))
    assert in_golden <= with_handle and len(with_handle) >= 58
    for report in reports:
        m = re.fullmatch(r"null handle rule asserted for (\d+) entry points", report)
        assert m and int(m.group(1)) == len(with_handle) - len(in_golden), (report, len(with_handle), len(in_golden))
