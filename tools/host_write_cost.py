"""Host cost per pg_graph_write_device call, without a GPU: tests/host/host_write_cost.cpp built with the host side of the library at -O2, no
sanitizer, against the stub HIP runtime (tests/host_build.py, no observer installed), pinned to one CPU. Prints, per run, microseconds per
1024-frame call of a graph of 64 Gain -> Reverb sub-mixers: steady calls at max_blocks 1 and 32, then calls with one voice command each.

usage: python tools/host_write_cost.py [runs] [other csrc directory ...]
With more than one source directory (this tree's phonic_amd/csrc is always the last) the runs alternate between them: that is how
profiles/write_path_refactor_ab.txt compares a parent commit's sources (any checkout's phonic_amd/csrc, next to its include/) with this tree's."""
import os
import pathlib
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import host_build  # noqa: E402

LABELS = ("steady, max_blocks 1", "steady, max_blocks 32", "command, max_blocks 1", "command, max_blocks 32")


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    trees = [os.path.abspath(p) for p in sys.argv[2:]] + [os.path.join(ROOT, "phonic_amd", "csrc")]
    with tempfile.TemporaryDirectory() as tmp:
        exes = []
        for i, csrc in enumerate(trees):
            out = pathlib.Path(tmp, "build%d" % i)
            out.mkdir()
            exes.append(host_build.build_host_program(out, "host_write_cost", sanitize=None, csrc=csrc))
        res = [[] for _ in trees]
        for _ in range(runs):
            for i, exe in enumerate(exes):
                r = subprocess.run(["taskset", "-c", "3", exe], capture_output=True, text=True, check=True).stdout.split()
                res[i].append([float(x) for x in r])
                print(trees[i], " ".join(r), flush=True)
    for col, label in enumerate(LABELS):
        for i, csrc in enumerate(trees):
            v = sorted(r[col] for r in res[i])
            print("%s: %s: %s (median %.3f)" % (label, csrc, " ".join("%.3f" % x for x in v), statistics.median(v)))


if __name__ == "__main__":
    main()
