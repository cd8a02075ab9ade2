"""What the benches and speed tools of this folder share: the import path of the product and the tests, a timer on HIP event pairs, and
the reader of a profiler run's per-kernel totals.  Importing it puts the repository on `sys.path`."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "image-to-video-i2v-attack_amd"), ROOT]


def timed(fn, reps, warm):
    """`warm` untimed calls, then `reps` calls each between a HIP event pair: (median, fastest, slowest) in ms."""
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def kernel_rows(path):
    """(name, calls, total ns) per kernel of a `rocprofv3 --kernel-trace --stats` run: from its results database (`.db`, the profiler's
    default output: the `kernels` view, one row per dispatch) or from its kernel stats csv (`--output-format csv`)."""
    if path.endswith(".db"):
        import sqlite3
        return sqlite3.connect(path).execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
    import csv
    return [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]
