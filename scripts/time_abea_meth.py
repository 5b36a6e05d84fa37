#!/usr/bin/env python3
"""Times abea's methylation scoring stage on one device: the device-resident score step, the host entry, the site planner and
the CPU restatement on 16 threads, all in one run.  Prints one JSON line and writes profiles/abea_meth_time_<preset>.json.

  python scripts/time_abea_meth.py --preset small|large [--reps N] [--no-write] [--no-cpu]

'large' is the 10 000 reads of abea large (seed 5001) with the generated record.  One warm-up, then the median of --reps.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PRESETS = {"small": (256, 5001), "large": (10000, 5001)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="small")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--no-cpu", action="store_true", help="skip the restatement (a profiler run)")
    a = ap.parse_args()
    import torch
    import abea_meth_ref as R
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import abea_meth as AM
    from genomicsbench_amd.datagen import gen_abea_meth

    n_reads, seed = PRESETS[a.preset]
    ms = gen_abea_meth(n_reads, seed)
    ms.sites()                                           # loads the library
    t = time.perf_counter()
    sites, jobs, arena = ms.sites()
    planner_ms = (time.perf_counter() - t) * 1e3
    js = ms.job_set(jobs, arena)
    t = time.perf_counter()
    plan = js.plan()
    plan_ms = (time.perf_counter() - t) * 1e3
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    d = AM.DeviceAbeaMethJobSet(js, dev)

    def timed(fn, reps):
        out = []
        for k in range(reps + 1):                     # the first run is the warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return float(np.median(out[1:])), out[1:]

    N.profile_begin()
    d.run(stream)
    torch.cuda.synchronize()
    per_class = {k: round(v[0], 3) for k, v in N.profile_end().items()}
    score_ms, score_all = timed(lambda: d.run(stream), a.reps)
    got = d.results()
    host_ms = 1e30
    for _ in range(2):
        t = time.perf_counter()
        hs = AM.score_host(js)
        host_ms = min(host_ms, (time.perf_counter() - t) * 1e3)
    same, cpu_ms = bool(np.array_equal(got.view(np.uint32), hs.view(np.uint32))), None
    if not a.no_cpu:
        t = time.perf_counter()
        want, _ = R.score(js, 16)
        cpu_ms = (time.perf_counter() - t) * 1e3
        same = same and bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    cells = js.cells()
    off = plan["class_off"]
    res = dict(kernel="abea_meth", preset=a.preset, n_reads=n_reads, seed=seed, n_sites=int(len(sites)), n_jobs=int(js.n_jobs), cells=cells,
               jobs_per_class=[int(off[c + 1] - off[c]) for c in range(4)], max_kmers=int(js.n_kmers.max()), max_rows=int(js.rows.max()),
               device=torch.cuda.get_device_name(0), reps=a.reps, score_ms=round(score_ms, 3), score_ms_all=[round(x, 3) for x in score_all],
               kernel_ms_per_class=per_class, cells_per_s=round(cells / (score_ms * 1e-3), 1), score_host_ms=round(host_ms, 3),
               planner_ms=round(planner_ms, 3), plan_ms=round(plan_ms, 3),
               restatement_16_threads_ms=None if cpu_ms is None else round(cpu_ms, 3),
               speedup_vs_restatement=None if cpu_ms is None else round(cpu_ms / score_ms, 2), equals_restatement=same)
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "abea_meth_time_%s.json" % a.preset), "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
