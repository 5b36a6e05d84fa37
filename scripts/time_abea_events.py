#!/usr/bin/env python3
"""Times abea's signal stage on one device: event detection, scalings, the chained host entry, the existing align step on
the same reads and the CPU restatement on 16 threads.  Prints one JSON line and writes profiles/abea_events_time_<preset>.json.

  python scripts/time_abea_events.py --preset small|large [--reps N] [--no-write]

'large' is the 10 000 reads of abea large (seed 5001) with generated raw signal.  One warm-up, then the median of --reps.
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
    a = ap.parse_args()
    import torch
    import abea_events_ref as R
    from genomicsbench_amd import abea_signal as AS
    from genomicsbench_amd.datagen import gen_abea_raw

    n_reads, seed = PRESETS[a.preset]
    ss = gen_abea_raw(n_reads, seed)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    d = AS.DeviceAbeaSignalSet(ss, dev)

    def timed(fn, reps):
        out = []
        for k in range(reps + 1):                     # the first run is the warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return float(np.median(out[1:])), out[1:]

    count_ms, _ = timed(lambda: d.count(stream), a.reps)
    d.size_outputs()
    fill_ms, _ = timed(lambda: d.fill(stream), a.reps)
    detect_ms, detect_all = timed(lambda: (d.count(stream), d.size_outputs(), d.fill(stream)), a.reps)
    scal_ms, _ = timed(lambda: d.scalings(stream), a.reps)
    drs, keep = d.align_set()
    align_ms, _ = timed(lambda: drs.run(stream), a.reps)
    off, ev, scale, shift, status = d.results()
    t = time.perf_counter()
    got = AS.signal_align_host(ss, event_cap=len(ev))
    chained_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    got = AS.signal_align_host(ss, event_cap=len(ev))
    chained_ms = min(chained_ms, (time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    want = R.run(ss, 16)
    cpu_ms = (time.perf_counter() - t) * 1e3
    same = bool(np.array_equal(off, want["event_off"]) and np.array_equal(ev["mean"].view(np.uint32), want["events"]["mean"].view(np.uint32))
                and np.array_equal(scale.view(np.uint32), want["scale"].view(np.uint32)))
    res = dict(kernel="abea_events", preset=a.preset, n_reads=n_reads, seed=seed, n_samples=int(ss.raw.size), n_events=int(len(ev)),
               device=torch.cuda.get_device_name(0), reps=a.reps,
               count_ms=round(count_ms, 3), fill_ms=round(fill_ms, 3), detect_ms=round(detect_ms, 3), detect_ms_all=[round(x, 3) for x in detect_all],
               scalings_ms=round(scal_ms, 3), detect_plus_scalings_ms=round(detect_ms + scal_ms, 3), align_ms=round(align_ms, 3),
               chained_host_ms=round(chained_ms, 3), restatement_16_threads_ms=round(cpu_ms, 3),
               speedup_vs_restatement=round(cpu_ms / (detect_ms + scal_ms), 2), ratio_to_align=round((detect_ms + scal_ms) / align_ms, 2),
               in_order_share=round(float(np.count_nonzero(status & AS.EV_INORDER)) / max(n_reads, 1), 5),
               reads_without_events=int(np.count_nonzero(status & AS.EV_NONE)), reads_aligned=int(np.count_nonzero(got["n_pairs"] > 0)),
               equals_restatement=same)
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "abea_events_time_%s.json" % a.preset), "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
