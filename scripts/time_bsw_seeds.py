"""Times whole-seed extension on generated seeds (device events, warm-up, median of N) and prints one JSON line:
  (a) gbx_bsw_extend_seeds_device: the whole call on the device, inputs resident in HBM;
  (b) the same work composed from the pair entry: host reversal, gbx_bsw_extend_device per side and band try on the seeds
      that try extends (descriptors up, results down), the band test and the hand-off on the host (tests/seedext_ref.py with
      the GPU as its ksw);
  (c) the flat bsw 'large' shape of bench.py (2 M pairs, seed 1002) through gbx_bsw_extend_device, for scale.
Cells are sum(qlen * tlen) over the extensions executed (band retries included).

    python scripts/time_bsw_seeds.py [--n 1000000] [--reps 10] [--reps-b 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if d not in sys.path:
        sys.path.insert(0, d)

import numpy as np  # noqa: E402

from genomicsbench_amd.bsw import DeviceBswBatch, make_params  # noqa: E402
from genomicsbench_amd.bsw_seeds import DeviceSeedBatch, gen_seeds, make_seed_params  # noqa: E402
import seedext_ref as R  # noqa: E402
from _mem_timing import median_ms  # noqa: E402


def composed(p, b, device, stream=None, stats=None):
    """Path (b): the restatement's composition with gbx_bsw_extend_device as the ksw step.  Each arena goes up once per call."""
    import torch
    arenas = {}

    def up(a):
        if id(a) not in arenas:
            arenas[id(a)] = (a, torch.from_numpy(np.concatenate([a, np.zeros(64, np.uint8)])).to(device))
        return arenas[id(a)][1]

    def ksw(params, pb):
        t = lambda x: torch.from_numpy(x).to(device)
        d = DeviceBswBatch.from_tensors(dict(ref=up(pb.ref), qer=up(pb.qer), idr=t(pb.idr), idq=t(pb.idq), len1=t(pb.len1),
                                             len2=t(pb.len2), h0=t(pb.h0)), device)
        d.run(params, stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        return d.results()
    return R.extend_seeds_ref(p, b, ksw=ksw, stats=stats), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-b", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--w", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    b = gen_seeds(args.n, args.seed)
    p = make_seed_params(w=args.w)

    d = DeviceSeedBatch(b, dev)
    ta, xa = median_ms(lambda: d.run(p, s), args.reps, args.warmup, s)
    got_a = d.results()

    stats = {}
    got_b, _ = composed(p, b, dev, s, stats)
    tb, xb = median_ms(lambda: composed(p, b, dev, s), args.reps_b, 1, s)

    flat = __import__("genomicsbench_amd.datagen", fromlist=["gen_bsw"]).gen_bsw(2_000_000, 1002)
    df = DeviceBswBatch(flat, dev)
    pf = make_params()
    tc, _ = median_ms(lambda: df.run(pf, s), args.reps, args.warmup, s)

    per_try = {side: [t["pairs"] for t in v] for side, v in stats.items()}
    cells = sum(t["cells"] for v in stats.values() for t in v)
    first = sum(v[0]["pairs"] for v in stats.values())
    line = {
        "what": "bsw whole-seed extension, %d generated seeds (gen_seeds seed %d), w=%d max_band_try=%d" % (b.n, args.seed, args.w, p.max_band_try),
        "a_device_ms": round(ta, 3), "a_ns_per_seed": round(ta * 1e6 / b.n, 2),
        "b_composed_ms": round(tb, 3), "b_ns_per_seed": round(tb * 1e6 / b.n, 2),
        "c_flat_large_ms": round(tc, 3), "c_ns_per_pair": round(tc * 1e6 / flat.n, 2),
        "c_flat_large_gcups": round(flat.nominal_cells / tc / 1e6, 1),
        "pairs_per_side_and_try": per_try, "cells": cells,
        "a_gcups": round(cells / ta / 1e6, 1), "b_gcups": round(cells / tb / 1e6, 1),
        "retry_fraction": round((sum(sum(v) for v in per_try.values()) - first) / max(first, 1), 5),
        "a_equals_b": bool(np.array_equal(got_a, got_b)),
        "a_runs_ms": [round(x, 3) for x in xa], "b_runs_ms": [round(x, 3) for x in xb],
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["a_equals_b"] else 1


if __name__ == "__main__":
    sys.exit(main())
