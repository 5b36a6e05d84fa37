"""What scripts/time_mem_*.py (and time_fmi_sal.py, time_bsw_seeds.py for median_ms) share: the import path, the common arguments,
the genome and its index, simulated pairs, the stage chain of ``mem_pipeline.Stages`` with its sizing pass, the timing loop and the
JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

import numpy as np  # noqa: E402

from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import fmi as FM  # noqa: E402
from genomicsbench_amd import mem_chain as MC  # noqa: E402


def median_ms(fn, reps, warmup, stream):
    for _ in range(warmup):
        fn()
    tm = N.StreamTimer()
    xs = []
    for _ in range(reps):
        tm.start(stream)
        fn()
        tm.stop(stream)
        xs.append(tm.elapsed_ms())
    return float(np.median(xs)), [round(x, 3) for x in xs]


def gen_pairs(g, n_pairs, seed, mutated=0.0, length=151, mean=350., sd=35.):
    """n_pairs FR fragments of g as interleaved reads: the fragment's first `length` bases, then the reverse complement of its
    last ones, each with about 1 % substitutions; a fraction `mutated` of the mates has a substitution every 15 bases on top
    (drawn last, so the reads of a seed are the same without it).  -> (reads, the mutated pairs)."""
    rng = np.random.default_rng(seed)
    frag = np.maximum(length + 20, np.rint(rng.normal(mean, sd, n_pairs)).astype(np.int64))
    at = rng.integers(0, len(g) - frag.max(), n_pairs)
    col = np.arange(length)
    fwd = g[at[:, None] + col]
    rev = 3 - g[(at + frag)[:, None] - 1 - col]
    reads = np.empty((2 * n_pairs, length), dtype=np.uint8)
    reads[0::2], reads[1::2] = fwd, rev
    hit = rng.random(reads.shape) < 0.01
    reads[hit] = (reads[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    which = np.nonzero(rng.random(n_pairs) < mutated)[0]
    reads[2 * which[:, None] + 1, np.arange(7, length, 15)] += 1
    reads %= 4
    return FM.FmiReadSet.fixed(reads), which


def parser(out_name):
    """The arguments all of them take; --out defaults to profiles/<out_name>."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--genome", type=int, default=512 << 20)
    ap.add_argument("--seed", type=int, default=6001)
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    return ap


def setup(args):
    """The genome of bench.py's fmi job at --genome bases and its index with 1-in-8 suffix-array samples, built on the GPU.
    -> (device, the current stream's raw handle, genome, index, samples, the seconds the genome and index took)."""
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    g = gen_fmi_genome(args.genome, args.seed)
    idx, smp = FM.build_index(g, device=dev, sa_compx=3)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return dev, s, g, idx, smp, time.perf_counter() - t0


def sized_stages(idx, smp, rs, text, l_pac, dev, s, args, **options):
    """The stage chain over the reads as one contig, after the sizing pass (capacities of count + 64) -> (Stages, counts).
    text: the 2 L-byte text, on the host or the device; `options` go to mem_pipeline.Stages."""
    from genomicsbench_amd.mem_pipeline import Stages
    last = options.pop("last", None)
    d = FM.DeviceFmi(idx, rs, dev)
    d.set_sa(smp)
    st = Stages(d, text, l_pac, max_occ=args.max_occ, params=dict(chain=MC.make_params(max_occ=args.max_occ)), **options)
    return st, st.tighten(s, 64, last=last)


def time_steps(st, s, args, last=None):
    """-> (the whole chain's median ms, its runs, {step: (median ms, runs)}) of the steps up to `last`."""
    steps = st.steps(s, last=last)

    def whole():
        for _, fn in steps:
            fn()
    t_all, all_xs = median_ms(whole, args.reps, args.warmup, s)
    return t_all, all_xs, {name: median_ms(fn, args.reps, 1, s) for name, fn in steps}


def emit(out, path, ok):
    """Prints the JSON line, writes it to `path` if one is given -> the exit status."""
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1
