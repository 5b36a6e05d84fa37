"""Times the suffix-array lookup of SMEM hits on the fmi 'large' shape (device events, warm-up, median of N) and prints one JSON
line: the 512-Mbp genome of bench.py's fmi job, its index built on the GPU with 1-in-8 suffix-array samples, the SMEMs of
--reads reads from gbx_fmi_smem_device, then gbx_fmi_sal_device on them on the same stream (max_occ 500, bwa's default).
Beside it the SMEM time for the same reads, and the LF steps as 64-byte line requests against the random-gather ceiling of
profiles/gather_peak.json.  A sample of the hits is checked against tests/sal_ref.py's restated walk.

    python scripts/time_fmi_sal.py [--reads 1000000] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if d not in sys.path:
        sys.path.insert(0, d)

import numpy as np  # noqa: E402

from genomicsbench_amd import fmi as FM  # noqa: E402
from _mem_timing import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=512 << 20)
    ap.add_argument("--seed", type=int, default=6001)
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=20000, help="hits checked against the restated walk")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome, gen_fmi_reads
    import sal_ref as R
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    g = gen_fmi_genome(args.genome, args.seed)
    idx, smp = FM.build_index(g, device=dev, sa_compx=3)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    build_s = time.perf_counter() - t0
    rs = gen_fmi_reads(g, args.reads, args.seed + 1)
    d = FM.DeviceFmi(idx, rs, dev)
    d.set_sa(smp)
    t_smem, _ = median_ms(lambda: d.run(s), args.reps, args.warmup, s)
    n_smem = int(d.n_out.item())
    assert n_smem <= d.out_cap and not d.overflow(), "SMEM output truncated"
    t_sal, xs = median_ms(lambda: d.sal(args.max_occ, stream=s), args.reps, args.warmup, s)
    torch.cuda.synchronize()
    pos, off = d.sal_results()
    steps, longest = d.sal_steps()
    hits = len(pos)
    # a sample of the hits against the restated walk over the host tables
    hidx, hsmp = idx.host(), smp.host()
    smems = d.out[:n_smem * FM.SMEM_DTYPE.itemsize].cpu().numpy().view(FM.SMEM_DTYPE)
    rows, roff = R.hit_rows(smems["k"], smems["s"], args.max_occ)
    assert np.array_equal(roff, off)
    pick = np.random.default_rng(1).choice(hits, min(args.check, hits), replace=False)
    ok = bool(np.array_equal(R.sa_walk(hidx, hsmp, rows[pick]), pos[pick]))
    peak = json.load(open(os.path.join(ROOT, "profiles", "gather_peak.json")))
    ceiling = max(r["dependent"] for r in peak["rows"]) * 1e9
    line_rate = steps * 64 / (t_sal * 1e-3)
    out = {"what": "gbx_fmi_sal_device on the SMEMs of gbx_fmi_smem_device, fmi 'large' genome", "genome_bp": args.genome,
           "reads": rs.n_reads, "index_build_s": round(build_s, 1), "max_occ": args.max_occ, "smems": n_smem, "hits": hits,
           "hits_per_smem": round(hits / max(n_smem, 1), 2), "lf_steps": steps, "lf_steps_mean": round(steps / max(hits, 1), 3),
           "lf_steps_max": longest, "sal_ms": round(t_sal, 3), "sal_ms_all": [round(x, 3) for x in xs], "smem_ms": round(t_smem, 3),
           "sal_over_smem": round(t_sal / t_smem, 4), "hits_per_s": round(hits / (t_sal * 1e-3)),
           "lines_per_s": round(steps / (t_sal * 1e-3)), "line_gb_per_s": round(line_rate / 1e9, 1),
           "gather_ceiling_frac": round(line_rate / ceiling, 3), "checked_hits": int(len(pick)), "checked_equal": ok,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
