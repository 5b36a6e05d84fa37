"""Times reads -> extension results on one stream on the fmi 'large' shape (device events, warm-up, median of N) and prints one
JSON line: the 512-Mbp genome of bench.py's fmi job, its index built on the GPU with 1-in-8 suffix-array samples, --reads
reads; gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device and gbx_bsw_extend_seeds_device queued back to back.
Each stage's device time, the whole chain's, and the chaining stage's compulsory bytes (what it must read and write once)
against the HBM roofline.  A sizing pass first learns the counts, so the timed passes run with tight capacities and no
host synchronisation inside.  A sample of reads is checked against tests/mem_chain_ref.py.

    python scripts/time_mem_chain.py [--reads 200000] [--reps 10] [--out profiles/mem_chain_time.json]
"""
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
from genomicsbench_amd import bsw_seeds as BS  # noqa: E402
from genomicsbench_amd import fmi as FM  # noqa: E402
from genomicsbench_amd import mem_chain as MC  # noqa: E402

HBM_GBS = 8000.0            # MI355X peak HBM3E bandwidth, GB/s


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--genome", type=int, default=512 << 20)
    ap.add_argument("--seed", type=int, default=6001)
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=300, help="reads checked against the restated rules")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_chain_time.json"))
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome, gen_fmi_reads
    import mem_chain_ref as R
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
    L = len(g)
    # sizing pass: the counts of every stage, then tight capacities
    d = FM.DeviceFmi(idx, rs, dev)
    d.set_sa(smp)
    d.run(s)
    d.sal(args.max_occ, stream=s)
    torch.cuda.synchronize()
    n_smem, n_pos = int(d.n_out.item()), int(d.n_pos.item())
    assert n_smem <= d.out_cap and not d.overflow() and n_pos <= d.pos_cap, "seeding output truncated"
    d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s)
    params = MC.make_params(max_occ=args.max_occ)
    mc = MC.DeviceMemChain(d, L, params=params)
    mc.run(s)
    torch.cuda.synchronize()
    n_chains, n_seeds = (int(x) for x in mc.counts.cpu().numpy())
    mc = MC.DeviceMemChain(d, L, params=params, chain_cap=n_chains + 64, seed_cap=n_seeds + 64)
    text = torch.from_numpy(MC.text_of(g)).to(dev)
    ext = mc.extension(text)
    sp = BS.make_seed_params()

    def whole():
        d.run(s)
        d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s)
        mc.run(s)
        ext.run(sp, s)
    t_all, all_xs = median_ms(whole, args.reps, args.warmup, s)
    t_smem, _ = median_ms(lambda: d.run(s), args.reps, 1, s)
    t_sal, _ = median_ms(lambda: d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s), args.reps, 1, s)
    t_chain, chain_xs = median_ms(lambda: mc.run(s), args.reps, 1, s)
    t_ext, _ = median_ms(lambda: ext.run(sp, s), args.reps, 1, s)
    torch.cuda.synchronize()
    got = mc.results()
    assert len(got["chains"]) == n_chains and len(got["seeds"]) == n_seeds
    # a sample of reads against the restated rules
    k = min(args.check, rs.n_reads)
    smems, smem_off = d.results()
    pos, pos_off = d.sal_results()
    want = R.chain_all(smems["m"].astype(np.int64), smems["n"].astype(np.int64), smems["s"], smem_off[:k + 1], pos, pos_off, rs.read_off[:k],
                       rs.read_len[:k], L, [0, L], R.params(max_occ=args.max_occ))
    nc, ns = len(want["chains"]), len(want["seeds"])
    ok = bool(got["chains"][:nc].tobytes() == want["chains"].tobytes() and got["seeds"][:ns].tobytes() == want["seeds"].tobytes() and
              np.array_equal(got["chain_off"][:k + 1], want["chain_off"]) and np.array_equal(got["l_rep"][:k], want["l_rep"]))
    # compulsory traffic of the chaining stage: SMEM records, offsets and hits in; chains, offsets, seeds and l_rep out
    rd = n_smem * 40 + (n_smem + 1) * 8 + n_pos * 8 + (rs.n_reads + 1) * 8 + rs.n_reads * 12
    wr = n_chains * 56 + (rs.n_reads + 1) * 8 + n_seeds * 40 + rs.n_reads * 4
    floor_ms = (rd + wr) / (HBM_GBS * 1e9) * 1e3
    res = ext.results(n_seeds)
    out = {"what": "smem -> sal -> chain -> extend on one stream, fmi 'large' genome", "genome_bp": args.genome, "reads": rs.n_reads,
           "index_build_s": round(build_s, 1), "max_occ": args.max_occ, "smems": n_smem, "hits": n_pos, "chains": n_chains,
           "seeds": n_seeds, "most_chains_made_by_a_checked_read": int(max(want["made"])) if want["made"] else 0,
           "smem_ms": round(t_smem, 3), "sal_ms": round(t_sal, 3),
           "chain_ms": round(t_chain, 3), "chain_ms_all": chain_xs, "extend_ms": round(t_ext, 3), "whole_ms": round(t_all, 3),
           "whole_ms_all": all_xs, "chain_over_smem_plus_sal": round(t_chain / (t_smem + t_sal), 4),
           "chain_bytes_read": rd, "chain_bytes_written": wr, "chain_hbm_floor_ms": round(floor_ms, 4),
           "chain_hbm_roofline_frac": round(floor_ms / t_chain, 4), "chain_workspace_bytes": int(mc.work_bytes),
           "extended_with_score": int((res[:, 0] > 0).sum()), "checked_reads": k, "checked_equal": ok,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
