"""Times reads -> one record per reported alignment on one stream on the fmi 'large' shape (device events, warm-up, median of N)
and prints one JSON line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device,
gbx_mem_regs_device and gbx_mem_cigar_device queued back to back.  Each stage's device time and the whole chain's; the regions
stage is to be read against the chain stage of the same run (both are serial per read with lanes across a list), and the CIGAR
stage on the reported regions against the CIGAR stage on all seeds (as scripts/time_mem_cigar.py runs it), which is timed
beside it.  A sizing pass first learns the counts, so the timed passes run with tight capacities and no host synchronisation
inside.  The regions of the first reads are checked against tests/mem_regs_ref.py.

    python scripts/time_mem_regs.py [--reads 200000] [--reps 10] [--out profiles/mem_regs_time.json]
"""
import argparse
import ctypes as C
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
from genomicsbench_amd import mem_cigar as MG  # noqa: E402
from genomicsbench_amd import mem_regs as MR  # noqa: E402


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
    ap.add_argument("--check", type=int, default=2000, help="reads whose regions are checked against the restated rules")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_regs_time.json"))
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome, gen_fmi_reads
    import mem_regs_ref as R
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
    sp, rp, cp = BS.make_seed_params(), MR.make_params(), MG.make_params()
    mc.run(s)
    ext.run(sp, s)
    rg = MR.DeviceMemRegs(ext, rp)
    rg.run(s)
    torch.cuda.synchronize()
    res = ext.results()
    first = rg.results()
    n_regs, n_sel = first["n_regs"], first["n_sel"]
    rg = MR.DeviceMemRegs(ext, rp, reg_cap=n_regs + 64, sel_cap=n_sel + 64)
    regions = res[res[:, 2] >= 0]
    lq_max, lt_max = int((regions[:, 3] - regions[:, 2]).max()), int((regions[:, 5] - regions[:, 4]).max())
    per_record = int(MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(cp), lq_max, lt_max))
    cg_all = MG.DeviceMemCigar(ext, cp, cigar_cap=8 * ext.n, z_bytes=len(regions) * per_record)
    cg = MG.DeviceMemCigar(rg.cigar_input, cp, cigar_cap=8 * rg.sel_cap, z_bytes=n_sel * per_record)

    def whole():
        d.run(s)
        d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s)
        mc.run(s)
        ext.run(sp, s)
        rg.run(s)
        cg.run(s)
    t_all, all_xs = median_ms(whole, args.reps, args.warmup, s)
    t_smem, _ = median_ms(lambda: d.run(s), args.reps, 1, s)
    t_sal, _ = median_ms(lambda: d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s), args.reps, 1, s)
    t_chain, _ = median_ms(lambda: mc.run(s), args.reps, 1, s)
    t_ext, _ = median_ms(lambda: ext.run(sp, s), args.reps, 1, s)
    t_rg, rg_xs = median_ms(lambda: rg.run(s), args.reps, 1, s)
    t_cg, cg_xs = median_ms(lambda: cg.run(s), args.reps, 1, s)
    t_cg_all, _ = median_ms(lambda: cg_all.run(s), args.reps, 1, s)
    torch.cuda.synchronize()
    got = rg.results()
    alns, cigar = cg.results()
    # the first reads against the restated rules
    k = min(args.check, rs.n_reads)
    ch = mc.results()
    off = ch["chain_off"][:k + 1]
    want = R.regs_all(ch["chains"][:off[-1]], off, ch["seeds"], res[:len(ch["seeds"])], ch["l_rep"][:k], R.params(), 0, sel_cap=0)
    m = want["n_regs"]
    ok = bool(np.array_equal(got["reg_off"][:k + 1], want["reg_off"]) and got["regs"][:m].tobytes() == want["regs"].tobytes())
    regs = got["regs"]
    out = {"what": "smem -> sal -> chain -> extend -> regs -> cigar on one stream, fmi 'large' genome", "genome_bp": args.genome,
           "reads": rs.n_reads, "index_build_s": round(build_s, 1), "max_occ": args.max_occ, "smems": n_smem, "hits": n_pos,
           "chains": n_chains, "seeds": n_seeds, "extended_regions": int(len(regions)), "regions": n_regs, "reported": n_sel,
           "secondary": int((regs["secondary"] >= 0).sum()), "supplementary": int(((regs["flag"] & 0x800) != 0).sum()),
           "reads_with_a_reported_region": int(len(np.unique(regs["read"][(regs["flag"] & 1) != 0]))),
           "mapq_histogram": np.bincount(regs["mapq"][(regs["flag"] & 1) != 0], minlength=61).tolist(),
           "boundary_inputs_in_the_checked_reads": int(want["boundary"]), "cigar_words": int(len(cigar)),
           "records_without_room": int((alns["rid"] == -2).sum()),
           "smem_ms": round(t_smem, 3), "sal_ms": round(t_sal, 3), "chain_ms": round(t_chain, 3), "extend_ms": round(t_ext, 3),
           "regs_ms": round(t_rg, 3), "regs_ms_all": rg_xs, "cigar_ms": round(t_cg, 3), "cigar_ms_all": cg_xs,
           "cigar_on_all_seeds_ms": round(t_cg_all, 3), "whole_ms": round(t_all, 3), "whole_ms_all": all_xs,
           "regs_over_chain": round(t_rg / t_chain, 4), "cigar_reported_over_all_seeds": round(t_cg / t_cg_all, 4),
           "checked_reads": k, "checked_equal": ok, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
