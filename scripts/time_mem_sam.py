"""Times read pairs -> SAM text on one stream on the fmi 'large' shape (device events, warm-up, median of N) and prints one JSON
line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device, gbx_mem_regs_device,
gbx_mem_pestat_device + gbx_mem_rescue_device, gbx_mem_pair_device, gbx_mem_cigar_device and gbx_mem_sam_device queued back to
back on the simulated FR pairs of scripts/time_mem_rescue.py.  Each stage's device time and the whole chain's; the SAM stage's
output bytes per second, its kernels' times, and the time to download its text into pinned host memory: the stage is to be read
against the cigar stage of the same run and against that download.  A sizing pass first learns the counts.  The first pairs'
lines are compared with the restated rules and every one of them goes through the validator.

    python scripts/time_mem_sam.py [--reads 200000] [--mutated 0.1] [--reps 10] [--out profiles/mem_sam_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if d not in sys.path:
        sys.path.insert(0, d)

import numpy as np  # noqa: E402

from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import bsw_seeds as BS  # noqa: E402
from genomicsbench_amd import fmi as FM  # noqa: E402
from genomicsbench_amd import mem_chain as MC  # noqa: E402
from genomicsbench_amd import mem_cigar as MG  # noqa: E402
from genomicsbench_amd import mem_pair as MP  # noqa: E402
from genomicsbench_amd import mem_regs as MR  # noqa: E402
from genomicsbench_amd import mem_rescue as MS  # noqa: E402
from genomicsbench_amd import mem_sam as SM  # noqa: E402
from time_mem_rescue import gen_pairs, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--genome", type=int, default=512 << 20)
    ap.add_argument("--seed", type=int, default=6001)
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mutated", type=float, default=0.1, help="fraction of the mates that hold no exact 19-mer")
    ap.add_argument("--check", type=int, default=300, help="pairs whose lines are checked against the restated rules")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_sam_time.json"))
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    import mem_sam_cases as K
    import mem_sam_ref as R
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    g = gen_fmi_genome(args.genome, args.seed)
    idx, smp = FM.build_index(g, device=dev, sa_compx=3)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    build_s = time.perf_counter() - t0
    rs, mutated = gen_pairs(g, args.reads // 2, args.seed + 1, args.mutated)
    L = len(g)
    names = ["read%d" % (k // 2) for k in range(rs.n_reads)]
    cnames = ["genome"]
    qual = np.random.default_rng(args.seed + 2).integers(33, 74, len(rs.enc)).astype(np.uint8)
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
    text_np = MC.text_of(g)
    ext = mc.extension(torch.from_numpy(text_np).to(dev))
    sp, rp, pp, cp = BS.make_seed_params(), MR.make_params(), MP.make_params(), MG.make_params()
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
    rsc = MS.DeviceMemRescue(rg, MS.make_params(), pp)
    rg.run(s)
    rsc.run(s)
    torch.cuda.synchronize()
    sized = rsc.results()
    pes = sized["pes"]
    rsc = MS.DeviceMemRescue(rg, MS.make_params(), pp, xreg_cap=sized["n_xregs"] + 64, xseed_cap=sized["n_xseeds"] + 64,
                             xsel_cap=sized["n_xsel"] + 64)
    pe = MP.DeviceMemPair(rsc, pp, pes_in=pes, psel_cap=sized["n_xregs"] + 64)
    rsc.run(s)
    pe.run(s)
    torch.cuda.synchronize()
    n_psel = pe.results()["n_psel"]
    pe = MP.DeviceMemPair(rsc, pp, pes_in=pes, psel_cap=n_psel + 64)
    cg = MG.DeviceMemCigar(pe.cigar_input, cp, cigar_cap=8 * pe.psel_cap, z_bytes=n_psel * per_record)
    sm = SM.DeviceMemSam(pe, cg, names, qual, cnames, max_recs=4, max_del=256)
    pe.run(s)
    cg.run(s)
    sm.run(s)
    torch.cuda.synchronize()
    nr, nm, nt = (int(x) for x in sm.counts.cpu().numpy())
    sm = SM.DeviceMemSam(pe, cg, names, qual, cnames, rec_cap=nr + 64, md_cap=nm + 64, text_cap=nt + 64)
    stages = [("smem", lambda: d.run(s)), ("sal", lambda: d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s)), ("chain", lambda: mc.run(s)),
              ("extend", lambda: ext.run(sp, s)), ("regs", lambda: rg.run(s)), ("rescue", lambda: rsc.run(s)), ("pair", lambda: pe.run(s)),
              ("cigar", lambda: cg.run(s)), ("sam", lambda: sm.run(s))]

    def whole():
        for _, fn in stages:
            fn()
    t_all, all_xs = median_ms(whole, args.reps, args.warmup, s)
    times = {name: median_ms(fn, args.reps, 1, s) for name, fn in stages}
    N.profile_begin()
    sm.run(s)
    torch.cuda.synchronize()
    kernels = {k: round(float(v[0]), 3) for k, v in N.profile_end().items() if k.startswith("mem_sam")}
    torch.cuda.synchronize()
    got = sm.results()
    pinned = torch.empty(got["n_text"], dtype=torch.uint8, pin_memory=True)
    t_down, down_xs = median_ms(lambda: pinned.copy_(sm.lines[:got["n_text"]], non_blocking=True), args.reps, 1, s)
    torch.cuda.synchronize()
    # the first pairs against the restated rules, and through the validator
    k = min(args.check, rs.n_reads // 2)
    pr, (alns, cigar) = pe.results(), cg.results()
    off = rsc.results()["xreg_off"][:2 * k + 1]
    want = R.sam_all(1, pr["pregs"][:off[-1]].view(K.REG_DTYPE), off, pr["pairs"][:k], alns, cigar, rs.enc, rs.read_off, rs.read_len, qual,
                     names[:2 * k], cnames, text_np, L, np.array([0, L]))
    head = got["lines"][:want["n_text"]].tobytes()
    ok = bool(head == want["lines"].tobytes() and got["recs"][:want["n_recs"]].tobytes() == want["recs"].tobytes())
    ok = ok and R.validate(head, text_np, cnames, np.array([0, L])) == want["n_recs"]
    flags = got["recs"]["flag"]
    out = {"what": "smem -> sal -> chain -> extend -> regs -> pestat + rescue -> pair -> cigar -> sam on one stream, fmi 'large' genome, "
                   "simulated FR pairs",
           "genome_bp": args.genome, "reads": rs.n_reads, "pairs": rs.n_reads // 2, "mutated_mates": int(len(mutated)),
           "index_build_s": round(build_s, 1), "max_occ": args.max_occ, "smems": n_smem, "hits": n_pos, "chains": n_chains, "seeds": n_seeds,
           "regions": n_regs, "reported": n_psel, "cigar_words": int(len(cigar)), "records": got["n_recs"], "md_bytes": got["n_md"],
           "text_bytes": got["n_text"], "unmapped_records": int(((flags & 0x4) != 0).sum()),
           "supplementary_records": int(((flags & 0x800) != 0).sum()), "proper_records": int(((flags & 0x2) != 0).sum())}
    for name, (t, xs) in times.items():
        out[name + "_ms"], out[name + "_ms_all"] = round(t, 3), xs
    out.update({"whole_ms": round(t_all, 3), "whole_ms_all": all_xs, "sam_kernels_ms": kernels,
                "sam_text_gb_per_s": round(got["n_text"] / times["sam"][0] / 1e6, 3), "sam_over_cigar": round(times["sam"][0] / times["cigar"][0], 3),
                "download_ms": round(t_down, 3), "download_ms_all": down_xs, "download_gb_per_s": round(got["n_text"] / t_down / 1e6, 3),
                "sam_over_download": round(times["sam"][0] / t_down, 3), "checked_pairs": k, "checked_equal": ok,
                "device": torch.cuda.get_device_name(0)})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
