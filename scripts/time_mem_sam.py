"""Times read pairs -> SAM text on one stream on the fmi 'large' shape (device events, warm-up, median of N) and prints one JSON
line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device, gbx_mem_regs_device,
gbx_mem_pestat_device + gbx_mem_rescue_device, gbx_mem_pair_device, gbx_mem_cigar_device and gbx_mem_sam_device queued back to
back on the simulated FR pairs of scripts/time_mem_rescue.py.  Each stage's device time and the whole chain's; the SAM stage's
output bytes per second, its kernels' times, and the time to download its text into pinned host memory: the stage is to be read
against the cigar stage of the same run and against that download.  A sizing pass first learns the counts.  The first pairs'
lines are compared with the restated rules and every one of them goes through the validator.

    python scripts/time_mem_sam.py [--reads 200000] [--mutated 0.1] [--reps 10] [--out profiles/mem_sam_time.json]
"""
import sys

import numpy as np

import _mem_timing as T
from genomicsbench_amd import _native as N


def main():
    ap = T.parser("mem_sam_time.json")
    ap.add_argument("--mutated", type=float, default=0.1, help="fraction of the mates that hold no exact 19-mer")
    ap.add_argument("--check", type=int, default=300, help="pairs whose lines are checked against the restated rules")
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.mem_chain import text_of
    import mem_sam_cases as K
    import mem_sam_ref as R
    dev, s, g, idx, smp, build_s = T.setup(args)
    rs, mutated = T.gen_pairs(g, args.reads // 2, args.seed + 1, args.mutated)
    L = len(g)
    names = ["read%d" % (k // 2) for k in range(rs.n_reads)]
    cnames = ["genome"]
    qual = np.random.default_rng(args.seed + 2).integers(33, 74, len(rs.enc)).astype(np.uint8)
    text_np = text_of(g)
    st, n = T.sized_stages(idx, smp, rs, torch.from_numpy(text_np).to(dev), L, dev, s, args, sam_input=(names, qual, cnames),
                           caps=dict(max_recs=4, max_del=256))
    rsc, pe, cg, sm = st.rescue, st.pair, st.cigar, st.sam
    n_smem, n_pos, n_chains, n_seeds, n_regs, n_psel = (n[k] for k in ("n_smem", "n_pos", "n_chains", "n_seeds", "n_regs", "n_psel"))
    t_all, all_xs, times = T.time_steps(st, s, args)
    N.profile_begin()
    sm.run(s)
    torch.cuda.synchronize()
    kernels = {k: round(float(v[0]), 3) for k, v in N.profile_end().items() if k.startswith("mem_sam")}
    torch.cuda.synchronize()
    got = sm.results()
    pinned = torch.empty(got["n_text"], dtype=torch.uint8, pin_memory=True)
    t_down, down_xs = T.median_ms(lambda: pinned.copy_(sm.lines[:got["n_text"]], non_blocking=True), args.reps, 1, s)
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
    return T.emit(out, args.out, ok)


if __name__ == "__main__":
    sys.exit(main())
