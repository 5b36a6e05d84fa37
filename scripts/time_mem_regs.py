"""Times reads -> one record per reported alignment on one stream on the fmi 'large' shape (device events, warm-up, median of N)
and prints one JSON line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device,
gbx_mem_regs_device and gbx_mem_cigar_device queued back to back.  Each stage's device time and the whole chain's; the regions
stage is to be read against the chain stage of the same run (both are serial per read with lanes across a list), and the CIGAR
stage on the reported regions against the CIGAR stage on all seeds (as scripts/time_mem_cigar.py runs it), which is timed
beside it.  A sizing pass first learns the counts, so the timed passes run with tight capacities and no host synchronisation
inside.  The regions of the first reads are checked against tests/mem_regs_ref.py.

    python scripts/time_mem_regs.py [--reads 200000] [--reps 10] [--out profiles/mem_regs_time.json]
"""
import sys

import numpy as np

import _mem_timing as T


def main():
    ap = T.parser("mem_regs_time.json")
    ap.add_argument("--check", type=int, default=2000, help="reads whose regions are checked against the restated rules")
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_reads
    from genomicsbench_amd.mem_chain import text_of
    from genomicsbench_amd.mem_cigar import DeviceMemCigar
    import mem_regs_ref as R
    dev, s, g, idx, smp, build_s = T.setup(args)
    rs = gen_fmi_reads(g, args.reads, args.seed + 1)
    st, n = T.sized_stages(idx, smp, rs, torch.from_numpy(text_of(g)).to(dev), len(g), dev, s, args, skip=("rescue", "pair"), last="cigar")
    mc, ext, rg, cg = st.chain, st.extend, st.regs, st.cigar
    n_smem, n_pos, n_chains, n_seeds, n_regs, n_sel = (n[k] for k in ("n_smem", "n_pos", "n_chains", "n_seeds", "n_regs", "n_sel"))
    res = ext.results()
    cg_all = DeviceMemCigar(ext, cg.params, cigar_cap=8 * ext.n, z_bytes=n["n_extended"] * n["z_per_record"])
    t_all, all_xs, times = T.time_steps(st, s, args, last="cigar")
    (t_smem, _), (t_sal, _), (t_chain, _), (t_ext, _), (t_rg, rg_xs), (t_cg, cg_xs) = (times[k] for k in ("smem", "sal", "chain", "extend", "regs", "cigar"))
    t_cg_all, _ = T.median_ms(lambda: cg_all.run(s), args.reps, 1, s)
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
           "chains": n_chains, "seeds": n_seeds, "extended_regions": n["n_extended"], "regions": n_regs, "reported": n_sel,
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
    return T.emit(out, args.out, ok)


if __name__ == "__main__":
    sys.exit(main())
