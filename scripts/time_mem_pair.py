"""Times read pairs -> paired alignment records on one stream on the fmi 'large' shape (device events, warm-up, median of N) and
prints one JSON line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device,
gbx_mem_regs_device, gbx_mem_pair_device and gbx_mem_cigar_device queued back to back on simulated FR pairs (interleaved reads,
read_id0 = 2 pair_id0).  Each stage's device time and the whole chain's; the paired-end stage is to be read against the regs
stage of the same run (both are serial per unit with lanes across a list).  A sizing pass first learns the counts, so the timed
passes run with tight capacities and no host synchronisation inside.  The first pairs are checked against tests/mem_pair_ref.py
under the call's own estimate (given to the reference as pes_in: the estimate is a reduction over the whole call).

    python scripts/time_mem_pair.py [--reads 200000] [--reps 10] [--out profiles/mem_pair_time.json]
"""
import sys

import numpy as np

import _mem_timing as T


def main():
    ap = T.parser("mem_pair_time.json")
    ap.add_argument("--check", type=int, default=2000, help="pairs that are checked against the restated rules")
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.mem_chain import text_of
    import mem_pair_ref as R
    dev, s, g, idx, smp, build_s = T.setup(args)
    rs, _ = T.gen_pairs(g, args.reads // 2, args.seed + 1)
    L = len(g)
    st, n = T.sized_stages(idx, smp, rs, torch.from_numpy(text_of(g)).to(dev), L, dev, s, args, skip=("rescue",), last="cigar")
    mc, rg, pe, cg = st.chain, st.regs, st.pair, st.cigar
    n_smem, n_pos, n_chains, n_seeds, n_regs, n_sel, n_psel = (n[k] for k in ("n_smem", "n_pos", "n_chains", "n_seeds", "n_regs", "n_sel", "n_psel"))
    t_all, all_xs, times = T.time_steps(st, s, args, last="cigar")
    (t_smem, _), (t_sal, _), (t_chain, _), (t_ext, _), (t_rg, rg_xs), (t_pe, pe_xs), (t_cg, cg_xs) = \
        (times[k] for k in ("smem", "sal", "chain", "extend", "regs", "pair", "cigar"))
    torch.cuda.synchronize()
    regs_out = rg.results()
    got = pe.results()
    alns, cigar = cg.results()
    # the first pairs against the restated rules, under the call's own estimate
    k = min(args.check, rs.n_reads // 2)
    ch = mc.results()
    off = regs_out["reg_off"][:2 * k + 1]
    pes = [tuple(x) for x in got["pes"][["low", "high", "failed", "avg", "std"]].tolist()]
    want = R.pair_all(regs_out["regs"][:off[-1]], off, regs_out["sel_seeds"], regs_out["sel_res"], ch["seeds"], ch["l_rep"][:2 * k], L,
                      np.array([0, L]), R.params(), 0, pes_in=pes, psel_cap=0)
    m = len(want["pregs"])
    ok = bool(got["pairs"][:k].tobytes() == want["pairs"].tobytes() and got["pregs"][:m].tobytes() == want["pregs"].tobytes())
    pr = got["pairs"]
    out = {"what": "smem -> sal -> chain -> extend -> regs -> pair -> cigar on one stream, fmi 'large' genome, simulated FR pairs",
           "genome_bp": args.genome, "reads": rs.n_reads, "pairs": rs.n_reads // 2, "index_build_s": round(build_s, 1), "max_occ": args.max_occ,
           "smems": n_smem, "hits": n_pos, "chains": n_chains, "seeds": n_seeds, "regions": n_regs, "reported_by_regs": n_sel,
           "reported": n_psel, "pestat": [list(x) for x in pes], "paired": int(pr["paired"].sum()), "proper": int(pr["proper"].sum()),
           "candidate_pairs": int(pr["n_cand"].sum()), "most_candidates_in_a_pair": int(pr["n_cand"].max()),
           "q_pe_histogram": np.bincount(pr["q_pe"], minlength=61).tolist(),
           "boundary_inputs_in_the_checked_pairs": int(want["boundary"]), "cigar_words": int(len(cigar)),
           "records_without_room": int((alns["rid"] == -2).sum()),
           "smem_ms": round(t_smem, 3), "sal_ms": round(t_sal, 3), "chain_ms": round(t_chain, 3), "extend_ms": round(t_ext, 3),
           "regs_ms": round(t_rg, 3), "regs_ms_all": rg_xs, "pair_ms": round(t_pe, 3), "pair_ms_all": pe_xs, "cigar_ms": round(t_cg, 3),
           "cigar_ms_all": cg_xs, "whole_ms": round(t_all, 3), "whole_ms_all": all_xs, "pair_over_regs": round(t_pe / t_rg, 4),
           "checked_pairs": k, "checked_equal": ok, "device": torch.cuda.get_device_name(0)}
    return T.emit(out, args.out, ok)


if __name__ == "__main__":
    sys.exit(main())
