"""Times read pairs -> paired alignment records with mate rescue on one stream on the fmi 'large' shape (device events, warm-up,
median of N) and prints one JSON line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device,
gbx_mem_regs_device, gbx_mem_pestat_device + gbx_mem_rescue_device, gbx_mem_pair_device and gbx_mem_cigar_device queued back to
back on simulated FR pairs (interleaved reads, read_id0 = 2 pair_id0).  A fraction of the mates is mutated until they hold no
exact 19-mer (a substitution every 15 bases), so they get no seed and only the rescue places them.  Each stage's device time and
the whole chain's; the rescue's SW kernel (stage mem_rescue_sw of the profile) is to be read against the extension of the same
run: both as nominal cells per second, the rescue's cells being rows x columns of every SW whose answer was used (from the
per-pair stats and the estimate's window), the extension's lq x rlen of every seed.  A sizing pass first learns the counts.  The
paired stage gets the sizing pass's estimate as pes_in, so no copy lies inside the timed passes.

    python scripts/time_mem_rescue.py [--reads 200000] [--mutated 0.1] [--reps 10] [--out profiles/mem_rescue_time.json]
"""
import sys

import numpy as np

import _mem_timing as T
from genomicsbench_amd import _native as N
from genomicsbench_amd import bsw_seeds as BS


def main():
    ap = T.parser("mem_rescue_time.json")
    ap.add_argument("--mutated", type=float, default=0.1, help="fraction of the mates that hold no exact 19-mer")
    ap.add_argument("--check", type=int, default=300, help="pairs that are checked against the restated rules")
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.mem_chain import text_of
    import mem_rescue_ref as R
    dev, s, g, idx, smp, build_s = T.setup(args)
    rs, mutated = T.gen_pairs(g, args.reads // 2, args.seed + 1, args.mutated)
    L = len(g)
    text_np = text_of(g)
    st, n = T.sized_stages(idx, smp, rs, torch.from_numpy(text_np).to(dev), L, dev, s, args, last="cigar")
    mc, rg, rsc, pe, cg, pes = st.chain, st.regs, st.rescue, st.pair, st.cigar, st.pes_in
    n_smem, n_pos, n_chains, n_seeds, n_regs, n_psel = (n[k] for k in ("n_smem", "n_pos", "n_chains", "n_seeds", "n_regs", "n_psel"))
    t_all, all_xs, times = T.time_steps(st, s, args, last="cigar")
    N.profile_begin()
    rsc.run(s)
    torch.cuda.synchronize()
    sw_ms = float(N.profile_end().get("mem_rescue_sw", (0., 0))[0])
    torch.cuda.synchronize()
    got = rsc.results()
    pr = pe.results()["pairs"]
    alns, cigar = cg.results()
    # nominal cells: the rescue's SWs have (read length) rows and (high - low + read length) columns before clamping
    fr = pes[1]
    length = int(rs.read_len[0])
    sw_cells = float(got["stats"]["n_sw"].sum()) * length * (int(fr["high"]) - int(fr["low"]) + length)
    ch = mc.results()
    ext_cells = float((ch["seeds"]["lq"].astype(np.int64) * ch["seeds"]["rlen"]).sum())
    # the first pairs against the restated rules, under the call's own estimate
    k = min(args.check, rs.n_reads // 2)
    regs_out = rg.results()
    off = regs_out["reg_off"][:2 * k + 1]
    seeds = np.zeros(mc.seed_cap, dtype=BS.SEED_DTYPE)
    seeds[:len(ch["seeds"])] = ch["seeds"]
    want = R.rescue_all(regs_out["regs"][:off[-1]], off, seeds, ch["l_rep"], rs.read_off, rs.read_len, text_np, rs.enc, L,
                        np.array([0, L]), pes, R.params(), 0, seed_cap=mc.seed_cap)
    m = want["n_xregs"]
    ok = bool(got["stats"][:k].tobytes() == want["stats"].tobytes() and
              got["xregs"][:m][["rb", "re", "qb", "qe", "score", "csub", "mapq", "flag"]].tobytes() ==
              want["xregs"][["rb", "re", "qb", "qe", "score", "csub", "mapq", "flag"]].tobytes())
    out = {"what": "smem -> sal -> chain -> extend -> regs -> pestat + rescue -> pair -> cigar on one stream, fmi 'large' genome, simulated FR pairs",
           "genome_bp": args.genome, "reads": rs.n_reads, "pairs": rs.n_reads // 2, "mutated_mates": int(len(mutated)),
           "index_build_s": round(build_s, 1), "max_occ": args.max_occ, "smems": n_smem, "hits": n_pos, "chains": n_chains, "seeds": n_seeds,
           "regions": n_regs, "regions_after_rescue": got["n_xregs"], "active_pairs": int((got["stats"]["n_sw"] > 0).sum()),
           "sws": int(got["stats"]["n_sw"].sum()), "regions_added": int(got["stats"]["n_added"].sum()),
           "rescued_mates": int((got["stats"]["n_kept"][mutated] > 0).sum()), "rescued_regions_kept": int(got["stats"]["n_kept"].sum()),
           "pestat": [list(x) for x in pes[["low", "high", "failed", "avg", "std"]].tolist()], "paired": int(pr["paired"].sum()),
           "proper": int(pr["proper"].sum()), "proper_among_mutated": int(pr["proper"][mutated].sum()), "reported": n_psel,
           "cigar_words": int(len(cigar)), "records_without_room": int((alns["rid"] == -2).sum()),
           "boundary_inputs_in_the_checked_pairs": int(want["boundary"])}
    for name, (t, xs) in times.items():
        out[name + "_ms"], out[name + "_ms_all"] = round(t, 3), xs
    out.update({"whole_ms": round(t_all, 3), "whole_ms_all": all_xs, "rescue_sw_kernel_ms": round(sw_ms, 3),
                "rescue_sw_nominal_cells": sw_cells, "extend_nominal_cells": ext_cells,
                "rescue_sw_gcells_per_s": round(sw_cells / sw_ms / 1e6, 3) if sw_ms > 0 else None,
                "extend_gcells_per_s": round(ext_cells / times["extend"][0] / 1e6, 3),
                "checked_pairs": k, "checked_equal": ok, "device": torch.cuda.get_device_name(0)})
    return T.emit(out, args.out, ok)


if __name__ == "__main__":
    sys.exit(main())
