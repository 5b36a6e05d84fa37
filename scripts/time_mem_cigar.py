"""Times reads -> alignment records on one stream on the fmi 'large' shape (device events, warm-up, median of N) and prints one
JSON line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device and
gbx_mem_cigar_device queued back to back.  Each stage's device time and the whole chain's; the CIGAR stage is to be read
against the extension stage of the same run (both are O(band x length) per seed).  A sizing pass first learns the counts, so
the timed passes run with tight capacities and no host synchronisation inside.  A sample of records is checked against
tests/mem_cigar_ref.py.

    python scripts/time_mem_cigar.py [--reads 200000] [--reps 10] [--out profiles/mem_cigar_time.json]
"""
import sys

import numpy as np

import _mem_timing as T
from genomicsbench_amd import bsw_seeds as BS


def main():
    ap = T.parser("mem_cigar_time.json")
    ap.add_argument("--check", type=int, default=2000, help="records checked against the restated rules")
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_reads
    from genomicsbench_amd.mem_chain import text_of
    import mem_cigar_ref as R
    dev, s, g, idx, smp, build_s = T.setup(args)
    rs = gen_fmi_reads(g, args.reads, args.seed + 1)
    L = len(g)
    text_h = text_of(g)
    st, n = T.sized_stages(idx, smp, rs, torch.from_numpy(text_h).to(dev), L, dev, s, args, skip=("regs", "rescue", "pair"), last="cigar")
    mc, ext, cg = st.chain, st.extend, st.cigar
    n_smem, n_pos, n_chains, n_seeds, lq_max, lt_max = (n[k] for k in ("n_smem", "n_pos", "n_chains", "n_seeds", "lq_max", "lt_max"))
    z_bytes, per_record = cg.z_bytes, n["z_per_record"]
    res = ext.results()
    t_all, all_xs, times = T.time_steps(st, s, args, last="cigar")
    (t_smem, _), (t_sal, _), (t_chain, _), (t_ext, _), (t_cg, cg_xs) = (times[k] for k in ("smem", "sal", "chain", "extend", "cigar"))
    torch.cuda.synchronize()
    alns, cigar = cg.results()
    # the first records against the restated rules (the C twin)
    k = min(args.check, ext.n)
    seeds = mc.seeds.cpu().numpy().view(BS.SEED_DTYPE)[:k]
    want_a, want_c = R.run_c(R.params(), seeds, res[:k], text_h, rs.enc, L, [0, L])
    ok = bool(alns[:k].tobytes() == want_a.tobytes() and np.array_equal(cigar[:len(want_c)], want_c))
    out = {"what": "smem -> sal -> chain -> extend -> cigar on one stream, fmi 'large' genome", "genome_bp": args.genome,
           "reads": rs.n_reads, "index_build_s": round(build_s, 1), "max_occ": args.max_occ, "smems": n_smem, "hits": n_pos,
           "chains": n_chains, "seeds": n_seeds, "regions": n["n_extended"], "cigar_words": int(len(cigar)),
           "records_without_room": int((alns["rid"] == -2).sum()), "records_through_the_dp": int((alns["w"] > 0).sum()),
           "tries_histogram": np.bincount(alns["tries"], minlength=4).tolist(), "longest_query": lq_max, "longest_text": lt_max,
           "z_bytes": z_bytes, "z_bytes_per_record": per_record,
           "smem_ms": round(t_smem, 3), "sal_ms": round(t_sal, 3), "chain_ms": round(t_chain, 3), "extend_ms": round(t_ext, 3),
           "cigar_ms": round(t_cg, 3), "cigar_ms_all": cg_xs, "whole_ms": round(t_all, 3), "whole_ms_all": all_xs,
           "cigar_over_extend": round(t_cg / t_ext, 4), "checked_records": k, "checked_equal": ok,
           "device": torch.cuda.get_device_name(0)}
    return T.emit(out, args.out, ok)


if __name__ == "__main__":
    sys.exit(main())
