"""Times reads -> extension results on one stream on the fmi 'large' shape (device events, warm-up, median of N) and prints one
JSON line: the 512-Mbp genome of bench.py's fmi job, its index built on the GPU with 1-in-8 suffix-array samples, --reads
reads; gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device and gbx_bsw_extend_seeds_device queued back to back.
Each stage's device time, the whole chain's, and the chaining stage's compulsory bytes (what it must read and write once)
against the HBM roofline.  A sizing pass first learns the counts, so the timed passes run with tight capacities and no
host synchronisation inside.  A sample of reads is checked against tests/mem_chain_ref.py.

    python scripts/time_mem_chain.py [--reads 200000] [--reps 10] [--out profiles/mem_chain_time.json]
"""
import sys

import numpy as np

import _mem_timing as T

HBM_GBS = 8000.0            # MI355X peak HBM3E bandwidth, GB/s


def main():
    ap = T.parser("mem_chain_time.json")
    ap.add_argument("--check", type=int, default=300, help="reads checked against the restated rules")
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_reads
    from genomicsbench_amd.mem_chain import text_of
    import mem_chain_ref as R
    dev, s, g, idx, smp, build_s = T.setup(args)
    rs = gen_fmi_reads(g, args.reads, args.seed + 1)
    L = len(g)
    st, n = T.sized_stages(idx, smp, rs, torch.from_numpy(text_of(g)).to(dev), L, dev, s, args, last="extend")
    d, mc, ext = st.fmi, st.chain, st.extend
    n_smem, n_pos, n_chains, n_seeds = n["n_smem"], n["n_pos"], n["n_chains"], n["n_seeds"]
    t_all, all_xs, times = T.time_steps(st, s, args, last="extend")
    (t_smem, _), (t_sal, _), (t_chain, chain_xs), (t_ext, _) = (times[k] for k in ("smem", "sal", "chain", "extend"))
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
    return T.emit(out, args.out, ok)


if __name__ == "__main__":
    sys.exit(main())
