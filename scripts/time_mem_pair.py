"""Times read pairs -> paired alignment records on one stream on the fmi 'large' shape (device events, warm-up, median of N) and
prints one JSON line: gbx_fmi_smem_device, gbx_fmi_sal_device, gbx_mem_chain_device, gbx_bsw_extend_seeds_device,
gbx_mem_regs_device, gbx_mem_pair_device and gbx_mem_cigar_device queued back to back on simulated FR pairs (interleaved reads,
read_id0 = 2 pair_id0).  Each stage's device time and the whole chain's; the paired-end stage is to be read against the regs
stage of the same run (both are serial per unit with lanes across a list).  A sizing pass first learns the counts, so the timed
passes run with tight capacities and no host synchronisation inside.  The first pairs are checked against tests/mem_pair_ref.py
under the call's own estimate (given to the reference as pes_in: the estimate is a reduction over the whole call).

    python scripts/time_mem_pair.py [--reads 200000] [--reps 10] [--out profiles/mem_pair_time.json]
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
from genomicsbench_amd import mem_pair as MP  # noqa: E402
from genomicsbench_amd import mem_regs as MR  # noqa: E402


def gen_pairs(g, n_pairs, seed, length=151, mean=350., sd=35.):
    """n_pairs FR fragments of g as interleaved reads: the fragment's first `length` bases, then the reverse complement of its
    last ones, each with about 1 % substitutions."""
    rng = np.random.default_rng(seed)
    frag = np.maximum(length + 20, np.rint(rng.normal(mean, sd, n_pairs)).astype(np.int64))
    at = rng.integers(0, len(g) - frag.max(), n_pairs)
    col = np.arange(length)
    fwd = g[at[:, None] + col]
    rev = 3 - g[(at + frag)[:, None] - 1 - col]
    reads = np.empty((2 * n_pairs, length), dtype=np.uint8)
    reads[0::2], reads[1::2] = fwd, rev
    hit = rng.random(reads.shape) < 0.01
    reads[hit] = (reads[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    return FM.FmiReadSet.fixed(reads)


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
    ap.add_argument("--check", type=int, default=2000, help="pairs that are checked against the restated rules")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_pair_time.json"))
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    import mem_pair_ref as R
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    g = gen_fmi_genome(args.genome, args.seed)
    idx, smp = FM.build_index(g, device=dev, sa_compx=3)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    build_s = time.perf_counter() - t0
    rs = gen_pairs(g, args.reads // 2, args.seed + 1)
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
    pe = MP.DeviceMemPair(rg, pp, psel_cap=n_regs + 64)
    rg.run(s)
    pe.run(s)
    torch.cuda.synchronize()
    n_psel = pe.results()["n_psel"]
    pe = MP.DeviceMemPair(rg, pp, psel_cap=n_psel + 64)
    cg = MG.DeviceMemCigar(pe.cigar_input, cp, cigar_cap=8 * pe.psel_cap, z_bytes=n_psel * per_record)

    def whole():
        d.run(s)
        d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s)
        mc.run(s)
        ext.run(sp, s)
        rg.run(s)
        pe.run(s)
        cg.run(s)
    t_all, all_xs = median_ms(whole, args.reps, args.warmup, s)
    t_smem, _ = median_ms(lambda: d.run(s), args.reps, 1, s)
    t_sal, _ = median_ms(lambda: d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s), args.reps, 1, s)
    t_chain, _ = median_ms(lambda: mc.run(s), args.reps, 1, s)
    t_ext, _ = median_ms(lambda: ext.run(sp, s), args.reps, 1, s)
    t_rg, rg_xs = median_ms(lambda: rg.run(s), args.reps, 1, s)
    t_pe, pe_xs = median_ms(lambda: pe.run(s), args.reps, 1, s)
    t_cg, cg_xs = median_ms(lambda: cg.run(s), args.reps, 1, s)
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
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
