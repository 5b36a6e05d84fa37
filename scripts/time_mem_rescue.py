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
from genomicsbench_amd import mem_rescue as MS  # noqa: E402


def gen_pairs(g, n_pairs, seed, mutated, length=151, mean=350., sd=35.):
    """n_pairs FR fragments of g as interleaved reads: the fragment's first `length` bases, then the reverse complement of its
    last ones, each with about 1 % substitutions; a fraction `mutated` of the mates has a substitution every 15 bases on top.
    -> (reads, the mutated pairs)."""
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
    which = np.nonzero(rng.random(n_pairs) < mutated)[0]
    reads[2 * which[:, None] + 1, np.arange(7, length, 15)] += 1
    reads %= 4
    return FM.FmiReadSet.fixed(reads), which


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
    ap.add_argument("--mutated", type=float, default=0.1, help="fraction of the mates that hold no exact 19-mer")
    ap.add_argument("--check", type=int, default=300, help="pairs that are checked against the restated rules")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_rescue_time.json"))
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    import mem_rescue_ref as R
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
    stages = [("smem", lambda: d.run(s)), ("sal", lambda: d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s)), ("chain", lambda: mc.run(s)),
              ("extend", lambda: ext.run(sp, s)), ("regs", lambda: rg.run(s)), ("rescue", lambda: rsc.run(s)), ("pair", lambda: pe.run(s)),
              ("cigar", lambda: cg.run(s))]

    def whole():
        for _, fn in stages:
            fn()
    t_all, all_xs = median_ms(whole, args.reps, args.warmup, s)
    times = {name: median_ms(fn, args.reps, 1, s) for name, fn in stages}
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
    want = R.rescue_all(regs_out["regs"][:off[-1]], off, seeds, ch["l_rep"], rs.read_off, rs.read_len, MC.text_of(g), rs.enc, L,
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
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
