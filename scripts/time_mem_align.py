"""Times ``mem_align.MemAligner.run`` box to box (host arrays in, SAM text in host memory out), batch by batch, on the inputs of
scripts/time_mem_sam.py (same genome, seeds and gen_pairs) cut into batches of 50 000 reads, and prints one JSON line.  The first
batch includes its reruns; from the second on the planner sizes from the batch before.  Per batch: wall milliseconds, reads per
second, the reruns and the stages they started from, capacity over need per stage, the bytes moved.  Beside it, in the same
process and on the first batch, the stage classes queued by hand as scripts/time_mem_sam.py queues them, with capacities a sizing
pass made tight: that chain's device time (whole_ms) and the time of its upload and of its download.  A steady-state batch is to
be read against whole_ms + upload_ms + download_ms: the gap is the price of the planner's margins, of the gather and of the
pinned staging copies.  The aligner's text of the first batch must equal the composed chain's.

    python scripts/time_mem_align.py [--reads 200000] [--batch 50000] [--genome 536870912] [--out profiles/mem_align_time.json]
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
from genomicsbench_amd import mem_align as MA  # noqa: E402
from genomicsbench_amd import mem_chain as MC  # noqa: E402
from genomicsbench_amd import mem_cigar as MG  # noqa: E402
from genomicsbench_amd import mem_pair as MP  # noqa: E402
from genomicsbench_amd import mem_regs as MR  # noqa: E402
from genomicsbench_amd import mem_rescue as MS  # noqa: E402
from genomicsbench_amd import mem_sam as SM  # noqa: E402
from time_mem_rescue import gen_pairs, median_ms  # noqa: E402

PAIRS = (("out_cap", "n_smem"), ("pos_cap", "n_pos"), ("chain_cap", "n_chains"), ("seed_cap", "n_seeds"), ("reg_cap", "n_regs"),
         ("sel_cap", "n_sel"), ("xreg_cap", "n_xregs"), ("xseed_cap", "n_xseeds"), ("xsel_cap", "n_xsel"), ("psel_cap", "n_psel"),
         ("cigar_cap", "n_cigar"), ("rec_cap", "n_recs"), ("md_cap", "n_md"), ("text_cap", "n_text"))


def composed(idx, smp, text_dev, rs, names, qual, L, args, dev, s):
    """scripts/time_mem_sam.py's chain on one batch: a sizing pass, tight capacities, then device events around the whole chain,
    around the upload of the batch and around the download of the text.  -> (dict, the text as bytes)."""
    import torch
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
    ext = mc.extension(text_dev)
    sp, rp, pp, cp = BS.make_seed_params(), MR.make_params(), MP.make_params(), MG.make_params()
    mc.run(s)
    ext.run(sp, s)
    rg = MR.DeviceMemRegs(ext, rp)
    rg.run(s)
    torch.cuda.synchronize()
    res, first = ext.results(), rg.results()
    rg = MR.DeviceMemRegs(ext, rp, reg_cap=first["n_regs"] + 64, sel_cap=first["n_sel"] + 64)
    regions = res[res[:, 2] >= 0]
    per_record = int(MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(cp), int((regions[:, 3] - regions[:, 2]).max()),
                                                            int((regions[:, 5] - regions[:, 4]).max())))
    rsc = MS.DeviceMemRescue(rg, MS.make_params(), pp)
    rg.run(s)
    rsc.run(s)
    torch.cuda.synchronize()
    sized = rsc.results()
    pes = sized["pes"]
    rsc = MS.DeviceMemRescue(rg, MS.make_params(), pp, xreg_cap=sized["n_xregs"] + 64, xseed_cap=sized["n_xseeds"] + 64, xsel_cap=sized["n_xsel"] + 64)
    pe = MP.DeviceMemPair(rsc, pp, pes_in=pes, psel_cap=sized["n_xregs"] + 64)
    rsc.run(s)
    pe.run(s)
    torch.cuda.synchronize()
    n_psel = pe.results()["n_psel"]
    pe = MP.DeviceMemPair(rsc, pp, pes_in=pes, psel_cap=n_psel + 64)
    cg = MG.DeviceMemCigar(pe.cigar_input, cp, cigar_cap=8 * pe.psel_cap, z_bytes=n_psel * per_record)
    sm = SM.DeviceMemSam(pe, cg, names, qual, ["genome"], max_recs=4, max_del=256)
    pe.run(s)
    cg.run(s)
    sm.run(s)
    torch.cuda.synchronize()
    nr, nm, nt = (int(x) for x in sm.counts.cpu().numpy())
    sm = SM.DeviceMemSam(pe, cg, names, qual, ["genome"], rec_cap=nr + 64, md_cap=nm + 64, text_cap=nt + 64)
    stages = [lambda: d.run(s), lambda: d.sal(args.max_occ, pos_cap=n_pos + 64, stream=s), lambda: mc.run(s), lambda: ext.run(sp, s),
              lambda: rg.run(s), lambda: rsc.run(s), lambda: pe.run(s), lambda: cg.run(s), lambda: sm.run(s)]

    def whole():
        for fn in stages:
            fn()
    t_all, all_xs = median_ms(whole, args.reps, args.warmup, s)
    torch.cuda.synchronize()
    got = sm.results()
    # the batch up (bases, offsets, lengths, qualities, names) and the text down, through pinned memory
    nm_arena, no = SM.arena(names)
    ups = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (rs.enc, rs.read_off, rs.read_len, qual, nm_arena, no)]
    dst = [torch.empty_like(u, device=dev) for u in ups]

    def up():
        for a, b in zip(dst, ups):
            a.copy_(b, non_blocking=True)
    t_up, up_xs = median_ms(up, args.reps, 1, s)
    pinned = torch.empty(got["n_text"] + got["n_recs"] * 112, dtype=torch.uint8, pin_memory=True)

    def down():
        pinned[:got["n_text"]].copy_(sm.lines[:got["n_text"]], non_blocking=True)
        pinned[got["n_text"]:].copy_(sm.recs[:got["n_recs"] * 112], non_blocking=True)
    t_down, down_xs = median_ms(down, args.reps, 1, s)
    torch.cuda.synchronize()
    out = {"whole_ms": round(t_all, 3), "whole_ms_all": all_xs, "upload_ms": round(t_up, 3), "upload_ms_all": up_xs,
           "download_ms": round(t_down, 3), "download_ms_all": down_xs, "upload_bytes": int(sum(u.numel() * u.element_size() for u in ups)),
           "download_bytes": int(pinned.numel()),
           "counts": {"n_smem": n_smem, "n_pos": n_pos, "n_chains": n_chains, "n_seeds": n_seeds, "n_regs": first["n_regs"], "n_psel": n_psel,
                      "n_recs": nr, "n_md": nm, "n_text": nt}}
    return out, got["lines"].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--batch", type=int, default=50_000)
    ap.add_argument("--genome", type=int, default=512 << 20)
    ap.add_argument("--seed", type=int, default=6001)
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mutated", type=float, default=0.1, help="fraction of the mates that hold no exact 19-mer")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_align_time.json"))
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.batch % 2 == 0 and args.reads % 2 == 0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    g = gen_fmi_genome(args.genome, args.seed)
    idx, smp = FM.build_index(g, device=dev, sa_compx=3)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    build_s = time.perf_counter() - t0
    rs, _ = gen_pairs(g, args.reads // 2, args.seed + 1, args.mutated)
    L = len(g)
    names = ["read%d" % (k // 2) for k in range(rs.n_reads)]
    qual = np.random.default_rng(args.seed + 2).integers(33, 74, len(rs.enc)).astype(np.uint8)
    text_np = MC.text_of(g)
    t0 = time.perf_counter()
    index = MA.MemIndex((idx, smp), np.array([0, L], dtype=np.int64), ["genome"], text=text_np)
    index_s = time.perf_counter() - t0
    al = MA.MemAligner(index)
    batches, first_text = [], None
    for k, lo in enumerate(range(0, rs.n_reads, args.batch)):
        hi = min(lo + args.batch, rs.n_reads)
        sub = rs.take(lo, hi)
        a0 = int(rs.read_off[lo])
        q = qual[a0:a0 + len(sub.enc)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = al.run(sub, names[lo:hi], q, id0=lo // 2)
        ms = (time.perf_counter() - t0) * 1e3
        if k == 0:
            first_text = got["sam"]
        st = got["stats"]
        over = {cap: round(st["caps"][cap] / max(st["counts"][cnt], 1), 2) for cap, cnt in PAIRS}
        batches.append({"reads": hi - lo, "ms": round(ms, 3), "reads_per_s": round((hi - lo) / ms * 1e3), "reruns": st["reruns"],
                        "rerun_stage": [MA.STAGES[x] for x in st["rerun_stage"]], "cap_over_need": over, "z_bytes": st["caps"]["z_bytes"],
                        "bytes_up": st["bytes_up"], "bytes_down": st["bytes_down"], "records": st["counts"]["n_recs"], "text_bytes": st["counts"]["n_text"]})
    # the steady state again, several times over one batch (the planner now sizes from a batch like it)
    lo, hi = 0, min(args.batch, rs.n_reads)
    sub = rs.take(lo, hi)
    q = qual[:len(sub.enc)]
    steady = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        al.run(sub, names[lo:hi], q, id0=0)
        steady.append(round((time.perf_counter() - t0) * 1e3, 3))
    al.close()
    comp, comp_text = composed(idx, smp, torch.from_numpy(text_np).to(dev), sub, names[lo:hi], q, L, args, dev, s)
    ok = bool(first_text == comp_text)
    box = comp["whole_ms"] + comp["upload_ms"] + comp["download_ms"]
    out = {"what": "MemAligner.run box to box per batch beside the hand-queued, tightly sized chain of scripts/time_mem_sam.py on the first batch",
           "genome_bp": args.genome, "reads": rs.n_reads, "batch_reads": args.batch, "read_length": int(rs.read_len[0]), "index_build_s": round(build_s, 1),
           "mem_index_create_s": round(index_s, 2), "batches": batches, "steady_ms_all": steady, "steady_ms": float(np.median(steady)),
           "steady_reads_per_s": round((hi - lo) / float(np.median(steady)) * 1e3), "composed": comp, "composed_box_ms": round(box, 3),
           "steady_over_composed_box": round(float(np.median(steady)) / box, 3), "first_batch_text_equal": ok, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
