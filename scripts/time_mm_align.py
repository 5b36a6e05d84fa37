#!/usr/bin/env python3
"""Times the base-level alignment stage (genomicsbench_amd.mm_align) on the input of scripts/time_mm_seed.py and writes one JSON
line to profiles/mm_align_time.json:

  seeding, chain, map   gbx_mm_seed_device, gbx_chain_device and gbx_mm_map_device, re-measured in this run (device events)
  align                 gbx_mm_align_device, split by the library's stage timers into planning (validity, jobs, the two scans), DP
                        (a wavefront a job) and packing (placing, the scan, words, statistics and records); cells per second over
                        the cells the jobs' bands hold
  paf                   gbx_mm_paf_cigar_device: the text with cg:Z:
  rows_ab               the DP with its rows in LDS against in the job's room, alternated in the same run
  cpu                   the same rules (mm_align_rules.h built for the host, libgbx_mm_cpu.so) on the first --cpu-reads reads, one
                        thread; its records and words must equal the device's

--preset large = --genome 67108864 --reads 4000 --read-len 10000.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def band_cells(tl, ql, w):
    """the cells of a job: antidiagonal r holds t in [max(0, r - ql + 1, (r - w + 1) >> 1), min(tl - 1, r, (r + w) >> 1)]"""
    w = min(w, tl + ql)
    r = np.arange(tl + ql - 1, dtype=np.int64)
    st = np.maximum(np.maximum(0, r - ql + 1), (r - w + 1) >> 1)
    en = np.minimum(np.minimum(tl - 1, r), (r + w) >> 1)
    return int(np.maximum(en - st + 1, 0).sum())


def planned_cells(P, regs, reg_off, off, cax, cay, seq_off, tseq_off):
    """rules 2-5 on the host: the cells of every region's jobs (an extension that is z-dropped stops short of its share)"""
    total = jobs = 0
    for r in range(len(reg_off) - 1):
        qlen = int(seq_off[r + 1] - seq_off[r])
        for g in regs[reg_off[r]:reg_off[r + 1]]:
            a0 = int(off[r]) + int(g["as"])
            x = (cax[a0:a0 + g["cnt"]] & 0xffffffff).astype(np.int64)
            y = (cay[a0:a0 + g["cnt"]] & 0xffffffff).astype(np.int64)
            sp = (cay[a0:a0 + g["cnt"]] >> 32 & 0xff).astype(np.int64)
            tlen = int(tseq_off[g["rid"] + 1] - tseq_off[g["rid"]])
            rs, qs = int(x[0] + 1 - sp[0]), int(y[0] + 1 - sp[0])
            re, qe = rs, qs
            lq = min(qs, P.max_ext)
            lt = min(rs, lq + P.bw)
            todo = [(lt, lq, P.bw)]
            for i in range(1, len(x)):
                re, qe = max(int(x[i] - (sp[i] >> 1)), rs), max(int(y[i] - (sp[i] >> 1)), qs)
                if i == len(x) - 1 or (re - rs >= P.min_ksw_len and qe - qs >= P.min_ksw_len):
                    todo.append((re - rs, qe - qs, max(P.bw, abs((re - rs) - (qe - qs)) + 1)))
                    rs, qs = re, qe
            lq = min(qlen - qe, P.max_ext)
            todo.append((min(tlen - re, lq + P.bw), lq, P.bw))
            for tl, ql, w in todo:
                if tl > 0 and ql > 0:
                    total += band_cells(tl, ql, w)
                    jobs += 1
    return total, jobs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", choices=["large"])
    ap.add_argument("--genome", type=int, default=1 << 22)
    ap.add_argument("--reads", type=int, default=400)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-reads", type=int, default=40, help="the reads the host build of the rules aligns (one thread)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mm_align_time.json"))
    a = ap.parse_args()
    if a.preset == "large":
        a.genome, a.reads, a.read_len = 1 << 26, 4000, 10000
    import torch
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import mm_align as MA
    from genomicsbench_amd import mm_map as MM
    from genomicsbench_amd import mm_seed as MS
    from time_mm_seed import make_inputs
    if not torch.cuda.is_available() or N.device_count() < 1:
        sys.exit("time_mm_align.py needs a GPU")
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    p = MS.make_params()
    refs, reads = make_inputs(a.genome, a.reads, a.read_len, a.seed)
    timer = N.StreamTimer()

    def timed(fn, reps):
        fn()                                                         # the warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            timer.start(s)
            fn()
            timer.stop(s)
            torch.cuda.synchronize()
            ms.append(timer.elapsed_ms())
        return min(ms), ms

    ix = MS.DeviceMmIndex(p, refs, dev, s, mini_cap=max(a.genome // 4, 1024))
    sd = MS.DeviceMmSeeder(ix, reads, mini_cap=max(sum(len(r) for r in reads) // 4, 1024), anchor_cap=1024)
    sd.run(s)
    n_mini, n_anchor = sd.counts()
    sd = MS.DeviceMmSeeder(ix, reads, mini_cap=n_mini, anchor_cap=max(n_anchor, 1))
    mp = MM.DeviceMmMapper(sd)
    mp.run(s)
    n_chain, n_reg, _ = mp.counts()
    assert mp.fits()
    # sized by runs that report the needs: the jobs' room first (every region flag 32), then the words, then the text
    mp = MM.DeviceMmMapper(sd, chain_cap=max(n_chain, 1), reg_cap=max(n_reg, 1), text_cap=1, align=True)
    al = mp.aligner
    al.caps = (1, 16, 1)
    mp.run(s)
    z_need = al.counts()[2]
    al.caps, al.sized_for = (1, z_need, 1), None
    al.run(s)
    n_jobs, n_words, z2, _ = al.counts()
    assert z2 == z_need
    al.caps, al.sized_for = (max(n_words, 1), z_need, 1), None
    al.run(s)
    n_text = al.counts()[3]
    al.caps, al.sized_for = (max(n_words, 1), z_need, max(n_text, 1)), None
    al.run(s)
    assert al.fits() and al.counts() == (n_jobs, n_words, z_need, n_text)
    seed_ms, seed_all = timed(lambda: sd.run(s), a.repeats)
    chain_ms, chain_all = timed(lambda: mp.cb.run(s), a.repeats)
    map_ms, map_all = timed(lambda: mp.run_map(s), a.repeats)
    align_ms, align_all = timed(lambda: al.run_align(s), a.repeats)
    paf_ms, paf_all = timed(lambda: al.run_paf(s), a.repeats)
    stages = {}
    for _ in range(a.repeats):                                       # the parts: best of the repeats each, after the warm-ups above
        N.profile_begin()
        al.run_align(s)
        torch.cuda.synchronize()
        prof = N.profile_end()
        for k in ("mm_align_plan", "mm_align_dp", "mm_align_pack"):
            if k in prof:
                stages[k] = min(stages.get(k, 1e30), prof[k][0])
    stage = lambda name: round(stages[name], 3) if name in stages else None
    # ---- the DP with its rows in LDS against in the job's room (GBX_MM_ALIGN_LDS=0, read per call), alternated
    ab = {"lds": [], "room": []}
    for _ in range(a.repeats):
        for name, env in (("lds", "1"), ("room", "0")):
            os.environ["GBX_MM_ALIGN_LDS"] = env
            N.profile_begin()
            al.run_align(s)
            torch.cuda.synchronize()
            ab[name].append(round(N.profile_end()["mm_align_dp"][0], 3))
    del os.environ["GBX_MM_ALIGN_LDS"]
    got = mp.results()
    regs, alns = got["regs"], got["alns"]
    P = al.p
    seq_off, tseq_off, off = sd.seq_off.cpu().numpy(), ix.off.cpu().numpy(), sd.off.cpu().numpy()
    cells, dp_jobs = planned_cells(P, regs, got["reg_off"], off, got["cax"], got["cay"], seq_off, tseq_off)
    # ---- the host build of the same rules on the first reads
    k = min(a.cpu_reads, a.reads)
    nr, na = int(got["reg_off"][k]), int(off[k])
    t0 = time.perf_counter()
    cpu = MA.align_cpu(P, regs[:nr], got["reg_off"][:k + 1], off[:k + 1], got["cax"][:na], got["cay"][:na], got["n_chained"][:k], reads[:k], refs)
    cpu_s = time.perf_counter() - t0
    assert cpu["alns"].tobytes() == alns[:nr].tobytes() and np.array_equal(cpu["cigar"], got["cigar"][:len(cpu["cigar"])]), \
        "the host build of the rules and the device disagree"
    cpu_cells, _ = planned_cells(P, regs[:nr], got["reg_off"][:k + 1], off[:k + 1], got["cax"], got["cay"], seq_off, tseq_off)
    aligned = (alns["flags"] & 1) > 0
    dp_ms = stages.get("mm_align_dp", align_ms)
    path = seed_ms + chain_ms + map_ms + align_ms + paf_ms
    rec = dict(what="base-level alignment of the regions beside seeding, chain and map in the same run; device events, a warm-up, best of the repeats",
               genome_bp=a.genome, reads=a.reads, read_len=a.read_len, seed=a.seed, anchors=n_anchor, regions=n_reg,
               seeding=dict(ms=round(seed_ms, 3), ms_all=[round(x, 3) for x in seed_all]),
               chain=dict(ms=round(chain_ms, 3), ms_all=[round(x, 3) for x in chain_all]),
               map=dict(ms=round(map_ms, 3), ms_all=[round(x, 3) for x in map_all]),
               align=dict(ms=round(align_ms, 3), ms_all=[round(x, 3) for x in align_all], plan_ms=stage("mm_align_plan"), dp_ms=stage("mm_align_dp"),
                          pack_ms=stage("mm_align_pack"), jobs=n_jobs, dp_jobs=dp_jobs, cells=cells, gcells_per_s=round(cells / (dp_ms * 1e-3) / 1e9, 3),
                          cigar_words=n_words, z_bytes=z_need, workspace_bytes=int(al.work_bytes), aligned=int(aligned.sum()),
                          zdropped=int(((alns["flags"] & 6) > 0).sum()), nm_per_kb=round(1000.0 * float(alns["nm"][aligned].sum()) / max(int(alns["blen"][aligned].sum()), 1), 2)),
               rows_ab=dict(what="mm_align_dp with the rows in LDS against in the job's room (GBX_MM_ALIGN_LDS=0), alternated; ms", lds_ms=ab["lds"],
                            room_ms=ab["room"], lds_median=float(np.median(ab["lds"])), room_median=float(np.median(ab["room"]))),
               paf=dict(ms=round(paf_ms, 3), ms_all=[round(x, 3) for x in paf_all], bytes=n_text),
               share_of_path=round(align_ms / path, 3),
               bound=max((("seeding", seed_ms), ("chain", chain_ms), ("map", map_ms), ("align", align_ms), ("paf", paf_ms)), key=lambda kv: kv[1])[0],
               cpu=dict(what="mm_align_rules.h on the host, one thread, the first reads' regions; records and words equal to the device's", reads=k,
                        regions=nr, cells=cpu_cells, align_s=round(cpu_s, 3), gcells_per_s=round(cpu_cells / cpu_s / 1e9, 4),
                        device_speedup_per_cell=round((cells / (align_ms * 1e-3)) / (cpu_cells / cpu_s), 1)),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
