#!/usr/bin/env python3
"""Times the stage behind the chain scores (genomicsbench_amd.mm_map) on the input of scripts/time_mm_seed.py and writes one JSON
line to profiles/mm_map_time.json:

  seeding, chain   gbx_mm_seed_device and gbx_chain_device, re-measured in this run (device events)
  map              gbx_mm_map_device, split by the library's stage timers into backtrack (chain ends, walks, chain order) and
                   regions (mm_gen_regs, parents, selection, mapq, the copy into place)
  paf              gbx_mm_paf_device: the text
  cpu              the same rules (mm_map_rules.h built for the host, libgbx_mm_cpu.so) on the same chain scores, one thread; its
                   chains and regions must equal the device's
  mmpaf            with --mmpaf: bin/mmpaf on the same input written to files; its text must equal the device path's

--preset large = --genome 67108864 --reads 4000 --read-len 10000.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", choices=["large"])
    ap.add_argument("--genome", type=int, default=1 << 22)
    ap.add_argument("--reads", type=int, default=400)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mmpaf", action="store_true", help="also run bin/mmpaf on the input written to files")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mm_map_time.json"))
    a = ap.parse_args()
    if a.preset == "large":
        a.genome, a.reads, a.read_len = 1 << 26, 4000, 10000
    import torch
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import mm_map as MM
    from genomicsbench_amd import mm_seed as MS
    from time_mm_seed import make_inputs
    if not torch.cuda.is_available() or N.device_count() < 1:
        sys.exit("time_mm_map.py needs a GPU")
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    p = MS.make_params()
    refs, reads = make_inputs(a.genome, a.reads, a.read_len, a.seed)
    timer = N.StreamTimer()

    def timed(fn, reps):
        fn()
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
    mp.run(s)                                                # sizes from the anchor count; then capacities that just fit
    n_chain, n_reg, n_text = mp.counts()
    assert mp.fits()
    mp = MM.DeviceMmMapper(sd, chain_cap=max(n_chain, 1), reg_cap=max(n_reg, 1), text_cap=max(n_text, 1))
    mp.run(s)
    assert mp.fits() and mp.counts() == (n_chain, n_reg, n_text)
    seed_ms, seed_all = timed(lambda: sd.run(s), a.repeats)
    chain_ms, chain_all = timed(lambda: mp.cb.run(s), a.repeats)
    map_ms, map_all = timed(lambda: mp.run_map(s), a.repeats)
    paf_ms, paf_all = timed(lambda: mp.run_paf(s), a.repeats)
    N.profile_begin()
    mp.run_map(s)
    mp.run_paf(s)
    torch.cuda.synchronize()
    prof = N.profile_end()
    stage = lambda name: round(prof[name][0], 3) if name in prof else None
    got, text = mp.results(), mp.paf()
    # ---- the host build of the same rules on the device's chain scores
    seeds = sd.results()
    f, par, _, v = mp.cb.results()
    seq_off = sd.seq_off.cpu().numpy()
    hashes = [MM.read_hash(nm, int(ln)) for nm, ln in zip(mp.read_names, np.diff(seq_off))]
    t0 = time.perf_counter()
    cpu = MM.map_cpu(mp.p, seeds["off"], seeds["ax"], seeds["ay"], f, par, v, seq_off, seeds["rep_len"], hashes)
    cpu_s = time.perf_counter() - t0
    assert np.array_equal(cpu["u"], got["u"]) and cpu["regs"].tobytes() == got["regs"].tobytes(), "the host build of the rules and the device disagree"
    per_read = np.diff(seeds["off"])
    regs = got["regs"]
    pri = regs["parent"] == regs["id"]
    rec = dict(what="from chain scores to PAF: backtrack, regions + parents + mapq, text, beside seeding and chain in the same run; device events, "
                    "best of the repeats",
               genome_bp=a.genome, reads=a.reads, read_len=a.read_len, seed=a.seed, anchors=n_anchor, anchors_per_read_max=int(per_read.max()),
               seeding=dict(ms=round(seed_ms, 3), ms_all=[round(x, 3) for x in seed_all]),
               chain=dict(ms=round(chain_ms, 3), ms_all=[round(x, 3) for x in chain_all]),
               map=dict(ms=round(map_ms, 3), ms_all=[round(x, 3) for x in map_all], backtrack_ms=stage("mm_map_chains"), regions_ms=stage("mm_map_regs"),
                        chains=n_chain, regions=n_reg, primaries=int(pri.sum()), mapped_reads=int((np.diff(got["reg_off"]) > 0).sum()),
                        mapq60=int((regs["mapq"] == 60).sum()), workspace_bytes=int(mp.work_bytes)),
               paf=dict(ms=round(paf_ms, 3), ms_all=[round(x, 3) for x in paf_all], bytes=n_text, lines=text.count("\n")),
               share_of_path=round((map_ms + paf_ms) / (seed_ms + chain_ms + map_ms + paf_ms), 3),
               bound=max((("seeding", seed_ms), ("chain", chain_ms), ("map", map_ms), ("paf", paf_ms)), key=lambda kv: kv[1])[0],
               cpu=dict(what="mm_map_rules.h on the host, one thread, chains and regions of the same chain scores; equal to the device's",
                        map_s=round(cpu_s, 4), device_speedup=round(cpu_s / (map_ms * 1e-3), 1)),
               device=torch.cuda.get_device_name(0))
    if a.mmpaf:
        with tempfile.TemporaryDirectory() as d:
            fa, fq, out = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq"), os.path.join(d, "out.paf")
            with open(fa, "wb") as fh:
                for i, r in enumerate(refs):
                    fh.write(b">ref%d\n" % i + r + b"\n")
            with open(fq, "wb") as fh:
                for i, r in enumerate(reads):
                    fh.write(b"@read%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(ROOT, "genomicsbench_amd", "bin", "mmpaf"), "-o", out, fa, fq], capture_output=True, text=True)
            wall = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr
            same = open(out).read() == text
            rec["mmpaf"] = dict(wall_s=round(wall, 2), report=r.stderr.strip().splitlines()[-1], text_equals_device_path=same)
            assert same, "mmpaf's text differs from the device path's"
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
