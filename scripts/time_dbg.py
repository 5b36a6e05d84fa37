"""Times dbg on one preset: the device build (gbx_dbg_build_device, median of --reps), occurrences/s, the host entry on 1
and on --gpus N devices, the driver's Kernel runtime, and the digests of a seeded sample of windows against the
restatement (tests/dbg_ref.py).  Prints one JSON line and writes it to profiles/dbg_time_<preset>.json, or, with the preset's
contig length overridden, to profiles/dbg_time_<preset>_len<N>.json (the record says so too).
    python scripts/time_dbg.py --preset large [--contig-len N] [--gpus N] [--reps 5] [--sample 8] [--keep DIR]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="large")
    ap.add_argument("--contig-len", type=int, default=0, help="override the preset's contig length")
    ap.add_argument("--gpus", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", default=None, help="write the BAM and FASTA into this directory (kept: a profiler run can reuse them)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import dbg_ref as R
    from genomicsbench_amd import _native as N, dbg as D, pileup as P
    from genomicsbench_amd.datagen import DBG_PRESETS, gen_dbg_reads
    pr = dict(DBG_PRESETS[a.preset])
    if a.contig_len:
        pr["contig_len"] = a.contig_len
    t = time.time()
    c, recs, fa = gen_dbg_reads(pr["contig_len"], pr["coverage"], pr["seed"])
    print("generated %d records in %.1f s" % (len(recs), time.time() - t), flush=True)
    d = a.keep or tempfile.mkdtemp()
    os.makedirs(d, exist_ok=True)
    bam, fasta = os.path.join(d, "d.bam"), os.path.join(d, "d.fa")
    P.write_bam(bam, c, recs)
    with open(fasta, "wb") as f:
        f.write(fa)
    del recs
    rs, (ctg, beg, end), _ = D.read_bam(bam, c[0][0])
    seq = D.read_fasta(fasta)[ctg]
    wins = D.make_windows(rs, beg, end, seq)
    t_gen = time.time() - t
    print("ingest done: %d reads, %d windows, %.1f s" % (rs.n_reads, wins.n_win, t_gen), flush=True)
    dd = D.DeviceDbg(rs, wins, "cuda:0")
    s = torch.cuda.current_stream()
    ms = []
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        dd.build(s.cuda_stream)
        e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    dev_ms = float(np.median(ms[1:]))
    st = dd.results()
    occ = int(st["n_occ"].sum())
    slots = int(wins.occ_slots(rs, 15).sum())
    out = dict(preset=a.preset, contig_len=pr["contig_len"], contig_len_overridden=bool(a.contig_len), coverage=pr["coverage"], reads=rs.n_reads, windows=wins.n_win, occurrences=occ,
               occurrence_slots=slots, device_ms=round(dev_ms, 3), device_ms_all=[round(x, 3) for x in ms[1:]],
               occ_per_s=round(occ / (dev_ms / 1e3), 1), workspace_bytes=int(dd.work_bytes), gen_s=round(t_gen, 1))
    for ng in sorted({1, a.gpus} - {0}):
        N.lib().gbx_host_set_devices(ng)
        D.build_host(rs, wins)
        t = time.time()
        hst = D.build_host(rs, wins)
        out["host_ms_%dgpu" % ng] = round((time.time() - t) * 1e3, 3)
        assert np.array_equal(hst, st), "host entry on %d devices differs from the device entry" % ng
    N.lib().gbx_host_set_devices(1)
    res = subprocess.run([os.path.join(ROOT, "genomicsbench_amd", "bin", "dbg"), bam, ctg, fasta, "16"], capture_output=True, timeout=900)
    m = re.search(rb"Kernel runtime: ([0-9.]+) s", res.stderr)
    out["driver_kernel_runtime_s"] = float(m.group(1)) if m else None
    rng = np.random.default_rng(7)
    sample = sorted(rng.choice(wins.n_win, size=min(a.sample, wins.n_win), replace=False).tolist())
    ok = 0
    for w in sample:
        _, want = R.graph(wins.window_ref(w), int(wins.ref_pos[w]), [rs.read(r) for r in range(wins.read_lo[w], wins.read_hi[w])])
        ok += all(int(st[w][f]) == want[f] for f in R.STATS_FIELDS)
    out["sample_windows"] = sample
    out["sample_verified"] = "%d/%d" % (ok, len(sample))
    line = json.dumps(out)
    print(line)
    name = "dbg_time_%s.json" % a.preset if not a.contig_len else "dbg_time_%s_len%d.json" % (a.preset, a.contig_len)
    path = a.out or os.path.join(ROOT, "profiles", name)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 0 if ok == len(sample) else 1


if __name__ == "__main__":
    sys.exit(main())
