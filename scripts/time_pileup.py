"""Times pileup on a generated preset: the device entries (layout and count, device-resident, HIP events), the host
entries and the driver's "Kernel runtime", on one GPU -> one JSON line (profiles/pileup_time_<preset>.json).
  python scripts/time_pileup.py --preset large [--reps 5] [--out file]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P_DT = ("r941", "r10")                            # the two DT:Z values of the generated reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--keep-bam")
    a = ap.parse_args()
    from genomicsbench_amd import pileup as P
    from genomicsbench_amd.datagen import gen_pileup_preset
    t = time.time()
    contigs, recs = gen_pileup_preset(a.preset, workers=a.threads)
    t_gen = time.time() - t
    d = tempfile.mkdtemp()
    bam = a.keep_bam or os.path.join(d, "p.bam")
    P.write_bam(bam, contigs, recs, threads=a.threads)
    del recs
    t_gen_write = time.time() - t
    name, clen = contigs[0]
    region = name
    import torch
    rs, (_, beg, end) = P.read_bam(bam, region, list(P_DT))
    nd, nh = 2, 5
    dev = P.DevicePileup(rs, "cuda:0", beg, end, nd, nh)
    s = torch.cuda.current_stream()
    dev.layout(s.cuda_stream)
    torch.cuda.synchronize()
    pc, st = dev.layout_results()
    dev.alloc_counts(st["n_cols"])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    lay, cnt = [], []
    for _ in range(a.reps + 1):
        ev[0].record(s)
        dev.layout(s.cuda_stream)
        ev[1].record(s)
        dev.count(stream=s.cuda_stream)
        ev[2].record(s)
        torch.cuda.synchronize()
        lay.append(ev[0].elapsed_time(ev[1]))
        cnt.append(ev[1].elapsed_time(ev[2]))
    lay, cnt = sorted(lay[1:]), sorted(cnt[1:])
    F = P.n_features(nd, nh)
    out_bytes = st["n_cols"] * F * 4 + st["n_cols"] * 8
    host = []
    for _ in range(2):
        t = time.time()
        P.pileup_host(rs, beg, end, nd, nh)
        host.append((time.time() - t) * 1000)
    del dev
    torch.cuda.empty_cache()
    exe = os.path.join(ROOT, "genomicsbench_amd", "bin", "pileup")
    r = subprocess.run([exe, bam, region, str(a.threads)] + list(P_DT), capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    kr = [float(ln.split()[2]) for ln in r.stderr.splitlines() if ln.startswith("Kernel runtime:")][0]
    hbm = 8.0e12 * 0.6                               # the write bound: ~60 % of the 8 TB/s peak reachable by streaming stores
    res = dict(preset=a.preset, contig_len=clen, reads=rs.n_reads, bases=rs.n_bases, aligned_bases=st["aligned_bases"],
               n_cols=st["n_cols"], max_ins=st["max_ins"], max_depth=st["max_depth"], num_dtypes=nd, num_homop=nh, features=F,
               layout_ms=round(lay[len(lay) // 2], 3), count_ms=round(cnt[len(cnt) // 2], 3),
               count_ms_min=round(cnt[0], 3), host_entry_ms=round(min(host), 1), driver_kernel_runtime_s=kr,
               aligned_bases_per_s_count=round(st["aligned_bases"] / (cnt[len(cnt) // 2] / 1e3)),
               output_bytes=out_bytes, write_bound_ms_at_4p8TBps=round(out_bytes / hbm * 1e3, 3),
               count_vs_write_bound=round(cnt[len(cnt) // 2] / (out_bytes / hbm * 1e3), 2),
               gen_s=round(t_gen, 1), gen_and_write_s=round(t_gen_write, 1), driver_stderr=r.stderr.strip().splitlines()[-3:])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
