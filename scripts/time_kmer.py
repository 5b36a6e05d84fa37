"""Times canonical k-mer counting on a kmer-cnt preset and prints one JSON line: the device-resident call (gbx_kmer_count_device
on reads already in HBM; device events, warm-up, median of --reps) at k = 15 and k = 17, the host entry (gbx_kmer_count_host,
host clock), and bin/kmer-cnt end to end on the preset written as FASTA (its own "Kernel time" and the wall time of the
process).  The count pass's kernel time (gbx_profile_*) is read against the random-atomic ceiling of profiles/atomic_peak.json.
The k = 15 result is checked against the host entry's.

    python scripts/time_kmer.py [--preset large] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import kmer as K  # noqa: E402
from genomicsbench_amd.datagen import gen_kmer_preset, write_fasta  # noqa: E402


def device_ms(d, reps):
    import torch
    d.run()
    torch.cuda.synchronize()
    tm = N.StreamTimer()
    xs = []
    for _ in range(reps):
        tm.start(None)
        d.run()
        tm.stop(None)
        torch.cuda.synchronize()
        xs.append(tm.elapsed_ms())
    N.profile_begin()
    d.run()
    torch.cuda.synchronize()
    prof = N.profile_end()
    return float(np.median(xs)), {k: round(v[0], 3) for k, v in prof.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    t0 = time.time()
    recs = gen_kmer_preset(a.preset)
    rs = K.KmerReadSet.from_records(recs, 5000)
    gen_s = time.time() - t0
    res = dict(preset=a.preset, reads=rs.n_reads, bases=rs.n_bases, gen_s=round(gen_s, 1))
    peak_path = os.path.join(ROOT, "profiles", "atomic_peak.json")
    peak = None
    if os.path.exists(peak_path):
        rows = json.load(open(peak_path))["rows"]
        peak = max(r.get("random", 0) for r in rows if r.get("table_mib") == 4096)
        res["atomic_peak_random_4gib_gadds"] = peak
    d = K.DeviceKmer(rs, "cuda:0", 15, n_hist=256, min_freq=0, sel_cap=0)
    for k in (15, 17):
        d.set_params(k, n_hist=256)
        ms, prof = device_ms(d, a.reps)
        npos = rs.n_positions(k)
        row = dict(positions=npos, device_ms=round(ms, 2), gkmers_per_s=round(npos / ms / 1e6, 3), kernels_ms=prof)
        if peak and prof.get("kmer_count"):
            rate = npos / (prof["kmer_count"] * 1e-3) / 1e9
            row["count_pass_gadds"] = round(rate, 3)
            row["count_pass_share_of_atomic_peak"] = round(rate / peak, 3)
        res["k%d" % k] = row
        if k == 15:
            dev15 = d.results()
    del d
    torch.cuda.empty_cache()
    K.count_host(rs, 15, n_hist=256)                                  # warm-up: lane, pinned buffers, the 4 GB table
    xs = []
    for _ in range(max(1, a.reps // 2)):
        t = time.time()
        host15 = K.count_host(rs, 15, n_hist=256)
        xs.append((time.time() - t) * 1e3)
    res["host_entry_k15_ms"] = round(float(np.median(xs)), 1)
    assert host15[0] == dev15[0] and np.array_equal(host15[1], dev15[1]), "host and device entries disagree"
    res["k15_stats"] = host15[0]
    N.lib().gbx_host_release()
    with tempfile.TemporaryDirectory() as td:
        fa = os.path.join(td, "reads.fasta")
        cfg = os.path.join(td, "k15.cfg")
        write_fasta(fa, recs)
        open(cfg, "w").write("kmer_size=15\nuse_minimizers=0\nassemble_kmer_sample=1\n")
        t = time.time()
        r = subprocess.run([os.path.join(ROOT, "genomicsbench_amd", "bin", "kmer-cnt"), "--reads", fa, "--config", cfg, "--threads", "16",
                            "--debug"], capture_output=True, text=True, timeout=900)
        wall = time.time() - t
        if r.returncode != 0:
            raise RuntimeError("kmer-cnt failed: %s" % r.stderr[-2000:])
        kt = float(re.search(r"Kernel time: ([0-9.]+) sec", r.stderr).group(1))
        tk = int(re.search(r"Total k-mers (\d+)", r.stderr).group(1))
        assert tk == host15[0]["n_distinct"], "driver and host entry disagree"
        res["driver"] = dict(kernel_time_s=kt, wall_s=round(wall, 2), threads=16)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
