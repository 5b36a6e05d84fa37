"""Times the kmer-cnt minimizer index on a kmer-cnt preset and prints one JSON line: the device-resident call
(gbx_kmer_index_device on reads already in HBM; device events, warm-up, median of --reps) with its time split into selection,
emit, sort and build (gbx_profile_*), the host entry (gbx_kmer_index_host, host clock), bin/kmer-cnt end to end on the preset
written as FASTA (its own "Kernel time" and the wall time of the process), and, in the same run, the single-thread host build of
the rules header (tests/hostcheck/kmer_index_check.cpp: hostcheck_ki_index).  The sort's traffic is stated next to its time: a
pass reads the digit's word for the histograms (8 B an item) and reads and writes both words in the scatter (32 B an item).
The device result is checked against the host entry's and the host build's.

    python scripts/time_kmer_index.py [--preset large] [--kmer 15] [--window 5] [--rate 10] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
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
from genomicsbench_amd import kmer_index as KI  # noqa: E402
from genomicsbench_amd.datagen import gen_kmer_preset, write_fasta  # noqa: E402


def host_build(rs, k, w, rate):
    """the rules header on one host thread -> (seconds, [chosen, distinct, repetitive frequency, selected, entries])"""
    src = os.path.join(ROOT, "tests", "hostcheck", "kmer_index_check.cpp")
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libkmer_index_check.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", so], check=True)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.hostcheck_ki_index.argtypes = [vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_float, vp, C.POINTER(C.c_float), vp, vp, vp]
        L.hostcheck_ki_index.restype = None
        out, mean = np.zeros(5, dtype=np.int64), C.c_float()
        t = time.time()
        L.hostcheck_ki_index(rs.enc.ctypes.data, rs.read_off.ctypes.data, rs.read_len.ctypes.data, rs.n_reads, k, w, rate, out.ctypes.data,
                             C.byref(mean), None, None, None)
        return time.time() - t, out.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="large")
    ap.add_argument("--kmer", type=int, default=15)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--rate", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    k, w = a.kmer, a.window
    t0 = time.time()
    recs = gen_kmer_preset(a.preset)
    rs = K.KmerReadSet.from_records(recs, 5000)
    res = dict(preset=a.preset, reads=rs.n_reads, bases=rs.n_bases, k=k, window=w, repeat_rate=a.rate, gen_s=round(time.time() - t0, 1))
    d = KI.DeviceKmerIndex(rs, "cuda:0", k, w, a.rate)
    res["workspace_bytes"] = d.work_bytes
    d.run()
    torch.cuda.synchronize()
    st = d.results()[0]
    d.set_params(k, w, a.rate, st["n_selected"], st["n_entries"])
    d.run()
    torch.cuda.synchronize()
    tm = N.StreamTimer()
    xs = []
    for _ in range(a.reps):
        tm.start(None)
        d.run()
        tm.stop(None)
        torch.cuda.synchronize()
        xs.append(tm.elapsed_ms())
    N.profile_begin()
    d.run()
    torch.cuda.synchronize()
    prof = {n: round(v[0], 3) for n, v in N.profile_end().items()}
    dev = d.results()
    ms = float(np.median(xs))
    key_passes, pos_passes = -(-2 * k // 8), -(-max(1, int(2 * rs.n_bases).bit_length()) // 8)
    sort_bytes = (key_passes + pos_passes) * 40 * st["n_chosen"]
    res["device"] = dict(ms=round(ms, 2), mbases_per_s=round(rs.n_bases / ms / 1e3, 1), stages_ms=prof, sort_passes=key_passes + pos_passes,
                         sort_bytes=sort_bytes)
    if prof.get("kmer_index_sort"):
        res["device"]["sort_tb_per_s"] = round(sort_bytes / (prof["kmer_index_sort"] * 1e-3) / 1e12, 3)
    res["stats"] = {f: (float(v) if f == "mean_frequency" else v) for f, v in dev[0].items()}
    del d
    torch.cuda.empty_cache()
    KI.index_host(rs, k, w, a.rate, kmer_cap=st["n_selected"], pos_cap=st["n_entries"])      # warm-up: lane, buffers
    xs = []
    for _ in range(max(1, a.reps // 2)):
        t = time.time()
        host = KI.index_host(rs, k, w, a.rate, kmer_cap=st["n_selected"], pos_cap=st["n_entries"])
        xs.append((time.time() - t) * 1e3)
    res["host_entry_ms"] = round(float(np.median(xs)), 1)
    assert all(np.array_equal(x, y) for x, y in zip(host[1:], dev[1:])) and host[0]["n_chosen"] == dev[0]["n_chosen"], "host and device entries disagree"
    N.lib().gbx_host_release()
    sec, out = host_build(rs, k, w, a.rate)
    assert out == [dev[0][f] for f in ("n_chosen", "n_distinct", "repetitive_frequency", "n_selected", "n_entries")], "the host build disagrees"
    res["host_build_1_thread_s"] = round(sec, 2)
    with tempfile.TemporaryDirectory() as td:
        fa, cfg = os.path.join(td, "reads.fasta"), os.path.join(td, "mini.cfg")
        write_fasta(fa, recs)
        open(cfg, "w").write("kmer_size=%d\nuse_minimizers=1\nminimizer_window=%d\nrepeat_kmer_rate=%g\nassemble_kmer_sample=1\n" % (k, w, a.rate))
        t = time.time()
        r = subprocess.run([os.path.join(ROOT, "genomicsbench_amd", "bin", "kmer-cnt"), "--reads", fa, "--config", cfg, "--threads", "16", "--debug"],
                           capture_output=True, text=True, timeout=900)
        wall = time.time() - t
        if r.returncode != 0:
            raise RuntimeError("kmer-cnt failed: %s" % r.stderr[-2000:])
        kt = float(re.search(r"Kernel time: ([0-9.]+) sec", r.stderr).group(1))
        assert int(re.search(r"K-mer index size: (\d+)", r.stderr).group(1)) == dev[0]["n_entries"], "driver and device entry disagree"
        res["driver"] = dict(kernel_time_s=kt, wall_s=round(wall, 2), threads=16)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
