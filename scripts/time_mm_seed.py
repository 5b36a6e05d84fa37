#!/usr/bin/env python3
"""Times the minimizer seeding stage (genomicsbench_amd.mm_seed) on a generated genome and simulated long reads and writes one
JSON line to profiles/mm_seed_time.json:

  index     build time (device events around gbx_mm_index_build_device) and bytes per reference base
  sketch    gbx_mm_sketch_device over the reads, bases/s, and the bytes its two passes read per base against the HBM rate
  seeding   gbx_mm_seed_device, anchors/s, split by the library's stage timers into sketch / lookup / fill / sort
  chain     gbx_chain_device on the very calls the seeding produced
  cpu       the same machine (mm_machine.h built for the host, libgbx_mm_cpu.so) over the same reads, one thread: the only thing
            the device figures are compared with

--preset large = --genome 67108864 --reads 4000 --read-len 10000 (40 Mb of reads against a 64 Mi genome).  Needs a GPU: no fallback.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED = 6.29e12          # bytes/s, float4 copy (the micro-architecture notes' measured figure; 8.0e12 is the specification)


def make_inputs(genome, n_reads, read_len, seed, n_contigs=4):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    g = acgt[rng.integers(0, 4, genome)]
    unit = acgt[rng.integers(0, 4, 171)]                       # a tandem repeat and a few ambiguous runs, as a real reference has
    o = genome // 3
    g[o:o + 171 * 300] = np.tile(unit, 300)[:len(g[o:o + 171 * 300])]
    for o in rng.integers(0, max(genome - 2000, 1), 8):
        g[o:o + 1000] = ord("N")
    cuts = np.linspace(0, genome, n_contigs + 1).astype(np.int64)
    refs = [g[cuts[i]:cuts[i + 1]].tobytes() for i in range(n_contigs)]
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGTN")] = list(b"TGCAN")
    reads = []
    for i in range(n_reads):
        o = int(rng.integers(0, max(genome - read_len, 1)))
        r = g[o:o + read_len].copy()
        sub = rng.random(len(r)) < 0.04                        # 4 % substitutions, 0.5 % deletions, 0.5 % insertions
        r[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
        r = r[rng.random(len(r)) >= 0.005]
        ins = np.flatnonzero(rng.random(len(r)) < 0.005)
        r = np.insert(r, ins, acgt[rng.integers(0, 4, len(ins))])
        reads.append((comp[r[::-1]] if i & 1 else r).tobytes())
    return refs, reads


def cpu_sketch_seconds(reads, p):
    L = C.CDLL(os.path.join(ROOT, "genomicsbench_amd", "libgbx_mm_cpu.so"))
    L.gbx_mm_cpu_sketch.restype = C.c_int64
    L.gbx_mm_cpu_sketch.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    cap = max(len(r) for r in reads) + 1
    ox, oy = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    t0, n = time.perf_counter(), 0
    for r in reads:
        n += L.gbx_mm_cpu_sketch(r, len(r), p.w, p.k, 0, p.is_hpc, 0, ox.ctypes.data, oy.ctypes.data, cap)
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", choices=["large"])
    ap.add_argument("--genome", type=int, default=1 << 22)
    ap.add_argument("--reads", type=int, default=400)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mm_seed_time.json"))
    a = ap.parse_args()
    if a.preset == "large":
        a.genome, a.reads, a.read_len = 1 << 26, 4000, 10000
    import torch
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import mm_seed as MS
    if not torch.cuda.is_available() or N.device_count() < 1:
        sys.exit("time_mm_seed.py needs a GPU")
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    p = MS.make_params()
    refs, reads = make_inputs(a.genome, a.reads, a.read_len, a.seed)
    read_bases = sum(len(r) for r in reads)
    cpu_s, cpu_n = cpu_sketch_seconds(reads, p)
    L = MS.lib()
    timer = N.StreamTimer()

    def timed(fn, reps):
        """the best and all of `reps` event timings of fn() on the stream, after one warm-up"""
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

    # ---- index: a minimizer for every fourth base is room enough at w = 10 (2 / (w + 1) of the bases); stats() would say otherwise
    ix = MS.DeviceMmIndex(p, refs, dev, s, mini_cap=max(a.genome // 4, 1024))
    wb = L.gbx_mm_index_workspace_bytes(p, ix.n_seqs, ix.total_len, ix.mini_cap)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    build = lambda: N.check(L.gbx_mm_index_build_device(p, ix.n_seqs, ix.text.data_ptr(), ix.off.data_ptr(), ix.total_len, ix.blob.data_ptr(),
                                                        ix.mini_cap, work.data_ptr(), wb, s))
    idx_ms, idx_all = timed(build, 3)
    del work
    # ---- sketch of the reads alone
    sd = MS.DeviceMmSeeder(ix, reads, mini_cap=max(read_bases // 4, 1024), anchor_cap=1024)
    swb = L.gbx_mm_sketch_workspace_bytes(p, sd.n_reads, sd.total_len)
    swork = torch.empty(swb, dtype=torch.uint8, device=dev)
    sk = lambda: N.check(L.gbx_mm_sketch_device(p, sd.n_reads, sd.text.data_ptr(), sd.seq_off.data_ptr(), sd.total_len, 0, sd.mini_x.data_ptr(),
                                                sd.mini_y.data_ptr(), sd.mini_cap, sd.mini_off.data_ptr(), sd.cnt.data_ptr(), swork.data_ptr(), swb, s))
    sk_ms, sk_all = timed(sk, a.repeats)
    # ---- seeding: a first run reports the anchors, the second has room for them
    sd.run(s)
    n_mini, n_anchor = sd.counts()
    sd = MS.DeviceMmSeeder(ix, reads, mini_cap=n_mini, anchor_cap=max(n_anchor, 1))
    seed_ms, seed_all = timed(lambda: sd.run(s), a.repeats)
    assert sd.fits() and sd.counts() == (n_mini, n_anchor)
    N.profile_begin()
    sd.run(s)
    torch.cuda.synchronize()
    prof = N.profile_end()
    stage = lambda *names: round(sum(prof[n][0] for n in names if n in prof), 3)
    split = dict(sketch=stage("mm_sketch_count", "mm_sketch_scan", "mm_sketch_fill"), lookup=stage("mm_seed_lookup"), fill=stage("mm_seed_fill"),
                 sort=stage("mm_seed_sort"))
    # ---- chain on the calls produced
    cb = sd.chain_batch()
    chain_ms, chain_all = timed(lambda: cb.run(s), a.repeats)
    # ---- bytes the sketch passes read: every base once per pass plus the warm start of each piece, two passes
    sketch_read_per_base = 2.0 * (1.0 + (p.w + p.k) / MS.SKETCH_CHUNK)
    rec = dict(what="minimizer seeding: index build, sketch, seeding split, chain on the produced calls; device events, best of the repeats",
               genome_bp=a.genome, reads=a.reads, read_len=a.read_len, read_bases=read_bases, k=p.k, w=p.w, seed=a.seed,
               index=dict(build_ms=round(idx_ms, 3), build_ms_all=[round(v, 3) for v in idx_all], keys=ix.info.n_keys, minimizers=ix.info.n_vals,
                          mid_occ=ix.info.mid_occ, bytes_per_base=round((16.0 * ix.info.n_keys + 8.0 * ix.info.n_vals) / a.genome, 3),
                          allocated_bytes_per_base=round(L.gbx_mm_index_bytes(ix.mini_cap) / a.genome, 3),
                          workspace_bytes_per_base=round(wb / a.genome, 3), layout="sorted distinct keys + CSR of values, binary search"),
               sketch=dict(ms=round(sk_ms, 3), ms_all=[round(v, 3) for v in sk_all], bases_per_s=round(read_bases / (sk_ms * 1e-3)),
                           minimizers=n_mini, bytes_read_per_base=round(sketch_read_per_base, 3),
                           hbm_bound_ms=round(sketch_read_per_base * read_bases / HBM_MEASURED * 1e3, 4),
                           share_of_hbm_rate=round(sketch_read_per_base * read_bases / HBM_MEASURED / (sk_ms * 1e-3), 5)),
               seeding=dict(ms=round(seed_ms, 3), ms_all=[round(v, 3) for v in seed_all], anchors=n_anchor,
                            anchors_per_s=round(n_anchor / (seed_ms * 1e-3)), stage_ms=split,
                            rep_len_total=int(sd.rep_len[:sd.n_reads].sum().item())),
               chain=dict(ms=round(chain_ms, 3), ms_all=[round(v, 3) for v in chain_all], anchors=cb.n_anchors),
               bound="chain" if chain_ms > seed_ms else "seeding",
               cpu=dict(what="mm_machine.h on the host, one thread, the reads' sketch only", sketch_s=round(cpu_s, 4), minimizers=cpu_n,
                        bases_per_s=round(read_bases / cpu_s), device_sketch_speedup=round(cpu_s / (sk_ms * 1e-3), 1)),
               device=torch.cuda.get_device_name(0))
    assert cpu_n == n_mini, "the host build of the machine and the device disagree on the number of minimizers"
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
