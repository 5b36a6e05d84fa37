#!/usr/bin/env python
"""Times abea's methylation frequency stage (f5c meth-freq on the device) on seeded, generated records.

    python scripts/time_abea_freq.py --preset small|large

large: 2^25 records over about 2^20 sites on 24 contigs, a fifth of them with num_cpgs 2..6; small: 2^18 over 2^14.  With and
without -s: the device stages (expand, sort, reduce, text) from the library's stage events after a warm-up, each with its
algorithmic bytes over its time as a share of the HBM peak; the host entry box to box; the driver from the text of all the
records (--driver-records N: of the first N).  Progress goes to stderr; prints one JSON line and writes
profiles/abea_freq_time_<preset>.json.
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
from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import abea_freq as AF  # noqa: E402

PRESETS = {"small": (1 << 18, 1 << 14), "large": (1 << 25, 1 << 20)}
N_CONTIGS, HBM_PEAK = 24, 8.0e12                              # bytes / s, MI355X
TEMPLATE = np.frombuffer(b"TACG" * 6 + b"AA", np.uint8)      # a record of k CpGs carries the last 4 k + 2 bytes
CHUNK = 1 << 20                                              # lines formatted at a time


def generate(n, n_sites, seed=20240521):
    rng = np.random.default_rng(seed)
    site = rng.integers(0, n_sites, n)
    k = np.where(rng.random(n) < 0.2, rng.integers(2, 7, n), 1).astype(np.int32)
    rec = np.zeros(n, AF.RECORD_DTYPE)
    rec["contig"] = site % N_CONTIGS
    rec["start"] = 10000 + 16 * (site // N_CONTIGS)
    rec["seq_len"] = 4 * k + 2
    rec["end"] = rec["start"] + np.where(k > 1, 4 * (k - 1), 0)
    rec["n_cpg"] = k
    rec["llr"] = np.round(rng.normal(0, 4, n), 2)
    rec["seq_off"] = 24 - 4 * k                               # records share the template's bytes: offsets need not be disjoint
    names = sorted(("chr%d" % (c + 1)).encode() for c in range(N_CONTIGS))
    return rec, TEMPLATE.copy(), names


def write_text(path, rec, arena, names, limit):
    """the call-methylation TSV of the first `limit` records -> its bytes"""
    a = arena.tobytes()
    total = 0
    with open(path, "wb") as f:
        total += f.write(AF_HEAD)
        for lo in range(0, limit, CHUNK):
            r = rec[lo:min(lo + CHUNK, limit)]
            lines = [b"%s\t%d\t%d\tr\t%.2f\t-100.00\t-101.00\t1\t%d\t%s\n" % (names[c], s, e, llr, k, a[off:off + ln])
                     for c, s, e, k, llr, off, ln in zip(r["contig"].tolist(), r["start"].tolist(), r["end"].tolist(), r["n_cpg"].tolist(), r["llr"].tolist(),
                                                         r["seq_off"].tolist(), r["seq_len"].tolist())]
            total += f.write(b"".join(lines))
    return total


def note(msg):
    print("time_abea_freq: " + msg, file=sys.stderr, flush=True)


AF_HEAD = b"chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_cpgs\tsequence\n"


def device_run(rec, arena, names, split, pos_bits, contig_bits):
    import torch
    dev = torch.device("cuda:0")

    def once():
        d = AF.DeviceAbeaFreq(dev, 2.5, split, pos_bits, contig_bits)
        d.add_records(rec, arena)
        d.count()
        d.size()
        d.fill()
        return d, d.text(names)
    once()                                                   # warm-up
    torch.cuda.synchronize()
    N.profile_begin()
    d, text = once()
    torch.cuda.synchronize()
    prof = N.profile_end()
    ms = lambda *ks: float(sum(prof[k][0] for k in ks if k in prof))
    n, items, sites, seq_bytes = len(rec), d.n_items, d.n_sites, d.n_bytes
    passes = 2 * ((pos_bits + 7) // 8) + (contig_bits + 7) // 8
    stage = {
        # records in, item offsets out and in again, sort items and FreqItems out (a split record's bytes are read twice)
        "expand": (ms("abea_freq_count", "abea_freq_expand"), 2 * 40 * n + 3 * 8 * n + 40 * items + (2 * int(rec["seq_len"].sum()) if split else 0)),
        # a pass: the histogram reads a word, the scatter reads and writes both
        "sort": (ms("abea_freq_sort"), passes * 40 * items),
        # keys and items in, three prefix arrays out, scanned (read + write, twice), read again per segment; the table and its arena out
        "reduce": (ms("abea_freq_reduce", "abea_freq_fill"), (16 + 24 + 24) * items + 3 * 32 * items + 2 * 32 * items + 40 * sites + 2 * seq_bytes),
        "text": (ms("abea_freq_tsv_count", "abea_freq_tsv_fill"), 2 * (40 * sites + seq_bytes) + 3 * 8 * sites + len(text)),
    }
    out = {k: dict(ms=round(v[0], 4), bytes=int(v[1]), hbm_share=round(v[1] / (v[0] * 1e-3) / HBM_PEAK, 4) if v[0] > 0 else "not measured") for k, v in stage.items()}
    out.update(items=int(items), sites=int(sites), text_bytes=len(text), sort_passes=passes, device_total_ms=round(sum(v[0] for v in stage.values()), 4))
    return out, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="small")
    ap.add_argument("--no-driver", action="store_true")
    ap.add_argument("--driver-records", type=int, default=0, help="the driver reads the text of the first N records (0: all)")
    a = ap.parse_args()
    n, n_sites = PRESETS[a.preset]
    rec, arena, names = generate(n, n_sites)
    pos_bits, contig_bits = AF.bits_for(int(rec["start"].max()) + 32), AF.bits_for(N_CONTIGS - 1)
    res = dict(preset=a.preset, records=n, site_span=n_sites, contigs=N_CONTIGS, pos_bits=pos_bits, contig_bits=contig_bits, hbm_peak_bytes_per_s=HBM_PEAK)
    m = min(n, a.driver_records) if a.driver_records > 0 else n
    tmp = tempfile.TemporaryDirectory()
    src, dst = os.path.join(tmp.name, "in.tsv"), os.path.join(tmp.name, "out.tsv")
    if not a.no_driver:
        res["driver_text_bytes"] = write_text(src, rec, arena, names, m)
        note("wrote the text of %d records, %d bytes" % (m, res["driver_text_bytes"]))
    for split in (False, True):
        key = "split" if split else "unsplit"
        r, text = device_run(rec, arena, names, split, pos_bits, contig_bits)
        note("%s: device stages done" % key)
        AF.freq_host(rec[:1024], arena, 2.5, split)          # the host lane's first use
        t0 = time.perf_counter()
        hs, ha = AF.freq_host(rec, arena, 2.5, split)
        out = AF.tsv_host(hs, ha, names)
        r["host_entry_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        assert out == text
        r["driver_ms"] = r["driver_records"] = "not measured"
        note("%s: host entry done" % key)
        if not a.no_driver:
            t0 = time.perf_counter()
            p = subprocess.run([os.path.join(ROOT, "genomicsbench_amd", "bin", "meth-freq"), "-i", src, "-o", dst] + (["-s"] if split else []), capture_output=True,
                               timeout=900)
            r["driver_ms"], r["driver_records"] = round(1e3 * (time.perf_counter() - t0), 3), m
            assert p.returncode == 0, p.stderr[-2000:]
            if m == n:
                assert open(dst, "rb").read() == text
            note("%s: driver done" % key)
        res[key] = r
    tmp.cleanup()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "abea_freq_time_%s.json" % a.preset), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
