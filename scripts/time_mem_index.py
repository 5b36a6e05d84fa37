"""Times the HIP index builder (fmi.build_index_native, gbx_fmi_build_device) beside the torch builder (fmi.build_index) in one
process on two genomes: gen_fmi_genome(N), and the same genome with 1 % of its length overwritten by copies of 5 000-base
stretches from elsewhere in it, so that groups of tied suffixes survive many doubling rounds.  For each: wall time of a build
(synchronised; the first native build and the best of --reps), the doubling rounds, the slots sorted per round, the native
workspace, and the torch path's peak allocation.  The two indexes must be equal.  One JSON line, written to --out.

    python scripts/time_mem_index.py [--genome 67108864] [--reps 2] [--out profiles/mem_index_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import fmi as FM  # noqa: E402


def planted(g, seed):
    """1 % of g overwritten by copies of 5 000-base stretches taken from elsewhere in it."""
    out = g.copy()
    rng = np.random.default_rng(seed)
    for _ in range(max(1, len(g) // 100 // 5000)):
        src, dst = (int(x) for x in rng.integers(0, len(g) - 5000, 2))
        out[dst:dst + 5000] = g[src:src + 5000]
    return out


def round_slots():
    L = FM._build_lib()
    buf, n = (C.c_int64 * 64)(), C.c_int32(0)
    N.check(L.gbx_fmi_build_rounds(buf, 64, C.byref(n)))
    return [int(buf[k]) for k in range(n.value)]


def measure(g, dev, reps, profile):
    import torch
    n1 = 2 * len(g) + 1
    dg = torch.from_numpy(g).to(dev)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nat = FM.build_index_native(dg, dev, sa_compx=3, info=True)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    slots = round_slots()
    prof = None
    if profile:
        N.profile_begin()
        FM.build_index_native(dg, dev, sa_compx=3)
        torch.cuda.synchronize()
        prof = {k: [round(v[0], 2), v[1]] for k, v in N.profile_end(64).items()}
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = FM.build_index(dg, device=dev, sa_compx=3)
    torch.cuda.synchronize()
    t_torch = time.perf_counter() - t0
    peak = int(torch.cuda.max_memory_allocated())
    idx, smp, info = nat
    equal = bool(idx.ref_seq_len == ref[0].ref_seq_len and idx.count == ref[0].count and idx.sentinel_index == ref[0].sentinel_index and
                 torch.equal(idx.cp_occ, ref[0].cp_occ) and torch.equal(smp.ms, ref[1].ms) and torch.equal(smp.ls, ref[1].ls))
    assert equal, "the native index differs from fmi.build_index's"
    assert info["rounds"] == len(slots) and (not slots or slots[0] == info["first_round_slots"])
    return {"suffixes": n1, "native_s_first": round(times[0], 4), "native_s": round(min(times), 4), "native_s_all": [round(t, 4) for t in times],
            "torch_s": round(t_torch, 4), "native_over_torch": round(min(times) / t_torch, 3), "rounds": info["rounds"],
            "native_slots_per_round": slots, "torch_slots_per_round": n1, "native_workspace_bytes": FM.build_workspace_bytes(len(g)),
            "native_workspace_bytes_per_symbol": round(FM.build_workspace_bytes(len(g)) / (2 * len(g)), 2),
            "torch_max_memory_allocated": peak, "torch_bytes_per_symbol": round(peak / (2 * len(g)), 1), "equal": equal, "native_profile_ms": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=64 << 20)
    ap.add_argument("--seed", type=int, default=6001)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--profile", type=int, default=1, help="one more native build between gbx_profile_begin / _end")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_index_time.json"))
    args = ap.parse_args()
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    g = gen_fmi_genome(args.genome, args.seed)
    out = {"what": "fmi.build_index_native (gbx_fmi_build_device) beside fmi.build_index (torch.sort prefix doubling), sa_compx 3, one process",
           "genome_bp": args.genome, "random": measure(g, dev, args.reps, args.profile), "planted_repeats": measure(planted(g, args.seed + 1), dev, args.reps, args.profile),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
