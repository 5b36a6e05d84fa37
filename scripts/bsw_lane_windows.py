"""CPU costing of column lock-step for bsw's compact lane classes: replays the windows of every row of bsw 'large' (seed 1002)
with the oracle's row loop, the pairs in the device's sorted order (the bsw_lsort_* kernels: query length, then min(h0, 255)),
in chunks of 64 taken from the end of each class's list as bsw_lane_kernel takes them.  Per class it prints the cells the
lanes compute, 64 x the widest window of every row (what the LDS lane kernel pays), 64 x the hull of the lanes' windows per
row in column pairs and in 8-column blocks (what a column-lock-step kernel pays), and the share of those blocks that some
running lane covers only in part (the masked variant).  Pairs of equal key are taken in input order (on the device their
order within a key is that of the sort's atomics).
usage: python scripts/bsw_lane_windows.py [n_pairs] [--json out.json]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
from genomicsbench_amd.bsw import make_params  # noqa: E402
from genomicsbench_amd.datagen import gen_bsw  # noqa: E402

LANE_QMAX, COMPACT_LIMIT, SCORE_LIMIT = 159, 256, 8192
RANGES = [("c47", 1, 47), ("c79", 48, 79), ("c99", 80, 99), ("c135", 100, 135), ("c159", 136, 159)]


def main():
    args = [a for a in sys.argv[1:]]
    out_json = None
    if "--json" in args:
        k = args.index("--json")
        out_json = args[k + 1]
        del args[k:k + 2]
    n = int(args[0]) if args else 2_000_000
    tmp = tempfile.mkdtemp()
    so = os.path.join(tmp, "lane_windows.so")
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", os.path.join(HERE, "bsw_lane_windows.c"), "-o", so])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.lane_windows.argtypes = [vp] + [C.c_int] * 7 + [C.c_int64] + [vp] * 9
    lib.lane_windows.restype = None

    b = gen_bsw(n, 1002)
    p = make_params()
    mat = np.array([p.mat[k] for k in range(25)], dtype=np.int8)
    mx = max(int(mat.max()), 0)
    q, t, h0 = b.len2.astype(np.int64), b.len1.astype(np.int64), b.h0.astype(np.int64)
    ok = (q >= 1) & (q <= LANE_QMAX) & (t >= 1) & (h0 >= 0) & (h0 + q * mx < SCORE_LIMIT)
    compact = ok & (h0 + q * mx < COMPACT_LIMIT)
    key = (q << 8) | np.minimum(h0, 255)
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(vp)  # noqa: E731
    res = {}
    for name, lo, hi in RANGES:
        sel = np.nonzero(compact & (q >= lo) & (q <= hi))[0]
        order = sel[np.argsort(key[sel], kind="stable")].astype(np.int32)
        st = np.zeros(8, dtype=np.float64)
        if len(order):
            lib.lane_windows(P(mat), p.o_del, p.e_del, p.o_ins, p.e_ins, p.zdrop, p.end_bonus, p.w, C.c_int64(len(order)), P(order),
                             P(b.ref), P(b.qer), P(b.idr), P(b.idq), P(b.len1), P(b.len2), P(b.h0), P(st))
        cells, widest, upair, ublock, nblk, nmask, rows, lrows = st
        r = {"pairs": int(len(order)), "cells": cells, "widest_x64": widest, "union_pairs_x64": upair, "union_blocks_x64": ublock,
             "blocks": nblk, "masked_blocks": nmask}
        if widest:
            r.update({"computed_over_widest": cells / widest, "union_pairs_over_widest": upair / widest,
                      "union_blocks_over_widest": ublock / widest, "masked_share": nmask / max(nblk, 1), "lane_rows_over_x64": lrows / (64 * rows)})
            print("%-5s %8d pairs  cells %.3e  widest x64 %.3e (%.1f %% computed)  union/widest: pairs %.3f  8-col blocks %.3f  "
                  "masked blocks %.1f %%" % (name, len(order), cells, widest, 100 * cells / widest, upair / widest, ublock / widest,
                                             100 * nmask / max(nblk, 1)))
        res[name] = r
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"what": "bsw 'large' (seed 1002, %d pairs) compact lane classes: lock-step window costs" % n, "classes": res}, f, indent=1)


if __name__ == "__main__":
    main()
