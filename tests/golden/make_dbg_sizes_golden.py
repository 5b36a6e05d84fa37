"""Records what gbx_dbg_workspace_bytes and gbx_dbg_assemble_workspace_bytes return over a grid, as
tests/golden/dbg_workspace_sizes.json.  Neither entry touches the device.  The committed file was written by the library as it
was BEFORE the workspace layouts moved to csrc/dbg_plan.h (GBX_LIB selects the library); tests/test_dbg_plan_cpu.py holds
the current library to it, byte for byte.  Run it again only to pin a deliberate change of the sizes."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N_WIN = [0, 1, 2, 7, 4096, 16000]
N_READS = [0, 1, 1000, 3200000]
MAX_OCC = [0, 1, 63, 64, 150000, 1 << 24, 1 << 31]


def grid(lib, params):
    out = []
    for nw in N_WIN:
        for nr in N_READS:
            for occ in MAX_OCC:
                out.append([nw, nr, occ, int(lib.gbx_dbg_workspace_bytes(C.byref(params), nw, nr, occ)),
                            int(lib.gbx_dbg_assemble_workspace_bytes(C.byref(params), nw, nr, occ))])
    return out


if __name__ == "__main__":
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import dbg as D
    rows = grid(N.lib(), D.make_params())
    with open(os.path.join(ROOT, "tests", "golden", "dbg_workspace_sizes.json"), "w") as f:
        json.dump({"columns": ["n_win", "n_reads", "max_window_occ", "build_bytes", "assemble_bytes"], "rows": rows}, f, indent=0)
        f.write("\n")
    print("%d grid points" % len(rows))
