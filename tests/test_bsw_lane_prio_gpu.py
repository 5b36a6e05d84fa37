"""bsw lane path: the issue priority of the lane wavefronts that hold the most LDS (GBX_BSW_LANE_PRIO) and the size of the
register kernel's persistent grid (GBX_BSW_LANE_REG_WAVES per CU) change when a wavefront runs, never what it computes: every
lane class, with and without the priority, against the oracle and against each other; a register grid smaller than its chunk
list."""
import ctypes as C

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd.bsw import BswBatch, DeviceBswBatch, make_params
from genomicsbench_amd.datagen import gen_bsw
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

# query-length ranges of the lane launches (LANE_RANGE_HI in bsw_kernels.hip): compact, wide
COMPACT_HI = (47, 79, 99, 135, 159)
WIDE_HI = (39, 79, 103, 127, 159)


def reg_launches():
    f = N.lib().gbx_debug_bsw_lane_reg_launches
    f.argtypes, f.restype = [], C.c_longlong
    return f()


def reg_waves():
    """Wavefronts per CU of the last bsw_lane_reg_kernel launch."""
    f = N.lib().gbx_debug_bsw_lane_reg_waves
    f.argtypes, f.restype = [], C.c_int
    return f()


def run_device(p, b):
    """The pairs on the resident path (unpacked bases: the 80..99 class runs on bsw_lane_reg_kernel, which must be launched)."""
    import torch
    before = reg_launches()
    d = DeviceBswBatch(b, torch.device("cuda:0"))
    d.run(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert reg_launches() > before, "bsw_lane_reg_kernel was not launched"
    return d.results()


def assert_same(got, want, b, what):
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).any(1))[0]
        k = int(rows[0])
        raise AssertionError("%s: %d/%d pairs differ; first k=%d got=%s want=%s (len1=%d len2=%d h0=%d)"
                             % (what, len(rows), len(want), k, got[k], want[k], b.len1[k], b.len2[k], b.h0[k]))


@pytest.fixture
def lane(monkeypatch):
    monkeypatch.setenv("GBX_BSW_LANE", "1")
    monkeypatch.setenv("GBX_BSW_DIRECT", "0")
    for name in ("GBX_BSW_LANE_REG", "GBX_BSW_LANE_PRIO", "GBX_BSW_LANE_REG_WAVES"):      # the defaults
        monkeypatch.delenv(name, raising=False)


def classes_reached(b, max_mat=1):
    """(compact, wide) launches that get pairs, by the library's rule: wide from h0 + qlen * max_mat = 256 on."""
    wide = b.h0.astype(np.int64) + b.len2.astype(np.int64) * max_mat >= 256
    rng_of = lambda ql, his: int(np.searchsorted(his, ql))
    comp = {rng_of(q, COMPACT_HI) for q in b.len2[~wide] if 1 <= q <= 159}
    wid = {rng_of(q, WIDE_HI) for q in b.len2[wide] if 1 <= q <= 159}
    return comp, wid


@pytest.mark.parametrize("scoring", ["default", "asym"])
def test_every_class_with_and_without_priorities(lane, monkeypatch, scoring):
    """Every compact class the generated reads reach (100..135: about 550 pairs, nine chunks) and, with every eighth seed score
    raised to 200, the wide launches; the kernels' SYM instances (default scoring) and the others (o_ins != o_del)."""
    p = make_params() if scoring == "default" else make_params(o_del=5, e_del=2, o_ins=7, e_ins=3)
    b = gen_bsw(6000, 31)
    h0 = b.h0.copy()
    h0[::8] = 200
    b = BswBatch(b.ref, b.qer, b.idr, b.idq, b.len1, b.len2, h0)
    comp, wid = classes_reached(b)
    # (the generated reads' queries end at 130: the 136..159 launch shares the 100..135 launch's kernel instance and priority)
    assert comp >= {0, 1, 2, 3} and wid >= {1, 2, 3, 4}, "the case misses lane classes: compact %s, wide %s" % (comp, wid)
    want = O.bsw_oracle(p, b, 8)
    on = run_device(p, b)
    monkeypatch.setenv("GBX_BSW_LANE_PRIO", "0")
    off = run_device(p, b)
    assert on.shape == (b.n, len(N.BSW_RESULT_FIELDS))
    assert_same(on, want, b, "priorities on vs oracle")
    assert_same(off, want, b, "priorities off vs oracle")
    assert_same(on, off, b, "priorities on vs off")


def test_capped_register_grid_smaller_than_its_list(lane, monkeypatch):
    """Only the register kernel's class (queries 80..99, some 24 k pairs: some 380 chunks) and one wavefront per CU, fewer
    wavefronts than chunks: each loops over several."""
    p = make_params()
    full = gen_bsw(200_000, 77)
    m = (full.len2 >= 80) & (full.len2 <= 99)
    b = BswBatch(full.ref, full.qer, full.idr[m], full.idq[m], full.len1[m], full.len2[m], full.h0[m])
    assert b.n > 64 * 300, "too few pairs for more chunks than one wavefront per CU: %d" % b.n
    want = O.bsw_oracle(p, b, 8)
    planned = run_device(p, b)                                  # the default: planned from the kernels' register counts
    default_waves = reg_waves()
    monkeypatch.setenv("GBX_BSW_LANE_REG_WAVES", "64")          # more than fit: what is resident, as the occupancy query has it
    uncapped = run_device(p, b)
    resident = reg_waves()
    print("register wavefronts per CU: %d planned, %d resident" % (default_waves, resident))
    assert 4 <= resident <= 16 and 1 <= default_waves <= resident, "register wavefronts per CU: %d planned, %d resident" % (default_waves, resident)
    monkeypatch.setenv("GBX_BSW_LANE_REG_WAVES", "1")
    capped = run_device(p, b)
    assert reg_waves() == 1
    assert_same(capped, want, b, "capped vs oracle")
    assert_same(uncapped, want, b, "uncapped vs oracle")
    assert_same(planned, want, b, "planned vs oracle")
    assert_same(capped, uncapped, b, "capped vs uncapped")
