"""GPU parity of bsw_lane_reg_kernel (the compact 80..99 lane class with its cells in registers) on the resident path (unpacked
bases), with the lane path forced on, against the oracle and bit for bit against bsw_lane_kernel (GBX_BSW_LANE_REG=0)."""
import ctypes as C

import numpy as np
import pytest

from cases import adversarial_bsw
from genomicsbench_amd import _native as N
from genomicsbench_amd.bsw import BswBatch, DeviceBswBatch, fill_scmat, make_params
from genomicsbench_amd.datagen import gen_bsw
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


def reg_launches():
    f = N.lib().gbx_debug_bsw_lane_reg_launches
    f.argtypes, f.restype = [], C.c_longlong
    return f()


def run_device(p, b, expect_reg=True):
    """The pairs on the resident path; checks that the register kernel was (or was not) launched."""
    import torch
    before = reg_launches()
    d = DeviceBswBatch(b, torch.device("cuda:0"))
    d.run(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ran = reg_launches() - before
    assert (ran > 0) == expect_reg, "bsw_lane_reg_kernel launches: %d" % ran
    return d.results()


def assert_same(got, want, b):
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).any(1))[0]
        k = int(rows[0])
        raise AssertionError("%d/%d pairs differ; first k=%d got=%s want=%s (len1=%d len2=%d h0=%d)"
                             % (len(rows), len(want), k, got[k], want[k], b.len1[k], b.len2[k], b.h0[k]))


def reads(n, seed, qlens, max_t=260):
    """n pairs: a query of a length drawn from `qlens`, a target that copies it with substitutions and short indels and then
    diverges (so windows narrow, widen and end inside the band), h0 up to the compact limit (h0 + qlen * 1 < 256)."""
    rng = np.random.default_rng(seed)
    ts, qs, h0 = [], [], []
    for _ in range(n):
        ql = int(rng.choice(qlens))
        q = rng.integers(0, 4, ql).astype(np.uint8)
        sub = rng.random() * 0.25
        cut = int(rng.integers(0, ql + 1)) if rng.random() < 0.4 else ql
        t, j = [], 0
        while j < cut:
            u = rng.random()
            if u < 0.02:
                j += int(rng.integers(1, 8))
                continue
            t.append(q[j] if rng.random() >= sub else int(rng.integers(0, 4)))
            if rng.random() < 0.02:
                t.extend(rng.integers(0, 4, int(rng.integers(1, 8))).tolist())
            j += 1
        tl = max(1, min(max_t, len(t) + int(rng.integers(0, 60))))
        t = np.array(t[:tl], dtype=np.uint8)
        if len(t) < tl:
            t = np.concatenate([t, rng.integers(0, 4, tl - len(t)).astype(np.uint8)])
        if rng.random() < 0.1:
            q[rng.random(ql) < 0.03] = 4
        hi = 255 - ql
        h0.append(int(rng.integers(max(0, hi - 40), hi + 1)) if rng.random() < 0.5 else int(rng.integers(0, hi + 1)))
        ts.append(t)
        qs.append(q)
    return BswBatch.from_sequences(ts, qs, np.array(h0, dtype=np.int32))


@pytest.fixture
def reg(monkeypatch):
    monkeypatch.setenv("GBX_BSW_LANE", "1")
    monkeypatch.setenv("GBX_BSW_DIRECT", "0")
    monkeypatch.delenv("GBX_BSW_LANE_REG", raising=False)     # the default: on


SCORINGS = {
    "default": {},
    "zdrop0": dict(zdrop=0),
    "zdrop_small": dict(zdrop=10, w=40),
    "asym": dict(o_del=5, e_del=2, o_ins=7, e_ins=3, zdrop=50, end_bonus=9, w=37, mat=fill_scmat(1, 5, -2)),
}


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_class_edges_vs_oracle(reg, scoring):
    """Queries on both edges of the class and beside it (79/80, 99/100, 135/136), h0 up to the compact limit, a ragged last chunk."""
    p = make_params(**SCORINGS[scoring])
    b = reads(64 * 37 + 23, 7, [79, 80, 81, 98, 99, 100, 101, 118, 134, 135, 136])
    assert_same(run_device(p, b), O.bsw_oracle(p, b, 8), b)


def test_every_length_of_the_classes_vs_oracle(reg):
    p = make_params()
    b = reads(64 * 60 + 5, 11, list(range(80, 100)))
    assert_same(run_device(p, b), O.bsw_oracle(p, b, 8), b)


def test_adversarial_vs_oracle(reg):
    """Diverged tails and long targets: windows that end early and grow again read the stale cells past end."""
    p = make_params()
    b = adversarial_bsw(8000, 5, max_q=140, max_t=600)
    assert_same(run_device(p, b), O.bsw_oracle(p, b, 8), b)


def test_bit_for_bit_against_lds_kernel(reg, monkeypatch):
    p = make_params()
    b = gen_bsw(200_000, 77)
    got = run_device(p, b)
    monkeypatch.setenv("GBX_BSW_LANE_REG", "0")
    want = run_device(p, b, expect_reg=False)
    assert got.shape == (b.n, len(N.BSW_RESULT_FIELDS))
    assert_same(got, want, b)
