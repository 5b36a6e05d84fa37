"""The read sets of tests/pileup_cases.py are what they claim to be: every property that test_pileup_edges_gpu.py relies
on is asserted here on the restatement (tests/pileup_ref.py) alone, on the CPU box.  No library call that needs a device."""
import numpy as np
import pytest

import pileup_cases as PC
import pileup_ref as PR


def test_restated_sizing_matches_the_table():
    """window / cap16 / cap32 as csrc/pileup_kernels.hip computes them (Wn, cap_cols) at the F values the cases use."""
    table = {10: (512, 3276, 1638), 50: (320, 655, 327), 100: (160, 327, 163), 520: (32, 63, 31), 10240: (32, 3, 1)}
    for F, want in table.items():
        assert (PC.window(F), PC.cap16(F), PC.cap32(F)) == want
    assert (PC.PC_LDS_WORDS, PC.PC_SUB, PC.PT_TILE) == (16384, 32, 8192)
    assert all(PC.window(F) % PC.PC_SUB == 0 and 2 * PC.window(F) <= max(PC.cap16(F), 2 * PC.PC_SUB) for F in range(10, 10250, 10))


@pytest.mark.parametrize("nd,nh", PC.FEATURE_GRID)
def test_feature_grid_claims(nd, nh):
    case = PC.feature_grid(nd, nh)
    assert case.F == 10 * nd * nh and (case.F == 10240) == ((nd, nh) in ((16, 64), (64, 16)))
    PC.check_feature_grid(case, PC.reference(case))


@pytest.mark.parametrize("F", list(PC.ROUNDS_F))
def test_rounds_claims(F):
    case = PC.rounds(F)
    assert case.F == F
    PC.check_rounds(case, PC.reference(case))


@pytest.mark.parametrize("F", list(PC.EDGES_F))
def test_window_edges_claims(F):
    case = PC.window_edges(F)
    assert case.F == F
    PC.check_window_edges(case, PC.reference(case))


@pytest.mark.parametrize("name", PC.COUNTER_WIDTH)
def test_counter_width_claims(name):
    case = PC.counter_width(name)
    PC.check_counter_width(case, PC.reference(case))


@pytest.mark.parametrize("k", [1, 2, 7, 50])
@pytest.mark.parametrize("name", ["c65534", "all65536", "idle", "wide_rounds"])
def test_scaled_reference_is_additive(name, k):
    """counts(k copies) == k * counts(1 copy), with the layout's depth and aligned bases: the shortcut by which the 65 k-read
    sets are restated, held against the restatement of the expanded reads"""
    case = PC.counter_width(name)
    mult = [min(int(m), k + c) for c, m in enumerate(case.mult)]
    rs = PC.expand(case.recs, mult)
    pc, st = PR.layout(rs, case.start, case.end, case.nd)
    want = (pc, st) + PR.counts(rs, case.start, case.end, pc, case.nd, case.nh)
    got = PC.scaled_reference(case.recs, mult, case.start, case.end, case.nd, case.nh)
    assert got[1] == want[1]
    for g, w in zip((got[0],) + got[2:], (want[0],) + want[2:]):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_expand_copies_reads_whole():
    case = PC.counter_width("wide_rounds")
    rs = case.reads
    assert rs.n_reads == 65540 and rs.seq.size == sum(m * ((len(r["seq"]) + 1) // 2) for r, m in zip(case.recs, case.mult))
    at = np.concatenate([[0], np.cumsum(case.mult)])
    for c, r in enumerate(case.recs):
        for i in {int(at[c]), int(at[c + 1]) - 1}:
            pos, cig, codes, qual, rev, dt = rs.read(i)
            assert (pos, cig, rev, dt) == (r["pos"], r["cigar"], r["rev"], r["dtype"])
            assert np.array_equal(codes, r["seq"]) and np.array_equal(qual, r["qual"])


@pytest.mark.parametrize("n", PC.SCAN_N + [-PC.SCAN_N[-1]])
def test_scan_edges_claims(n):
    case = PC.scan_edges(abs(n), n < 0)
    assert case.end - case.start == abs(n)
    PC.check_scan_edges(case, PC.layout_reference(case))


@pytest.mark.parametrize("n_reads", PC.PMAX_READS)
def test_pmax_reads_claims(n_reads):
    case = PC.pmax_reads(n_reads)
    assert case.reads.n_reads == n_reads
    PC.check_pmax_reads(case, PC.reference(case))


def test_scan_big_claims():
    case = PC.scan_big()
    assert case.end - case.start == 1025 * 8192 + 3
    PC.check_scan_big(case, PC.layout_reference(case))
