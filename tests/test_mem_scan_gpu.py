"""The exclusive scan the four bwa-mem stages share (csrc/mem_scan.hip) across its 1024-entry block boundary: the stages' other
GPU tests have at most 300 units, one block.  A scan has n + 1 entries per quantity, so n = 1023 fills one block exactly, 1024
leaves the total alone in a second block and 2049 needs three; the paired-end stage scans 2 n_pairs + 1 entries.  The inputs are
the stages' own generators, the comparison each stage's own, exact, against its restated rules."""
import numpy as np
import pytest

import mem_chain_cases as KC
import mem_cigar_cases as KG
import mem_pair_cases as KP
import mem_regs_cases as KR
import test_mem_chain_gpu as TC
import test_mem_cigar_gpu as TG
import test_mem_pair_gpu as TP
import test_mem_regs_gpu as TR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_reads", [1023, 1024, 1025, 2049])
def test_chain_reads_across_scan_blocks(n_reads):
    want = TC.both_entries(KC.synthetic(n_reads, 31))
    assert len(want["chain_off"]) == n_reads + 1 and want["chain_off"][-1] == len(want["chains"]) > n_reads


@pytest.mark.parametrize("n_reads", [1023, 1024, 1025, 2049])
def test_regs_reads_across_scan_blocks(n_reads):
    want = TR.both_entries(KR.synthetic(n_reads, 32))
    assert len(want["reg_off"]) == n_reads + 1 and want["reg_off"][-1] == want["n_regs"] > n_reads > want["n_sel"] > 0


@pytest.mark.parametrize("n_pairs", [511, 512, 513, 1025])
def test_pair_pairs_across_scan_blocks(n_pairs):
    j = KP.synthetic(n_pairs, 33)
    want = TP.both_entries(j)
    assert want["boundary"] == 0, want["notes"][:3]                  # (what makes the exact comparison valid: test_mem_pair_cpu.py)
    assert len(j["reg_off"]) == 2 * n_pairs + 1 and want["n_psel"] > n_pairs


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_cigar_records_across_scan_blocks(n):
    """The device entry takes exactly n records here (no slack records behind them), the host entry too."""
    j = KG.synthetic(n, 34)
    want = KG.reference_c(j)
    got, nc, ok = TG.device(j, slack=0)
    assert ok and nc == len(want[1]) > n
    KG.same(got, want)
    KG.same(TG.host(j), want)


def test_regs_upstream_overflow_across_scan_blocks():
    """A count one above its capacity: both totals are -1 and every offset is 0, the total's entry in the second block too."""
    j = KR.synthetic(1025, 35)
    n_chains, n_seeds = len(j["chains"]), len(j["seeds"])
    for counts in ([n_chains + 8, n_seeds], [n_chains, n_seeds + 8]):                      # (the capacities are 7 above the counts)
        got, ok = TR.device(j, counts=counts)
        assert ok and got["n_regs"] == -1 and got["n_sel"] == -1 and len(got["reg_off"]) == 1026 and (got["reg_off"] == 0).all()
        assert (got["sel_res"] == -1).all() and not got["sel_seeds"].tobytes().strip(b"\0")


def test_pair_upstream_overflow_across_scan_blocks():
    """The region count one above its capacity (5 above the count): the total is -1, no pair and no record is made."""
    j = KP.synthetic(1025, 36)
    got, intact, unchanged = TP.device(dict(j, pes_in=None), n_regs=len(j["regs"]) + 6)
    assert intact and unchanged and got["n_psel"] == -1
    assert not got["pairs"].tobytes().strip(b"\0") and got["pes"]["failed"].tolist() == [1, 1, 1, 1]
    assert (got["psel_res"] == -1).all() and not got["psel_seeds"].tobytes().strip(b"\0")
