"""GPU parity of csrc/dbg_kernels.hip at its own edges, on the calls of tests/dbg_cases.py: k-mers that share a node slot's
tag and home (the byte compare and the probe past a taken slot), one such window 256 times in a batch, tables at the load
their sizing allows with a probe that wraps, node counts and first-touch keys on the finish kernel's 256-rank rounds, its
record buffer filled to the byte, successor lists of 200, the filter's thresholds and an awkward layout of windows and
reads.  Every comparison is exact against the restatement tests/dbg_ref.py (tests/test_dbg_edges_cpu.py asserts, on the
CPU alone, that each call is what it is named for): stats and digest from gbx_dbg_build_host and gbx_dbg_build_device, and
from both graph entries every node field - src as a number, first_edge across rounds and windows - and every edge."""
import ctypes

import pytest

import dbg_cases as DC
import dbg_ref as R
from genomicsbench_amd import dbg as D

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in DC.all_cases()}
STATS_ONLY = [c.name for c in DC.families()["replicated"]]


def same_stats(got, want, what):
    assert len(got) == len(want)
    for w, st in enumerate(want):
        for f in R.STATS_FIELDS:
            assert int(got[w][f]) == st[f], "%s: window %d: %s is %d, the restatement has %d" % (what, w, f, int(got[w][f]), st[f])


def same_graph(case, res, w0, w1, what):
    """windows [w0, w1) of a graph_* result against the restatement, field by field"""
    nodes, edges, node_off, edge_off = res
    rs, ws, _ = case.packed()
    want_st, want_g = case.want()
    assert int(node_off[-1]) == len(nodes) == sum(st["n_nodes"] for st in want_st[w0:w1]), what
    assert int(edge_off[-1]) == len(edges) == sum(st["n_edges"] for st in want_st[w0:w1]), what
    for j in range(w1 - w0):
        want, srcs = want_g[w0 + j], case.src_numbers(w0 + j)
        got = D.render(rs, ws, nodes, edges, node_off, edge_off, case.k, j)
        assert len(got) == len(want), (what, w0 + j)
        first_edge = int(edge_off[j])
        for x, (g, h) in enumerate(zip(got, want)):
            nd = nodes[int(node_off[j]) + x]
            where = "%s: window %d node %d" % (what, w0 + j, x)
            assert int(nd["src"]) == srcs[x], "%s: src is %d, the restatement has %s = %d" % (where, int(nd["src"]), h["src"], srcs[x])
            assert (int(nd["n_edges"]), int(nd["first_edge"])) == (len(h["edges"]), first_edge), where
            assert (g["kmer"], g["colours"], g["position"], g["weight"]) == (h["kmer"], h["colours"], h["position"], h["weight"]), where
            assert g["edges"] == h["edges"], where
            first_edge += len(h["edges"])
        assert first_edge == int(edge_off[j + 1])


def one_window_workspace(case):
    """test_dbg_gpu.py's `small` recipe: the head, and tables for the largest window alone: every window a batch of its own
    (but empty ones, which need next to nothing)"""
    from genomicsbench_amd import _native as N
    rs, ws, p = case.packed()
    occ = int(ws.occ_slots(rs, case.k).max())
    L = N.lib()
    return L.gbx_dbg_workspace_bytes(ctypes.byref(p), ws.n_win, rs.n_reads, 0) + L.gbx_dbg_workspace_bytes(ctypes.byref(p), 1, 0, occ)


def run_case(case, graphs=True, work_bytes=None, ranges=None):
    import torch
    rs, ws, p = case.packed()
    want_st, _ = case.want()
    st = D.build_host(rs, ws, p)
    same_stats(st, want_st, case.name + " build_host")
    dd = D.DeviceDbg(rs, ws, "cuda:0", p, work_bytes=work_bytes)
    dd.build(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dst = dd.results()
    same_stats(dst, want_st, case.name + " DeviceDbg")
    if not graphs:
        return
    for w0, w1 in ranges or [(0, ws.n_win)]:
        same_graph(case, D.graph_host(rs, ws, st, w0, w1, p), w0, w1, "%s graph_host [%d, %d)" % (case.name, w0, w1))
        same_graph(case, dd.graph(dst, w0, w1), w0, w1, "%s DeviceDbg.graph [%d, %d)" % (case.name, w0, w1))


@pytest.mark.parametrize("name", [n for n in CASES if n not in STATS_ONLY])
def test_edges(name):
    """Guards, by family: collide - node_slot's k-byte compare behind a tag match (first, middle and last byte; the slot's
    text in the reference or in a read) and the step past a slot another k-mer holds; full_tables - probes in tables with
    2 free node slots and 1 free edge slot, and the wrap of (i + 1) & mask; rounds, two_c, late_key - the in-place
    compaction of byfirst and n, ebase and s_digest carried across rounds, with n_nodes and 2C on, below and above multiples
    of 256 and a key in the last slot 2C - 1; records_full - rec[] filled to its last byte, with and without dropped
    successors; fanout - the four of least first appearance out of 201 in list order, weights summed; quality - the
    filter at min_qual and min_qual - 1, 'N' and 0x200; layout, rounds_call - windows without slots, reads without slots,
    shared reads, and first_edge / src across windows."""
    run_case(CASES[name])


@pytest.mark.parametrize("name", STATS_ONLY)
def test_one_window_256_times(name):
    """the race for the shared home slot has two outcomes (three k-mers: six); 256 copies in one batch, one graph"""
    run_case(CASES[name], graphs=False)


@pytest.mark.parametrize("name", ["layout", "rounds_call"])
def test_one_window_per_batch_and_sub_ranges(name):
    """a workspace for one window at a time (the plan's batches, cand0 and base start over), and graphs of window ranges with
    w0 > 0, where the host entry rebases the reference and the reads and src is moved back: [1, n), the last window alone
    (rounds_call: the 513-node path) and a range that starts and ends on empty windows"""
    case = CASES[name]
    n = case.n_win
    inner = {"layout": (2, 9), "rounds_call": (0, 7)}[name]
    assert all(case.occ(w) == 0 for w in (inner[0], inner[1] - 1)) and any(case.occ(w) for w in range(*inner))
    run_case(case, ranges=[(1, n), (n - 1, n), inner])
    run_case(case, work_bytes=one_window_workspace(case), ranges=[(0, n), (1, n), inner])
