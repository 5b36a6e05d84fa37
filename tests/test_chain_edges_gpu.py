"""GPU parity of csrc/chain_kernels.hip at its own edges, on the calls of tests/chain_cases.py: ring sizes and flushes, every
tier of the look-back, the max_skip break in every tier and lane position, the four shapes of the ordered n_skip logic,
marks into the ring and by direct store, the folded compares of the narrow path, the fp64 gap cost, unsorted calls and
cuts.  Every comparison is bit-exact against the oracle (which tests/test_chain_edges_cpu.py holds equal to the
restatement tests/chain_ref.py on the same calls, where it also asserts that each call reaches the path it is named for).
A family runs as one call list, through chain_host and through DeviceChainBatch."""
import numpy as np
import pytest

import chain_cases as CC
import chain_ref as CR
from genomicsbench_amd.chain import DeviceChainBatch, chain_host
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu
NAMES = ("score", "parent", "target", "peak")
_want = {}


def expected(family):
    """the oracle's five outputs over the family's call list, computed once"""
    if family not in _want:
        _want[family] = O.chain_oracle(*CC.pack(CC.families()[family]), return_pairs=True)
    return _want[family]


def fact_of(case, ring, k):
    """the restatement's records of anchor k of the case (the first chunks), for the message"""
    recs = [r for r in case.ref(ring if ring in case.rings else case.rings[0])[5] if r["iabs"] == k]
    return [{f: r[f] for f in ("i", "c", "tier", "nvalid", "shape", "nskip_in", "brk", "live0")} for r in recs[-3:]]


def assert_same(got, want, family, what, ring):
    cases = CC.families()[family]
    off = np.concatenate([[0], np.cumsum([len(c.x) for c in cases])])
    for name, g, w in zip(NAMES, got, want):
        if not np.array_equal(g, w):
            at = int(np.argmax(g != w))
            ci = int(np.searchsorted(off, at, side="right")) - 1
            k = at - int(off[ci])
            raise AssertionError("%s, case %s: %s differs at %d anchors, first at anchor %d of the case: got %d want %d; its last chunks %s" % (
                what, cases[ci].name, name, int((g != w).sum()), k, g[at], w[at], fact_of(cases[ci], ring, k)))


def run_family(family, ring, split=True, wide=False):
    import torch
    cases = CC.families()[family]
    packed = CC.pack(cases)
    want = expected(family)
    assert_same(chain_host(*packed), want[:4], family, "chain_host", ring)
    d = DeviceChainBatch(*packed, torch.device("cuda:0"))
    d.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_same(d.results(), want[:4], family, "DeviceChainBatch", ring)
    assert d.evaluated_pairs() == int(want[4]), family
    # packing moves no cut: the rule is per call, so the jobs of the list are the jobs of its calls
    jobs = [j for c in cases for j in CR.chain_jobs(*c.call, split=split, wide=wide)]
    assert d.job_stats() == (len(jobs), max(n for _, n, _ in jobs)), family


@pytest.mark.parametrize("ring", ["auto", "short", "long"])
@pytest.mark.parametrize("family", list(CC.families()))
def test_edges(family, ring, monkeypatch):
    """Guards, by family: lengths - the slab flush at ib >= R + 64, the tail flush, `pkmax` of a partial last block, ring
    wrap-around; lookback - `valid = j >= st` in every tier, `jhi - 63 >= live0`, `jj >= live0`; breaks - `bl`, `before`,
    `last_bl` and the visited count; shapes - the quiet, popcount, lead and scan branches of phase 3 and the n_skip they
    hand on; marks - mark_targets' ring / direct split at live0 and `tj == iabs` through both memories; folds - dq_lim, dr_lim
    and the unsigned compares; gap - fp64 c_lin; unsorted - the st walk and the rounding of a negative gap cost; cuts and
    max_iter - chain_st_kernel and chain_jobs_kernel."""
    ringsize = {"auto": 512, "short": 512, "long": 768}[ring]
    if ring != "auto":
        monkeypatch.setenv("GBX_CHAIN_RING", ring)
    run_family(family, ringsize)


@pytest.mark.parametrize("mode", ["GBX_CHAIN_WIDE", "GBX_CHAIN_NOSPLIT"])
@pytest.mark.parametrize("ring", ["auto", "short", "long"])
@pytest.mark.parametrize("family", CC.NARROW_OR_CUT)
def test_edges_on_the_general_path_and_without_cuts(family, ring, mode, monkeypatch):
    """the families with narrow or cut jobs again with every job on the general 64-bit path, and with every call one job"""
    if ring != "auto":
        monkeypatch.setenv("GBX_CHAIN_RING", ring)
    monkeypatch.setenv(mode, "1")
    run_family(family, {"auto": 512, "short": 512, "long": 768}[ring], split=mode != "GBX_CHAIN_NOSPLIT", wide=mode == "GBX_CHAIN_WIDE")


def test_the_two_anchor_unsorted_call_on_the_device():
    c = CC.unsorted_two()
    s, p, t, k = chain_host(*CC.pack([c]))
    assert (list(s), list(p), list(t), list(k)) == ([15, 41], [-1, 0], [0, 0], [15, 41])
