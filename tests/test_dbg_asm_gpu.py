"""GPU parity of the dbg assembly stage (csrc/dbg_asm_kernels.hip, csrc/capi_dbg_asm.hip) on the calls of
tests/dbg_asm_cases.py and on the two fixtures: every field of gbx_dbg_assemble_host and gbx_dbg_assemble_device - per window
the final k, the builds, the cyclic flag, the final graph's stats and the counts; per start its node, edge, status and
place; per path its nodes, weight, positions and sequence, in finishing order - exactly against the restatement
tests/dbg_asm_ref.py (tests/test_dbg_asm_cpu.py asserts, on the CPU alone, that each case is what its name says)."""
import os
import subprocess

import numpy as np
import pytest

import dbg_asm_cases as AC
import dbg_asm_ref as AR
from genomicsbench_amd import dbg as D
from genomicsbench_amd import dbg_asm as A

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in AC.all_cases()}
COUNTS = ("k", "n_builds", "cyclic", "n_paths", "n_path_nodes", "n_gave_up", "n_steps")


def same(res, want, what):
    """a Result against the restatement's windows, and the layout of the starts, paths and path nodes"""
    assert len(res.wins) == len(want), what
    by_round = sorted(range(len(want)), key=lambda w: (want[w]["n_builds"], w))
    first_start = first_path = first_node = 0
    for w in by_round:
        got, h, where = res.window(w), want[w], "%s: window %d" % (what, w)
        for f in COUNTS:
            assert got[f] == h[f], "%s: %s is %d, the restatement has %d" % (where, f, got[f], h[f])
        assert got["stats"] == h["stats"], where
        assert (int(res.wins[w]["first_start"]), int(res.wins[w]["n_starts"])) == (first_start, len(h["starts"])), where
        for g, s in zip(got["starts"], h["starts"]):
            assert (g["win"], g["node"], g["edge"], g["status"]) == (w, s["node"], s["edge"], s["status"]), where
            assert (g["first_node"], g["n_nodes"]) == (first_node, sum(len(x["nodes"]) for x in s["paths"])), where
            assert g["paths"] == s["paths"], "%s: start at node %d edge %d" % (where, s["node"], s["edge"])
            first_node += g["n_nodes"]
        for s in range(first_start, first_start + len(h["starts"])):
            assert int(res.starts[s]["first_path"]) == first_path, where
            first_path += int(res.starts[s]["n_paths"])
        first_start += len(h["starts"])
    assert (len(res.starts), len(res.paths), len(res.path_nodes), len(res.path_seq)) == (first_start, first_path, first_node, first_node), what


def run(rs, ws, p, ap, want, what, work_bytes=None, caps=(1024, 1024, 1 << 16)):
    import torch
    same(A.assemble_host(rs, ws, p, ap, caps), want, what + " assemble_host")
    da = A.DeviceAsm(rs, ws, "cuda:0", p, ap, caps, work_bytes)
    assert da.assemble(torch.cuda.current_stream().cuda_stream) == 0, what
    torch.cuda.synchronize()
    res = da.results()
    same(res, want, what + " DeviceAsm")
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_cases(name):
    """Guards, by family.  cycles: a self-loop, a 2-cycle, a ring with a tail, pure rings of unary nodes, a diamond (no visited-flag shortcut), the READ-only edge at
    min_weight - 1 and min_weight, the weight-1 edge into a REF|READ node, a fifth successor that would close the ring, empty
    graphs, lines on either side of the wavefront width and of the LDS-to-workspace switch with and without a cycle behind
    them, 70 and 300 sources in the first trips, a cyclic window between acyclic ones and one window 256 times.  retry: runs
    that stop looping at k = 20, 30 and 55 or never, a reference that runs out, k_step 1, no retry, and batches whose cyclic
    subset shrinks to the last and to the first window.  paths: SNP, insertion and deletion at k = 3 and 15, the start edge
    and the extension edges at min_weight - 1 and min_weight, a dead end, read-only cycles dropped at the repeat, 2 to 4
    branches in finishing order, 20 / 21 / 22 finished paths, 20 / 21 pending, max_steps at and below the need, paths of 63
    to 1000 nodes, 0 / 65 / 257 starts and the starts of several windows in one call."""
    case = CASES[name]
    rs, ws, p = case.packed()
    run(rs, ws, p, case.asm_params(), case.want_asm(), name)


@pytest.mark.parametrize("name", ["shrinks_to_last", "shrinks_to_first", "run_60", "ref_runs_out", "cyclic_between_acyclic"])
def test_final_stats_are_the_build_at_the_final_k(name):
    """the stats of every window, byte for byte, against gbx_dbg_build_host at the window's final k"""
    case = CASES[name]
    rs, ws, p = case.packed()
    res = A.assemble_host(rs, ws, p, case.asm_params())
    for k in sorted(set(int(x) for x in res.wins["k"])):
        st = D.build_host(rs, ws, D.make_params(k, case.min_qual))
        for w in np.flatnonzero(res.wins["k"] == k):
            assert res.stats[w].tobytes() == st[w].tobytes(), (name, k, int(w))


@pytest.mark.parametrize("name", ["shrinks_to_first", "starts_of_several_windows", "long_cycle_256_times"])
def test_small_workspace(name):
    """The least workspace the entry takes (the head for the call, the searches' paths and the range area of the largest
    window alone, plus about 1.5 KB for every further window): the windows go in several ranges - the eight equal windows of
    shrinks_to_first one by one in every round, the 257-start window of starts_of_several_windows alone between two ranges -
    and the running totals, the plan and the offsets are carried from range to range."""
    from genomicsbench_amd import _native as N
    import ctypes
    case = CASES[name]
    rs, ws, p = case.packed()
    occ = int(ws.occ_slots(rs, case.k).max())
    size = lambda n_win, n_reads, max_occ: N.lib().gbx_dbg_assemble_workspace_bytes(ctypes.byref(p), n_win, n_reads, max_occ)  # noqa: E731
    small = size(1, 0, occ) + size(ws.n_win, rs.n_reads, 0) - size(1, 0, 0)
    run(rs, ws, p, case.asm_params(), case.want_asm(), name + " (small workspace)", work_bytes=small)
    with pytest.raises(N.GbxError):
        A.DeviceAsm(rs, ws, "cuda:0", p, case.asm_params(), work_bytes=size(1, 0, occ) - 1024).assemble(None)


def test_capacities():
    """short capacities: GBX_ERR_UNSUPPORTED, the totals say what to allocate, what fitted is as it would be with room, and
    the Python wrapper's second call has it all"""
    import torch
    from genomicsbench_amd import _native as N
    case = CASES["starts_65"]
    rs, ws, p = case.packed()
    want = case.want_asm()
    nodes = want[0]["n_path_nodes"]
    da = A.DeviceAsm(rs, ws, "cuda:0", p, case.asm_params(), caps=(65, 10, 33))
    assert da.assemble(torch.cuda.current_stream().cuda_stream) == N.GBX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert da.totals() == [65, 65, nodes]
    part, full = da.results(), A.assemble_host(rs, ws, p, case.asm_params(), caps=(1, 1, 1))
    same(full, want, "starts_65 (regrown)")
    assert part.starts.tobytes() == full.starts.tobytes() and part.paths.tobytes() == full.paths[:10].tobytes()
    assert part.path_nodes.tobytes() == full.path_nodes[:33].tobytes() and part.path_seq.tobytes() == full.path_seq[:33].tobytes()
    assert part.wins.tobytes() == full.wins.tobytes()


def test_arguments():
    from genomicsbench_amd import _native as N
    case = CASES["snp_k3"]
    rs, ws, p = case.packed()
    for bad in (dict(k_step=0), dict(min_weight=-1), dict(max_pending=A.MAX_PENDING + 1), dict(max_finished=-1), dict(max_steps=-1),
                dict(k_last=64, k_step=62)):
        with pytest.raises(N.GbxError):
            A.assemble_host(rs, ws, p, A.make_asm_params(**bad))
    res = A.assemble_host(rs, ws, D.make_params(60), A.make_asm_params(k_last=60, k_step=4))      # 60 -> 64: the largest k there is
    assert int(res.wins["k"][0]) == 60 and int(res.wins["cyclic"][0]) == 0


@pytest.mark.parametrize("name", ["dbg_adv", "dbg_var"])
def test_fixture(name):
    rs, ws = AC.fixture(name)
    run(rs, ws, D.make_params(), A.make_asm_params(), AC.fixture_want(name), name)


@pytest.mark.parametrize("name", ["dbg_adv", "dbg_var"])
def test_driver_assemble_print(name):
    """bin/dbg --assemble --print against the same text rendered from the restatement"""
    exe = os.path.join(os.path.dirname(os.path.abspath(A.__file__)), "bin", "dbg")
    out = subprocess.run([exe, os.path.join(AC.GOLDEN, name + ".bam"), "ctg1", os.path.join(AC.GOLDEN, name + ".fa"), "1", "--assemble", "--print"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    want = []
    for w in AC.fixture_want(name):
        want += [AR.line(w)] + AR.path_lines(w)
    assert out.stdout.decode("latin-1").splitlines() == want
