"""The dbg_asm restatement (tests/dbg_asm_ref.py) on the CPU: against the recorded dumps of the reference's own compiled
detectCyclesInGraph_Recursive and getVariantPathsThroughGraphFromNode on the two fixtures (tests/golden/dbg_asm_reference.json),
against a second cycle check of another kind, and every hand-made case of tests/dbg_asm_cases.py against what its name says."""
import gzip
import json
import os

import numpy as np
import pytest

import dbg_asm_cases as AC
import dbg_asm_ref as AR
import dbg_ref as R

CASES = {c.name: c for c in AC.all_cases()}


def peel(nodes, min_weight):
    """cyclic by peeling nodes of in-degree 0 (the kernel's kind of method; the restatement walks depth first)"""
    deg = [0] * len(nodes)
    for nd in nodes:
        for e, w in nd["edges"]:
            deg[e] += AR.counted(nodes, e, w, min_weight)
    todo = [i for i, d in enumerate(deg) if d == 0]
    left = len(nodes)
    while todo:
        left -= 1
        for e, w in nodes[todo.pop()]["edges"]:
            if AR.counted(nodes, e, w, min_weight):
                deg[e] -= 1
                if deg[e] == 0:
                    todo.append(e)
    return left != 0


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_what_its_name_says(name):
    case = CASES[name]
    case.check(case)
    for w in case.want_asm():
        assert w["cyclic"] == peel(w["nodes"], case.ap["min_weight"])


def test_families_cover_the_limits():
    """the cases sit on the kernel's own limits: the wavefront width and the LDS-to-workspace switch, as the source has them"""
    src = open(os.path.join(os.path.dirname(AC.GOLDEN), os.pardir, "genomicsbench_amd", "csrc", "gbx_internal.h")).read()
    assert "constexpr int DBG_ASM_LDS_NODES = %d;" % AC.LDS_NODES in src
    for n in (AC.WAVE - 1, AC.WAVE, AC.WAVE + 1, AC.LDS_NODES - 1, AC.LDS_NODES, AC.LDS_NODES + 1):
        for tail in ("", "_cycle"):
            assert CASES["line_%d%s" % (n, tail)].want()[0][0]["n_nodes"] == n


def test_dbg_var_is_its_generator(tmp_path):
    """tests/golden/dbg_var.bam / .fa are gen_dbg_reads(6000, 30, 7): the same reads and contig"""
    from genomicsbench_amd import dbg as D, pileup as P
    from genomicsbench_amd.datagen import gen_dbg_reads
    contigs, recs, fa = gen_dbg_reads(6000, 30, 7)
    assert open(os.path.join(AC.GOLDEN, "dbg_var.fa"), "rb").read() == fa
    P.write_bam(str(tmp_path / "again.bam"), contigs, recs)
    a, ra, _ = D.read_bam(str(tmp_path / "again.bam"), "ctg1")
    b, rb, _ = D.read_bam(os.path.join(AC.GOLDEN, "dbg_var.bam"), "ctg1")
    assert ra == rb
    for f in ("seq_off", "seq", "qual", "flag", "pos", "end"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_fixture_figures():
    """what the two fixtures pin: dbg_adv the cycle check and the retry to its end, dbg_var the paths"""
    adv, var = AC.fixture_want("dbg_adv"), AC.fixture_want("dbg_var")
    assert [(w["k"], w["cyclic"]) for w in adv] == [(50, 0)] + [(55, 0)] * 5
    assert sum(len(w["starts"]) for w in adv) == 2 and sum(w["n_paths"] for w in adv) == 0
    assert [(w["k"], w["cyclic"]) for w in var] == [(15, 0)] + [(20, 0)] * 6 + [(15, 0)]
    starts = [s for w in var for s in w["starts"]]
    lens = [len(x["nodes"]) for s in starts for x in s["paths"]]
    assert (len(starts), len(lens), min(lens), max(lens)) == (18, 12, 17, 24)
    assert all(s["status"] == AR.OK for s in starts) and max(s["steps"] for s in starts) <= 23


def dump_lines(name):
    """the restatement in the recorded dump's text form (tests/golden/dbg_asm_reference.json: "format")"""
    from genomicsbench_amd import dbg as D
    rs, ws = AC.fixture(name)
    p = AR.params()
    out = []
    for w in range(ws.n_win):
        ref, pos = ws.window_ref(w), int(ws.ref_pos[w])
        reads = [rs.read(r) for r in range(int(ws.read_lo[w]), int(ws.read_hi[w]))]
        k, tries = 15, []
        while True:
            nodes, _ = R.graph(ref, pos, reads, k)
            cyc = AR.cyclic(nodes, p["min_weight"])
            tries.append("%d:%d" % (k, cyc))
            if not cyc or k > p["k_last"]:
                break
            k += p["k_step"]
        out.append("W %d %s" % (w, " ".join(tries)))
        for i, j in AR.starts(nodes, p["min_weight"]):
            status, fin, _, _ = AR.search(nodes, i, j, p)
            out.append("S %d %d %s %d" % (i, j, "NULL" if status == AR.GAVE_UP else "OK", len(fin)))
            for path, wt in fin:
                out.append("P %d %s %s" % (wt, ",".join(str(v) for v in path), bytes(nodes[v]["kmer"][0] for v in path).decode("latin-1")))
    return out


@pytest.mark.parametrize("name", ["dbg_adv", "dbg_var"])
def test_restatement_against_the_reference_dump(name):
    meta = json.load(open(os.path.join(AC.GOLDEN, "dbg_asm_reference.json")))
    with gzip.open(os.path.join(AC.GOLDEN, meta["dumps"][name]["file"]), "rt", encoding="latin-1") as f:
        want = f.read().splitlines()
    assert dump_lines(name) == want
