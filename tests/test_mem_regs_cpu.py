"""Alignment regions without a GPU: the restated rules (tests/mem_regs_ref.py) on the hand-built cases and their hand-written
outcomes, on the frozen worked example and on generated reads (invariants, no mapq on a log() boundary), hash_64, the exported
symbols and struct sizes, and the argument checks of the host entry that come before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mem_regs as MR
from genomicsbench_amd.bsw_seeds import SEED_DTYPE
import mem_regs_cases as K
import mem_regs_ref as R

OUT_FIELDS = ("seed", "secondary", "sub", "sub_n", "seedcov", "mapq", "flag", "sel")


@pytest.fixture(scope="module")
def generated():
    return [K.straddle(), K.synthetic(300, 21), K.synthetic(300, 22, read_id0=5000)]


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_cases_against_their_hand_written_outcomes(name):
    j = K.hand_built()[name]
    detail = []
    out = K.reference(j, sel_cap=len(j["seeds"]), detail=detail)
    assert len(j["expect"]) == len(j["l_rep"])
    for r, (made, want) in enumerate(j["expect"]):
        a, b = out["reg_off"][r], out["reg_off"][r + 1]
        assert detail[r]["made"] == made, (r, detail[r]["made"])
        got = [tuple(int(x[f]) for f in OUT_FIELDS) for x in out["regs"][a:b]]
        assert got == want, (r, got)
    assert out["boundary"] == 0


def test_every_branch_has_its_case():
    """What each case is there for does happen in it."""
    J = K.hand_built()

    def run(name):
        d = []
        return K.reference(J[name], sel_cap=len(J[name]["seeds"]), detail=d), d
    out, d = run("tenth_of_lq")
    assert len(d[0]["made"]) == 2 and len(d[1]["made"]) == 1               # kept by .1 lq; 10 is not above 10
    out, d = run("overlapping_seed")
    assert [len(x["made"]) for x in d] == [2, 2, 1]
    out, d = run("dedup")
    assert [x["after_dedup"] for x in d] == [[0], [3], [5]]                # p loses; q loses; a tie: q loses
    out, d = run("walk_rid")
    assert d[0]["after_dedup"] == [2] and sorted(d[1]["after_dedup"]) == [3, 4, 5]
    out, d = run("walk_max_chain_gap")
    assert sorted(d[0]["after_dedup"]) == [0, 2]
    out, d = run("identical_hit")
    assert len(d[0]["made"]) == 2 and len(d[0]["after_dedup"]) == 1
    out, _ = run("supplementary")
    g = out["regs"]
    assert g["flag"].tolist() == [1, 0, 0x801] and g["mapq"].tolist() == [9, 0, 9] and out["n_sel"] == 2
    lone = R.mapq_values(type("X", (), dict(sub=0, sub_n=0, score=45, qb=50, qe=100, rb=5050, re=5100, lq=100)), 0, R.params())
    assert lone == [60] * len(lone)                                        # uncapped it would have been 60
    out, _ = run("absent_and_empty")
    assert out["reg_off"].tolist() == [0, 1, 1, 2]
    # the CIGAR list mirrors the region and carries sc0 = 0 whatever the extension had there
    assert J["absent_and_empty"]["res"][1, 7] == 7 and out["sel_res"][0].tolist() == [100, 100, 0, 100, 100, 200, 100, 0]
    assert out["sel_seeds"][0] == J["absent_and_empty"]["seeds"][1] and (out["sel_res"][2:] == -1).all()


def test_worked_example_from_its_fixture():
    ex = K.example()
    chains = np.array([tuple(x) for x in ex["chains"]], dtype=R.CHAIN_DTYPE)
    seeds = np.array([tuple(x) for x in ex["seeds"]], dtype=R.SEED_DTYPE)
    assert ex["chain_fields"] == list(R.CHAIN_DTYPE.names) and ex["seed_fields"] == list(R.SEED_DTYPE.names)
    assert ex["reg_fields"] == list(R.REG_DTYPE.names) and ex["res_fields"] == list(R.RESULT_FIELDS)
    detail = []
    out = R.regs_all(chains, ex["chain_off"], seeds, np.array(ex["res"], dtype=np.int32), ex["l_rep"], R.params(), ex["read_id0"],
                     detail=detail)
    assert [x["made"] for x in detail] == ex["made"] and [x["after_dedup"] for x in detail] == ex["after_dedup"]
    assert out["reg_off"].tolist() == ex["reg_off"] and out["n_sel"] == ex["n_sel"]
    assert [[int(v) for v in row] for row in out["regs"].tolist()] == ex["regs"]
    n = ex["n_sel"]
    assert [[int(v) for v in row] for row in out["sel_seeds"][:n].tolist()] == ex["sel_seeds"] and out["sel_res"][:n].tolist() == ex["sel_res"]
    assert out["boundary"] == 0


def test_no_input_of_the_tests_lies_on_a_log_boundary(generated):
    """The GPU comparison is exact without a tolerance only if no mapq of the test inputs changes when a log() moves by an ulp."""
    others = [K.synthetic(1, 21), K.synthetic(2, 21), K.synthetic(20, 23)] + [K.synthetic(150, 40 + t, read_id0=1000 * t) for t in range(4)]
    for j in list(K.hand_built().values()) + generated + others:          # every input test_mem_regs_gpu.py generates
        assert K.reference(j)["boundary"] == 0
    x = type("X", (), dict(sub=0, sub_n=0, score=60, qb=0, qe=100, rb=0, re=100, lq=100))
    assert len(R.mapq_values(x, 0, R.params())) == 3 and len(R.mapq_values(x, 0, R.params(mapq_coef_len=200))) == 1


def test_invariants_on_generated_reads(generated):
    for j in generated:
        out = K.reference(j)
        g, off = out["regs"], out["reg_off"]
        P = K.p_of(j)
        assert off[0] == 0 and off[-1] == len(g) == out["n_regs"] and (np.diff(off) >= 0).all()
        rep = (g["flag"] & 1) != 0
        assert (g["secondary"][rep] < 0).all() and (g["score"][rep] >= P["T"]).all()
        assert ((g["flag"] & ~0x801) == 0).all() and (g["sel"][~rep] == -1).all() and (g["mapq"][g["secondary"] >= 0] == 0).all()
        assert (g["mapq"] >= 0).all() and (g["mapq"] <= 60).all()
        assert np.array_equal(g["sel"][rep], np.arange(out["n_sel"]))       # the CIGAR list follows the output order
        res = j["res"]
        for r in range(len(off) - 1):
            a = g[off[r]:off[r + 1]]
            assert (a["read"] == r).all()
            assert (np.diff(a["score"]) <= 0).all()                          # output order: score descending
            for i, x in enumerate(a):
                if x["secondary"] >= 0:                                       # a secondary points at an earlier primary
                    assert x["secondary"] < i and a[x["secondary"]]["secondary"] < 0
            first = a[(a["flag"] & 1) != 0]
            if len(first):
                assert (first["flag"][1:] == 0x801).all() and first["flag"][0] == 1 and (first["mapq"] <= first["mapq"][0]).all()
            c0, c1 = j["chain_off"][r], j["chain_off"][r + 1]
            lo = j["chains"][c0]["seed_off"] if c1 > c0 else 0
            hi = lo + int(j["chains"][c0:c1]["n_seeds"].sum())
            assert len(set(a["seed"].tolist())) == len(a) and ((a["seed"] >= lo) & (a["seed"] < hi)).all()
        s = j["seeds"][g["seed"]]
        assert (res[g["seed"], 2] >= 0).all()                                 # never from an absent seed
        assert np.array_equal(g["rb"], s["roff"] + res[g["seed"], 4]) and np.array_equal(g["seedlen0"], s["len"])
        n = out["n_sel"]
        k = g[rep]
        assert out["sel_seeds"][:n].tobytes() == j["seeds"][k["seed"]].tobytes()
        want = np.stack([k["score"], k["truesc"], k["qb"], k["qe"], k["rb"] - s[rep]["roff"], k["re"] - s[rep]["roff"], k["w"], 0 * k["w"]], 1)
        assert np.array_equal(out["sel_res"][:n], want)
        assert (out["sel_res"][n:] == -1).all() and not out["sel_seeds"][n:].tobytes().strip(b"\0")
    st = K.reference(generated[0])
    assert np.diff(st["reg_off"]).tolist()[:9] == [0, 1, 2, 63, 64, 65, 130, 70, 130]
    assert (st["regs"]["flag"] == 0x801).sum() > 64 and (st["regs"]["secondary"] >= 0).sum() > 64


def test_hash_64_on_frozen_values():
    """bwa's hash_64 (Thomas Wang's 64-bit mix); the values come from the C function compiled on its own."""
    for k, v in ((0, 0x6a396cd39c352659), (1, 0x20353c45b09bc659), (1000, 0x66f2b87ef0e0de60), (1234567, 0xf34e955a234fcbca),
                 ((1 << 64) - 1, 0x9d7b7a2832582c16)):
        assert R.hash_64(k) == v, hex(k)
    assert R.hash_64(1000) == R.hash_64(1000 + (1 << 64))
    assert len({R.hash_64(k) for k in range(5000)}) == 5000


def test_new_symbols_are_exported_and_the_struct_sizes_agree():
    L = N.lib()
    for name in ("gbx_mem_regs_default_params", "gbx_mem_regs_workspace_bytes", "gbx_mem_regs_device", "gbx_mem_regs_host"):
        assert hasattr(L, name), name
    p = MR.make_params()
    for k, v in R.DEFAULTS.items():
        assert getattr(p, k) == (np.float32(v) if isinstance(v, float) else v), k
    assert C.sizeof(MR.RegsParams) == 64 and MR.REG_DTYPE == R.REG_DTYPE and MR.REG_DTYPE.itemsize == 88
    # the sizes gbx.h states
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gbx.h")) as f:
        h = f.read()
    assert re.search(r"typedef struct gbx_mem_regs_params \{\s*/\* (\d+) bytes", h).group(1) == "64"
    assert re.search(r"typedef struct gbx_mem_reg \{\s*/\* (\d+) bytes", h).group(1) == "88"
    assert MR.lib().gbx_mem_regs_workspace_bytes(1000, 400000) > 400000 * 100
    assert MR.make_params(mapq_coef_len=100).mapq_coef_fac == np.float32(np.log(100.0))
    with pytest.raises(TypeError):
        MR.make_params(zdrop=100)


def host_rc(j, **params):
    try:
        MR.regs_host(MR.make_params(**dict(j["params"], **params)), j["chains"], j["chain_off"], j["seeds"], j["res"], j["l_rep"])
    except N.GbxError as e:
        return e.code, str(e)
    return 0, ""


def test_host_entry_checks_its_arguments_before_a_device_is_touched():
    """GBX_ERR_ARG / GBX_ERR_UNSUPPORTED, not GBX_ERR_NO_DEVICE: these returns come before the first HIP call."""
    j = K.hand_built()["absent_and_empty"]
    for bad in (dict(e_del=0), dict(e_ins=0), dict(a=0), dict(a=1, b=-1), dict(w=-1)):
        rc, msg = host_rc(j, **bad)
        assert rc == N.GBX_ERR_ARG and any(k in msg for k in bad), (bad, rc, msg)
    rc, msg = host_rc(j, mapq_coef_len=0)
    assert rc == N.GBX_ERR_UNSUPPORTED and "mapq_coef_len" in msg
    off = j["chain_off"].copy()
    off[1], off[2] = off[2] + 1, off[1]
    rc, msg = host_rc(dict(j, chain_off=off))
    assert rc == N.GBX_ERR_ARG and "chain_off" in msg and "read 1" in msg
    off = j["chain_off"].copy()
    off[-1] += 1
    assert host_rc(dict(j, chain_off=off))[0] == N.GBX_ERR_ARG
    ch = j["chains"].copy()
    ch["n_seeds"][1] += 2                             # chains 1 and 2 both end past the seeds then: the lowest is named
    ch["n_seeds"][2] += 5
    rc, msg = host_rc(dict(j, chains=ch))
    assert rc == N.GBX_ERR_ARG and "chain 1" in msg
    ch = j["chains"].copy()
    ch["seed_off"][0] = -1
    rc, msg = host_rc(dict(j, chains=ch))
    assert rc == N.GBX_ERR_ARG and "chain 0" in msg


def test_alignments_joins_regions_and_cigars():
    from genomicsbench_amd.mem_cigar import ALN_DTYPE
    out = K.reference(K.hand_built()["supplementary"])
    alns = np.zeros(2, dtype=ALN_DTYPE)
    alns["rid"], alns["pos"], alns["is_rev"], alns["n_cigar"], alns["cigar_off"], alns["nm"] = [0, 0], [1000, 5050], [0, 1], [2, 2], [0, 2], [0, 3]
    cigar = np.array([50 << 4, 50 << 4 | 4, 50 << 4 | 4, 50 << 4], dtype=np.uint32)
    assert MR.alignments(out["regs"], alns, cigar) == [(0, 0, 1000, 0, 9, 0, "50M50S", 0), (0, 0, 5050, 1, 9, 0x810, "50S50M", 3)]
