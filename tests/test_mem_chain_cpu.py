"""Seed chaining without a GPU: the restated rules (tests/mem_chain_ref.py) on the frozen worked example and on generated reads,
the exported symbols, and the argument checks of the host entry that come before a device is touched."""
import ctypes as C

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd.bsw_seeds import SEED_DTYPE
import mem_chain_cases as K
import mem_chain_ref as R


def test_worked_example_from_its_fixture():
    ex = K.example()
    J = K.hand_built()
    for name in ("example", "example_min_seed_len_10"):
        got = K.reference(J[name])
        assert got["fates"] == [ex["fates"]] and got["made"] == [ex["chains_made"]]
        assert got["chain_off"].tolist() == [0, len(ex["chains"])]
        assert got["l_rep"].tolist() == [ex["l_rep"]]
        for g, w in zip(got["chains"], ex["chains"]):
            assert {k: int(g[k]) for k in w} == w
        assert len(got["seeds"]) == len(ex["seed_records"])
        for g, w in zip(got["seeds"], ex["seed_records"]):
            assert {k: int(g[k]) for k in w} == w
    assert ex["variant"]["params"] == J["example_min_seed_len_10"]["params"]


def test_the_scan_drops_a_chain_that_nothing_rescues():
    got = K.reference(K.hand_built()["filter"])
    a, b = got["chain_off"][2], got["chain_off"][3]
    ch = got["chains"][a:b]
    assert got["made"][2] == 3 and ch["pos"].tolist() == [5000, 2000] and ch["kept"].tolist() == [3, 1]


@pytest.fixture(scope="module")
def generated():
    return [K.synthetic(300, 11, many=(5, 77)), K.synthetic(200, 12, L=9000, contig_off=[0, 700, 760, 4000, 9000], many=(9,))]


def test_both_lookups_of_lower_agree(generated):
    jobs = list(K.hand_built().values()) + generated
    for j in jobs:
        a, b = K.reference(j, "bisect"), K.reference(j, "scan")
        K.same(a, b)
        assert a["fates"] == b["fates"]
    assert max(K.reference(generated[0])["made"]) > 64


def test_reference_invariants_on_generated_reads(generated):
    for j in generated:
        out = K.reference(j)
        L, co = j["L"], j["contig_off"]
        chains, seeds = out["chains"], out["seeds"]
        for r in range(len(j["read_len"])):
            hits = [(int(j["m"][q]), int(j["n"][q]) + 1 - int(j["m"][q]), int(j["pos"][h])) for q in range(j["smem_off"][r], j["smem_off"][r + 1])
                    for h in range(j["pos_off"][q], j["pos_off"][q + 1])]
            fate = out["fates"][r]
            assert len(fate) == len(hits)
            # every hit is in exactly one chain, or was dropped as contained, or was skipped for contig < 0
            for (q, ln, rb), f in zip(hits, fate):
                crosses = rb < 0 or R.contig_of(rb, rb + ln, L, co.tolist()) < 0
                assert (f == "skipped") == crosses
                assert f in ("skipped", "contained") or 0 <= f < out["made"][r]
            # the kept chains' seeds are exactly the hits with that chain's id, in order
            ids = {}
            for (q, ln, rb), f in zip(hits, fate):
                if isinstance(f, int):
                    ids.setdefault(f, []).append((q, ln, rb))
            for c in chains[out["chain_off"][r]:out["chain_off"][r + 1]]:
                sd = seeds[c["seed_off"]:c["seed_off"] + c["n_seeds"]]
                got = [(int(x["qbeg"]), int(x["len"]), int(x["rbeg"] + x["roff"])) for x in sd]
                assert got in list(ids.values()) and got[0][2] == c["pos"]
        # every emitted seed satisfies the gbx_bsw_seed rules, inside the 2 L text and the reads' arena
        assert (seeds["qbeg"] >= 0).all() and (seeds["len"] >= 1).all() and (seeds["qbeg"] + seeds["len"] <= seeds["lq"]).all()
        assert (seeds["rbeg"] >= 0).all() and (seeds["rbeg"] + seeds["len"] <= seeds["rlen"]).all()
        assert (seeds["roff"] >= 0).all() and (seeds["roff"] + seeds["rlen"] <= 2 * L).all()
        assert (seeds["qoff"] >= 0).all() and (seeds["qoff"] + seeds["lq"] <= int(j["read_len"].sum())).all()
        # every window lies inside one contig on one strand
        for c in chains:
            r0, r1 = int(c["rmax0"]), int(c["rmax1"])
            assert r0 < r1 and R.contig_of(r0, r1, L, co.tolist()) == c["contig"]
        assert sorted(set(chains["kept"].tolist())) == [1, 2, 3] and (out["l_rep"] > 0).any()


def test_new_symbols_are_exported():
    L = N.lib()
    for name in ("gbx_mem_chain_default_params", "gbx_mem_chain_workspace_bytes", "gbx_mem_chain_device", "gbx_mem_chain_host"):
        assert hasattr(L, name), name
    p = MC.make_params()
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert C.sizeof(MC.ChainParams) == 56 and MC.CHAIN_DTYPE == R.CHAIN_DTYPE and SEED_DTYPE == R.SEED_DTYPE
    assert MC.lib().gbx_mem_chain_workspace_bytes(1000, 24000, 400000) > 400000 * 100
    with pytest.raises(TypeError):
        MC.make_params(zdrop=100)


def test_text_of_is_genome_plus_reverse_complement():
    g = np.array([0, 1, 2, 3, 3, 0], dtype=np.uint8)
    assert MC.text_of(g).tolist() == [0, 1, 2, 3, 3, 0, 3, 0, 0, 1, 2, 3]


def host_rc(j, **params):
    sm = np.zeros(len(j["m"]), dtype=FM.SMEM_DTYPE)
    sm["m"], sm["n"], sm["s"] = j["m"], j["n"], j["s"]
    rs = FM.FmiReadSet(np.zeros(int(j["read_len"].sum()), np.uint8), j["read_off"], j["read_len"])
    try:
        MC.chain_host(MC.make_params(**params), sm, j["smem_off"], j["pos"], j["pos_off"], rs, j["L"], j["contig_off"])
    except N.GbxError as e:
        return e.code, str(e)
    return 0, ""


def test_host_entry_checks_its_arguments_before_a_device_is_touched():
    """GBX_ERR_ARG (-1), not GBX_ERR_NO_DEVICE: these returns come before the first HIP call."""
    j = K.hand_built()["contigs"]
    bad = dict(j, contig_off=np.array([0, 650, 300, 1000], dtype=np.int64))
    rc, msg = host_rc(bad)
    assert rc == N.GBX_ERR_ARG and "contig_off" in msg
    bad = dict(j, contig_off=np.array([0, 300, 650, 999], dtype=np.int64))
    assert host_rc(bad)[0] == N.GBX_ERR_ARG
    rc, msg = host_rc(j, e_del=0)
    assert rc == N.GBX_ERR_ARG and "e_del" in msg
    assert host_rc(j, e_ins=0)[0] == N.GBX_ERR_ARG and host_rc(j, w=-1)[0] == N.GBX_ERR_ARG
    off = j["smem_off"].copy()
    off[1], off[2] = off[2], off[1] - 1
    rc, msg = host_rc(dict(j, smem_off=off))
    assert rc == N.GBX_ERR_ARG and "smem_off" in msg
    off = j["pos_off"].copy()
    off[2] = off[1] - 1
    assert host_rc(dict(j, pos_off=off))[0] == N.GBX_ERR_ARG
