"""Paired-end without a GPU: the restated rules (tests/mem_pair_ref.py) on the hand-built cases and their hand-written outcomes,
on the frozen worked example and on generated pairs (invariants, no boundary input), infer_dir, the two summation orders of the
estimate, the exported symbols and struct sizes, the argument checks of the host entry that come before a device is touched, and
sam_fields."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mem_pair as MP
import mem_pair_cases as K
import mem_pair_ref as R


def rows(a, fields):
    return [tuple(int(x[f]) for f in fields) for x in a]


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_cases_against_their_hand_written_outcomes(name):
    j = K.hand_built()[name]
    out = K.reference(j)
    ex = j["expect"]
    assert rows(out["pairs"], K.PAIR_FIELDS) == [tuple(x) for x in ex["pairs"]]
    if ex["pes"] is not None:
        got = [tuple(x) for x in out["pes"][["low", "high", "failed", "avg", "std"]].tolist()]
        assert got == [tuple(x) for x in ex["pes"]]
    assert out["boundary"] == 0, out["notes"]


def test_infer_dir_on_every_value():
    """L = 1000; b >= L is the reverse strand, 2L - 1 - b its forward coordinate."""
    for b1, b2, want in ((100, 400, (0, 300)), (400, 100, (3, 300)), (100, 100, (3, 0)),       # same strand, ahead / behind / equal
                         (1100, 1400, (0, 300)), (1400, 1100, (3, 300)),
                         (100, 1599, (1, 300)),                                               # p2 = 1999 - 1599 = 400 > 100
                         (400, 1899, (2, 300)),                                               # p2 = 100 < 400
                         (1599, 100, (1, 300)),                                               # p2 = 1899 > 1599
                         (1899, 400, (2, 300))):                                              # p2 = 1599 < 1899
        assert R.infer_dir(1000, b1, b2) == want, (b1, b2)
    assert {R.infer_dir(1000, a, b)[0] for a in (10, 700, 1300, 1990) for b in (10, 700, 1300, 1990)} == {0, 1, 2, 3}


def test_every_branch_has_its_case():
    """What each case is there for does happen in it."""
    J = K.hand_built()
    ref = lambda name: K.reference(J[name])
    out = ref("nine_against_ten")
    assert [len(v) for v in out["insert_sizes"]] == [9, 10, 0, 0] and out["pes"]["failed"].tolist() == [1, 0, 1, 1]
    out = ref("five_percent")
    assert [len(v) for v in out["insert_sizes"]] == [10, 220, 0, 0] and out["pes"]["failed"].tolist() == [1, 0, 1, 1]
    assert out["pes"]["high"][0] == 318                              # failed by the 5 % rule: the numbers stay
    out = ref("four_std_clamps")
    assert (out["pes"]["low"][1], out["pes"]["high"][1]) == (172, 428) != (290 - 60, 310 + 60)
    assert [len(v) for v in ref("cal_sub_and_contig")["insert_sizes"]] == [0, 10, 0, 0]     # neither the 11th nor the 12th pair counts
    assert ref("erfc_underflow")["pairs"]["n_cand"][0] == 1 and math.erfc(100 * math.sqrt(.5)) == 0.
    a, b = ref("hash_tie_a"), ref("hash_tie_b")                     # the same q twice; the hash picks another mate for another pair id
    assert a["pairs"]["score"][0] == a["pairs"]["sub"][0] == 180 and a["pairs"]["dist"][0] != b["pairs"]["dist"][0]
    out = ref("z_on_secondary")
    g = out["pregs"]
    assert J["z_on_secondary"]["regs"]["secondary"].tolist() == [-1, -1, 0]
    assert g["secondary"].tolist() == [-1, -1, -2] and g["sub"][2] == 100 and g["flag"].tolist() == [1, 0, 1] and g["mapq"][2] == 40
    assert g["sel"].tolist() == [0, -1, 1] and out["n_psel"] == 2
    # a region the regs stage did not report (25 < T) is chosen: its records are built
    j = J["below_T"]
    out = ref("below_T")
    assert j["regs"]["flag"].tolist() == [1, 0] and len(j["sel_seeds"]) == 1 and out["n_psel"] == 2
    x = j["regs"][1]
    s = j["seeds"][int(x["seed"])]
    assert out["psel_seeds"][1] == s
    assert out["psel_res"][1].tolist() == [25, 25, 0, 25, int(x["rb"] - s["roff"]), int(x["re"] - s["roff"]), 100, 0]
    out = ref("is_multi_proper")                                    # the unpaired way: both of the mate's hits stay, the second supplementary
    assert out["pregs"]["flag"].tolist() == [1, 1, 0x801] and out["pregs"]["sel"].tolist() == [0, 1, 2]
    assert ref("no_pairing")["pairs"]["n_cand"][0] == 0 and ref("other_contig")["pairs"]["n_cand"][0] == 0


def test_the_two_summation_orders():
    """pestat_bwa adds S one value at a time; on these inputs the agreed order gives the same bounds, and avg / std within
    1e-12.  An input on which they part is reported as a boundary input."""
    j = K.gpu_inputs()["many"]
    out = K.reference(j)
    bwa = R.pestat_bwa(out["insert_sizes"])
    for d in range(4):
        p = out["pes"][d]
        assert (p["low"], p["high"], p["failed"]) == bwa[d][:3]
        assert abs(p["std"] - bwa[d][4]) <= 1e-12 * bwa[d][4] and p["avg"] == bwa[d][3]
    bd = R.Boundary()
    # p25 / p75 = 300 / 301: [300 - 3, 301 + 3], which avg -+ 4 std = [298.5, 302.5] does not move
    assert R.pestat_one([300] * 5 + [301] * 5, bd) == (297, 304, 0, 300.5, .5) and bd.n == 0
    # (int) truncates towards zero; a truncated quantity within 1e-9 of an integer is noted
    assert R.Boundary().trunc(2.5, "x") == 2 and R.Boundary().trunc(-2.5, "x") == -2
    bd = R.Boundary()
    bd.trunc(200.0000000001, "qd")
    assert bd.n == 1


def test_worked_example_from_its_fixture():
    ex = K.example()
    assert ex["reg_fields"] == list(R.REG_DTYPE.names) and ex["seed_fields"] == list(R.SEED_DTYPE.names)
    assert ex["pestat_fields"] == list(R.PESTAT_DTYPE.names) and ex["pair_fields"] == list(R.PAIR_DTYPE.names)
    arr = lambda k, dt: np.array([tuple(x) for x in ex[k]], dtype=dt)
    out = R.pair_all(arr("regs", R.REG_DTYPE), ex["reg_off"], arr("sel_seeds", R.SEED_DTYPE), np.array(ex["sel_res"], dtype=np.int32),
                     arr("seeds", R.SEED_DTYPE), ex["l_rep"], ex["L"], ex["contig_off"], R.params(), ex["pair_id0"])
    assert out["insert_sizes"] == ex["insert_sizes"] and out["n_psel"] == ex["n_psel"] and out["boundary"] == 0
    assert out["pes"].tobytes() == arr("pes", R.PESTAT_DTYPE).tobytes()
    assert out["pairs"].tobytes() == arr("pairs", R.PAIR_DTYPE).tobytes()
    assert out["pregs"].tobytes() == arr("pregs", R.REG_DTYPE).tobytes()
    n = ex["n_psel"]
    assert out["psel_seeds"][:n].tobytes() == arr("psel_seeds", R.SEED_DTYPE).tobytes() and out["psel_res"][:n].tolist() == ex["psel_res"]


def test_no_input_of_the_tests_is_a_boundary_input():
    """The GPU comparison is exact without a tolerance only if no truncated quantity of the test inputs lies within 1e-9 of an
    integer and bwa's summation order gives the same estimate."""
    for name, j in list(K.hand_built().items()) + list(K.gpu_inputs().items()):
        out = K.reference(j)
        assert out["boundary"] == 0, (name, out["notes"][:3])


def test_invariants_on_generated_pairs():
    for name in ("many", "many_id0", "straddle", "given"):
        j = K.gpu_inputs()[name]
        out = K.reference(j)
        P = K.p_of(j)
        g, pr, off, src = out["pregs"], out["pairs"], j["reg_off"], j["regs"]
        assert len(g) == len(src) and len(pr) == (len(off) - 1) // 2
        same = [f for f in g.dtype.names if f not in ("sub", "secondary", "mapq", "flag", "sel")]
        assert all(np.array_equal(g[f], src[f]) for f in same)
        rep = (g["flag"] & 1) != 0
        assert np.array_equal(g["sel"][rep], np.arange(out["n_psel"])) and (g["sel"][~rep] == -1).all()
        assert out["n_psel"] <= len(g)
        for p, x in enumerate(pr):
            for e, z in ((0, x["z0"]), (1, x["z1"])):
                a = g[off[2 * p + e]:off[2 * p + e + 1]]
                assert -1 <= z < max(len(a), 1)
                if x["paired"]:
                    assert a["flag"].tolist() == [int(i == z) for i in range(len(a))] and a["mapq"][z] == x["q_se%d" % e]
                else:
                    assert a.tobytes() == out["pregs"][off[2 * p + e]:off[2 * p + e + 1]].tobytes()
                    assert (z == 0) == (len(a) > 0 and a["score"][0] >= P["T"])
            assert (x["dir"] == -1) == (min(x["z0"], x["z1"]) < 0) and 0 <= x["q_pe"] <= 60
            assert not x["proper"] or (x["z0"] >= 0 and x["z1"] >= 0)
            assert x["n_sub"] <= max(x["n_cand"] - 1, 0) and (x["n_cand"] > 0 or x["score"] == 0)
        n = out["n_psel"]
        assert (out["psel_res"][n:] == -1).all() and not out["psel_seeds"][n:].tobytes().strip(b"\0")
        k = g[rep]
        s = j["seeds"][k["seed"]]
        assert out["psel_seeds"][:n].tobytes() == s.tobytes()
        assert np.array_equal(out["psel_res"][:n, 0], k["score"]) and np.array_equal(out["psel_res"][:n, 4], k["rb"] - s["roff"])
    out = K.reference(K.gpu_inputs()["many"])
    assert out["pes"]["failed"].tolist() == [0, 0, 0, 1] and all(len(v) > 0 for v in out["insert_sizes"])     # all four occur, RR below ten
    assert out["pairs"]["proper"].sum() > 250 and (out["pairs"]["paired"] == 0).sum() > 10
    st = K.gpu_inputs()["straddle"]
    assert (np.diff(st["reg_off"])[0::2] + np.diff(st["reg_off"])[1::2]).tolist() == [63, 64, 65, 200, 98]
    assert K.reference(st)["pairs"]["n_cand"][4] == 6                # 89 skipped below low, one at low and five beyond, the walk ended by high


def test_new_symbols_are_exported_and_the_struct_sizes_agree():
    L = N.lib()
    for name in ("gbx_mem_pair_default_params", "gbx_mem_pair_workspace_bytes", "gbx_mem_pair_device", "gbx_mem_pair_host"):
        assert hasattr(L, name), name
    p = MP.make_params()
    for k, v in R.DEFAULTS.items():
        assert getattr(p, k) == (np.float32(v) if isinstance(v, float) else v), k
    assert C.sizeof(MP.PairParams) == 56 and MP.PAIR_DTYPE == R.PAIR_DTYPE and MP.PESTAT_DTYPE == R.PESTAT_DTYPE
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gbx.h")) as f:
        h = f.read()
    assert re.search(r"typedef struct gbx_mem_pair_params \{\s*/\* (\d+) bytes", h).group(1) == "56"
    assert re.search(r"typedef struct gbx_mem_pestat \{\s*/\* (\d+) bytes", h).group(1) == "32"
    assert re.search(r"typedef struct gbx_mem_pair \{\s*/\* (\d+) bytes", h).group(1) == "56"
    w = MP.lib().gbx_mem_pair_workspace_bytes
    assert w(1000, 5000, 10000) > 5000 * 32 + 4 * 10001 * 4 and w(1000, 5000, 1 << 20) - w(1000, 5000, 10000) >= 16 * ((1 << 20) - 10000)
    with pytest.raises(TypeError):
        MP.make_params(w=100)


def host_rc(j, pair_id0=None, pes_in=None, **params):
    try:
        MP.pair_host(MP.make_params(**dict(j["params"], **params)), j["regs"], j["reg_off"], j["sel_seeds"], j["sel_res"], j["seeds"], j["l_rep"],
                     j["L"], j["contig_off"], j["pair_id0"] if pair_id0 is None else pair_id0, j["pes_in"] if pes_in is None else pes_in)
    except N.GbxError as e:
        return e.code, str(e)
    return 0, ""


def test_host_entry_checks_its_arguments_before_a_device_is_touched():
    """GBX_ERR_ARG / GBX_ERR_UNSUPPORTED, not GBX_ERR_NO_DEVICE: these returns come before the first HIP call."""
    j = K.hand_built()["n_sub"]
    for bad in (dict(e_del=0), dict(e_ins=0), dict(a=0), dict(max_ins=0), dict(max_ins=(1 << 20) + 1)):
        rc, msg = host_rc(j, **bad)
        assert rc == N.GBX_ERR_ARG and any(k in msg for k in bad), (bad, rc, msg)
    rc, msg = host_rc(j, mapq_coef_len=0)
    assert rc == N.GBX_ERR_UNSUPPORTED and "mapq_coef_len" in msg
    for pid in (-1, 1 << 23):                        # 2^23 - 1 + one pair is the last that fits
        rc, msg = host_rc(j, pair_id0=pid)
        assert rc == N.GBX_ERR_ARG and "pair_id0" in msg
    off = j["reg_off"].copy()
    off[1] = off[2] + 1
    rc, msg = host_rc(dict(j, reg_off=off))
    assert rc == N.GBX_ERR_ARG and "reg_off" in msg and "read 1" in msg
    off = j["reg_off"].copy()
    off[-1] += 1
    assert host_rc(dict(j, reg_off=off))[0] == N.GBX_ERR_ARG
    g = j["regs"].copy()
    g["rid"][2], g["rid"][3] = 2, -1                 # the lowest offender is named
    rc, msg = host_rc(dict(j, regs=g))
    assert rc == N.GBX_ERR_ARG and "region 2" in msg and "rid" in msg
    g = j["regs"].copy()
    g["seed"][1] = len(j["seeds"])
    rc, msg = host_rc(dict(j, regs=g))
    assert rc == N.GBX_ERR_ARG and "region 1" in msg and "seed" in msg
    rc, msg = host_rc(j, pes_in=[K.FAILED, (100, 500, 0, 300., 0.), K.FAILED, K.FAILED])
    assert rc == N.GBX_ERR_ARG and "direction 1" in msg and "std" in msg
    co = j["contig_off"].copy()
    co[1] = 0
    assert host_rc(dict(j, contig_off=co))[0] == N.GBX_ERR_ARG


def test_sam_fields():
    """A proper FR pair (read 0 forward at 1000, its mate reverse, 100M at 1201) and a pair whose second end has nothing."""
    from genomicsbench_amd.mem_cigar import ALN_DTYPE
    pairs = np.zeros(2, dtype=MP.PAIR_DTYPE)
    pairs["proper"] = [1, 0]
    g = np.zeros(3, dtype=MP.REG_DTYPE)
    g["read"], g["flag"], g["sel"], g["mapq"] = [0, 1, 2], [1, 1, 1], [0, 1, 2], [60, 48, 37]
    alns = np.zeros(3, dtype=ALN_DTYPE)
    alns["rid"], alns["pos"], alns["is_rev"], alns["n_cigar"], alns["cigar_off"] = [0, 0, 1], [1000, 1201, 77], [0, 1, 1], [1, 1, 2], [0, 1, 2]
    cigar = np.array([100 << 4, 100 << 4, 90 << 4, 10 << 4 | 4], dtype=np.uint32)
    assert MP.sam_fields(pairs, g, alns, cigar) == [
        (0, 0x1 | 0x2 | 0x40 | 0x20, 0, 1000, 60, "100M", 0, 1201, 301),          # p0 = 1000, p1 = 1201 + 99: -(1000 - 1300 - 1)
        (1, 0x1 | 0x2 | 0x80 | 0x10, 0, 1201, 48, "100M", 0, 1000, -301),
        (2, 0x1 | 0x40 | 0x8 | 0x10 | 0x20, 1, 77, 37, "90M10S", 1, 77, 0),        # the unmapped mate takes its place and strand
        (3, 0x1 | 0x80 | 0x4 | 0x10 | 0x20, 1, 77, 0, "*", 1, 77, 0)]
