"""The SAM-record rules on the CPU: the restatement tests/mem_sam_ref.py against hand-built cases whose lines are
written out, against an independent validator of SAM text, against the frozen example and against mem_pair.sam_fields; the host
entry's argument checks, which return before a device is touched."""
import json
import os

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mem_pair as MP
from genomicsbench_amd import mem_sam as SM
import mem_sam_cases as K
import mem_sam_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def checked(j, w):
    """The validator on a call's text and records; -> the number of lines."""
    return R.validate(w["lines"].tobytes(), j["text"], j["contig_names"], j["contig_off"], w["recs"])


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_lines(name):
    j = K.hand_built()[name]
    w = K.reference(j)
    assert w["lines"].tobytes().decode("latin-1") == "".join(K.expected()[name])
    assert checked(j, w) == w["n_recs"] == int(w["rec_off"][-1])
    # md and the records tile their buffers as the lines do
    assert int(w["recs"]["md_len"].sum()) == w["n_md"] and int(w["recs"]["line_len"].sum()) == w["n_text"]
    for rec in w["recs"]:
        md = w["md"][int(rec["md_off"]):int(rec["md_off"]) + int(rec["md_len"])].tobytes()
        line = w["lines"][int(rec["line_off"]):int(rec["line_off"]) + int(rec["line_len"])].tobytes()
        assert (b"\tMD:Z:" + md + b"\t" in line) == (rec["n_cigar"] > 0) and (md != b"") == (rec["n_cigar"] > 0)


def test_the_cases_cover_what_they_name():
    """The shapes the cases are there for occur in their lines."""
    E = {k: "".join(v) for k, v in K.expected().items()}
    md = lambda name, read: [l.split("MD:Z:")[1].split("\t")[0] for l in E[name].split("\n") if l.startswith(read + "\t")][0]
    assert md("m_runs", "m1_all") == "0" + md("m_runs", "m1_all")[1] + "0" and md("m_runs", "m1_none") == "1"
    assert md("m_runs", "m129_none") == "129" and md("m_runs", "m65_at63").startswith("63") and md("m_runs", "m65_at64").startswith("64")
    assert md("m_runs", "m129_all").count("0") >= 130 and len(md("m_runs", "m129_all")) == 2 * 129 + 1
    a = md("m_runs", "m65_adjacent")
    assert a.startswith("63") and a[3] == "0" and a.endswith("0") and len(a) == 6
    c = md("counts_pos", "count_8")
    assert [int(x) for x in __import__("re").findall(r"\d+", c)] == [9, 10, 99, 100, 28]
    assert [l.split("\t")[3] for l in E["counts_pos"].split("\n")[:-1]] == ["9", "10", "99", "100"]
    assert [l.split("\t")[3] for l in E["big_pos"].split("\n")[:-1]] == ["999999999", "1000000000"]
    tl = [int(l.split("\t")[8]) for l in E["tlen"].split("\n")[:-1]]
    assert min(tl) < 0 < max(tl) and 0 in tl
    assert {l.split("\t")[4] for l in E["tlen"].split("\n")[:-1]} == {"0", "60"}
    assert "0^" in E["indels"] and "^GGT0" in E["indels"] and "\t25M2D5S\t" in E["indels"] and "N" in md("n_bases", "n_text_del")
    sup = [l.split("\t") for l in E["three_records"].split("\n")[:-1] if int(l.split("\t")[1]) & 0x800]
    assert len(sup) == 3 and all("H" in f[5] and "S" not in f[5] for f in sup)
    assert all("S" in l.split("\t")[5] for l in E["three_records_Y"].split("\n")[:-1])
    assert E["three_records"].split("\n")[0].split("SA:Z:")[1].count(";") == 2
    assert "\tMC:Z:5H70M5H\t" in E["three_records"] and "\tMC:Z:5S70M5S\t" in E["three_records"]
    assert len(E["long"].split("\n")[0].split("\t")[9]) == 1024 and E["long"].split("\n")[1].startswith("y" * 300 + "\t")
    assert all(l.split("\t")[10] == "*" for l in E["long_no_qual"].split("\n")[:-1])


def test_big_pos():
    j = K.big_pos()
    w = K.reference(j)
    assert w["lines"].tobytes().decode("latin-1") == K.expected()["big_pos"]
    assert checked(j, w) == 2


@pytest.mark.parametrize("name", ["tlen", "three_records", "three_records_Y", "unmapped", "long"])
def test_rows_equal_sam_fields(name):
    """On the nine fields they share, the records are mem_pair.sam_fields' rows."""
    j = K.hand_built()[name]
    w = K.reference(j)
    want = MP.sam_fields(j["pairs"], j["regs"].view(MP.REG_DTYPE), j["alns"], j["cigar"])
    assert w["rows"] == want
    got = [(int(x["read"]), int(x["flag"]), int(x["rid"]), int(x["pos"]), int(x["mapq"]), int(x["mrid"]), int(x["mpos"]), int(x["tlen"]))
           for x in w["recs"]]
    assert got == [r[:5] + r[6:] for r in want]


def example_job():
    with open(os.path.join(HERE, "golden", "mem_sam_example.json")) as f:
        e = json.load(f)["example"]
    code = lambda s: np.array(["ACGTN".index(c) for c in s], dtype=np.uint8)
    g = code(e["genome"])
    pairs = np.zeros(len(e["proper"]), dtype=K.PAIR_DTYPE)
    pairs["proper"] = e["proper"]
    j = dict(mode=e["mode"], softclip=e["softclip"], regs=np.array([tuple(x) for x in e["regs"]], dtype=K.REG_DTYPE),
             reg_off=np.array(e["reg_off"], np.int64), pairs=pairs, alns=np.array([tuple(x) for x in e["alns"]], dtype=K.ALN_DTYPE),
             cigar=np.array(e["cigar"], np.uint32), qer=code(e["qer"]), read_off=np.array(e["read_off"], np.int64),
             read_len=np.array(e["read_len"], np.int32), qual=np.frombuffer(e["qual"].encode("latin-1"), np.uint8), names=e["names"],
             contig_names=e["contig_names"], text=K.text_of(g), L=len(g), contig_off=np.array(e["contig_off"], np.int64))
    want = dict(recs=np.array([tuple(x) for x in e["recs"]], dtype=R.SAM_DTYPE), rec_off=np.array(e["rec_off"], np.int64), n_recs=len(e["recs"]),
                md=np.frombuffer(e["md"].encode(), np.uint8), n_md=len(e["md"]), lines=np.frombuffer(e["lines"].encode("latin-1"), np.uint8),
                n_text=len(e["lines"]))
    return j, want


def test_frozen_example():
    j, want = example_job()
    K.same(K.reference(j), want)
    assert checked(j, want) == 5


def test_capacities_cut_as_the_device_does():
    j = K.hand_built()["indels"]
    full = K.reference(j)
    w = K.reference(j, rec_cap=2, md_cap=7, text_cap=100)
    assert (w["n_recs"], w["n_md"], w["n_text"]) == (full["n_recs"], full["n_md"], full["n_text"])
    assert w["recs"].tobytes() == full["recs"][:2].tobytes() and w["md"].tobytes() == full["md"][:7].tobytes()
    assert w["lines"].tobytes() == full["lines"][:100].tobytes()


def test_validator_refuses_wrong_lines():
    """The validator is no echo: a wrong MD base, NM, SEQ length or position fails it."""
    j = K.hand_built()["indels"]
    good = K.reference(j)["lines"].tobytes()
    R.validate(good, j["text"], j["contig_names"], j["contig_off"])
    for old, new in ((b"MD:Z:5A14^GC37", b"MD:Z:5C14^GC37"), (b"NM:i:6", b"NM:i:5"), (b"\t20M2D10M3I27M\t", b"\t20M2D10M3I28M\t"),
                     (b"chr1\t901\t", b"chr1\t902\t"), (b"MD:Z:19T0^GGT0G19", b"MD:Z:19T0^GGA0G19")):
        assert old in good
        with pytest.raises(AssertionError):
            R.validate(good.replace(old, new), j["text"], j["contig_names"], j["contig_off"])


def test_header():
    assert SM.header(["chr1", b"contig_two"], K.CO, 4000) == "@SQ\tSN:chr1\tLN:1500\n@SQ\tSN:contig_two\tLN:2500\n"


def host_rc(j, **kw):
    j = dict(j, **{k: v for k, v in kw.items() if k in j})
    caps = {k: v for k, v in kw.items() if k not in j}
    try:
        SM.sam_host(SM.make_params(softclip=j["softclip"]), j["mode"], j["regs"], j["reg_off"], j["pairs"], j["alns"], j["cigar"], j["qer"],
                    j["read_off"], j["read_len"], j["qual"], j["names"], j["contig_names"], j["text"], j["L"], j["contig_off"], **caps)
    except N.GbxError as e:
        return e.code, str(e)
    return 0, ""


def test_host_entry_checks_its_arguments_before_a_device_is_touched():
    """GBX_ERR_ARG naming the lowest offender, not GBX_ERR_NO_DEVICE: these returns come before the first HIP call."""
    j = K.hand_built()["three_records"]               # 2 reads, 7 regions (2 of them unreported), 5 alignments

    def bad(what, **kw):
        rc, msg = host_rc(j, **kw)
        assert rc == N.GBX_ERR_ARG and what in msg, (kw.keys(), rc, msg)
    bad("softclip", softclip=2)
    bad("mode", mode=2)
    off = j["reg_off"].copy()
    off[1] = off[2] + 1
    bad("not monotone at read 1", reg_off=off)
    bad("contig_off", contig_off=np.array([0, 1500, 3999], np.int64))
    bad("text_bytes", text=j["text"][:-1])
    g = j["regs"].copy()
    g["sel"][[2, 5]] = 5
    bad("region 2: sel = 5", regs=g)
    a = j["alns"].copy()
    a["rid"][[0, 1]] = [-1, 2]                         # alns are in reverse order: region 3 has alns[0], region 2 alns[1]
    bad("region 2: its alignment's rid = 2", alns=a)
    a = j["alns"].copy()
    a["cigar_off"][2] = len(j["cigar"]) - 1
    bad("region 1: its CIGAR words", alns=a)
    c = j["cigar"].copy()
    c[int(j["alns"]["cigar_off"][2])] = 10 << 4 | 5
    bad("region 1: CIGAR op 5", cigar=c)
    c = j["cigar"].copy()
    c[int(j["alns"]["cigar_off"][2])] += 1 << 4
    bad("region 1: its CIGAR covers 101 read bases of 100", cigar=c)
    a = j["alns"].copy()
    a["pos"][2] = 1500 - 54
    bad("region 1: its CIGAR covers", alns=a)
    rl = j["read_len"].copy()
    rl[1] = 0
    bad("read 1:", read_len=rl)
    ro = j["read_off"].copy()
    ro[:] = len(j["qer"]) - 10
    bad("read 0:", read_off=ro)


def test_text_cap_is_safe_for_the_cases():
    for name, j in sorted(K.hand_built().items()):
        w = K.reference(j)
        per_read = max(np.diff(w["rec_off"]))
        cap = SM.text_cap(w["n_recs"], len(j["cigar"]), len(j["qer"]), sum(len(n) for n in j["names"]), max(len(n) for n in j["contig_names"]),
                          max_recs=per_read, max_del=3)
        assert w["n_text"] <= cap and w["n_md"] <= cap, name
