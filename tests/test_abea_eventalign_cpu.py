"""abea eventalign, CPU: the restatement (tests/abea_eventalign_ref.c) against the reference's own results.

tests/golden/abea_eventalign.npz: 23 hand-made reads of 96 to 350 bases (abea_eventalign_ref.golden_specs), forward and reverse:
a read that is one segment; reads whose first segment emits 49, 50 and 51 states before the cut; outlier events (B on the path);
deleted bases and k-mers without events (K on the path); an insertion of 80 bases (a long-row segment); a deletion of 130
reference bases (the read ends there); clips; lower case and IUPAC codes; a region trim; a read that ends by |start - stop| < 2.
The file holds the inputs and what the reference's eventalign.c returned for them (realign_read, summarize_alignment and
emit_event_alignment_tsv with both print_read_names and both scale_events values), compiled unmodified as C++ with its asserts
on against empty stand-ins for the htslib / HDF5 headers (a stub bam1_t with core.pos, the flag and a CIGAR)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abea_eventalign_ref as R  # noqa: E402
import abea_meth_ref as MR  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abea_eventalign.npz")
CALIB = ("scale", "shift", "var", "log_var", "events_per_base", "map", "flags")
CG = ("cigar_off", "cigar", "pos", "rc", "ref_off", "ref_len", "ref_arena")


def golden():
    g = np.load(GOLDEN)
    calib, cg = {k: g["calib_" + k] for k in CALIB}, {k: g["cg_" + k] for k in CG}
    return g, calib, cg


def golden_groups(g):
    """the reads of the golden by the region they ran with: [(region, read indices)]"""
    regions = sorted({(int(a), int(b)) for a, b in g["region"]})
    return [(rg, np.flatnonzero((g["region"] == rg).all(axis=1))) for rg in regions]


def subset(g, calib, cg, idx):
    """the reads idx as a batch of their own (the arenas stay whole)"""
    c = {k: (calib[k] if k == "map" else calib[k][idx]) for k in CALIB}
    off = np.zeros(len(idx) + 1, np.int64)
    cig = []
    for j, r in enumerate(idx):
        cig.append(cg["cigar"][cg["cigar_off"][r]:cg["cigar_off"][r + 1]])
        off[j + 1] = off[j] + len(cig[-1])
    s = dict(cigar_off=off, cigar=np.concatenate(cig), pos=cg["pos"][idx], rc=cg["rc"][idx], ref_off=cg["ref_off"][idx], ref_len=cg["ref_len"][idx],
             ref_arena=cg["ref_arena"])
    ev, eoff = [], np.zeros(len(idx) + 1, np.int64)
    for j, r in enumerate(idx):
        ev.append(g["events"][g["event_off"][r]:g["event_off"][r + 1]])
        eoff[j + 1] = eoff[j] + len(ev[-1])
    return g["seq_off"][idx], g["seq_len"][idx], eoff, np.concatenate(ev), c, s


def assert_records_equal_golden(g, idx, o, eoff):
    goff = np.concatenate([[0], np.cumsum(g["n_rec"])])
    for j, r in enumerate(idx):
        want = g["rec"][goff[r]:goff[r + 1]]
        got = R.read_records(o, eoff, j)
        assert o["status"][j] == 0 and np.array_equal(got, want), str(g["names"][r])


def test_restatement_equals_golden_records():
    g, calib, cg = golden()
    seen = 0
    for region, idx in golden_groups(g):
        so, sl, eoff, ev, c, s = subset(g, calib, cg, idx)
        o = R.run(so, sl, eoff, ev["mean"], g["model"], c, s, region)
        assert_records_equal_golden(g, idx, o, eoff)
        seen += len(idx)
    assert seen == len(g["n_rec"]) == 23


def test_golden_holds_what_it_says():
    g, _, _ = golden()
    names = [str(n) for n in g["names"]]
    goff = np.concatenate([[0], np.cumsum(g["n_rec"])])
    rec = lambda nm: g["rec"][goff[names.index(nm)]:goff[names.index(nm) + 1]]
    nev = np.diff(g["event_off"])
    assert set(g["cg_rc"].tolist()) == {0, 1} and set((g["cg_cigar"] & 0xf).tolist()) >= {0, 1, 2, 4, 5, 7, 8}
    for rc in (0, 1):
        assert (rec("outlier event, rc %d" % rc)["state"] == ord("B")).sum() >= 2
        jumps = np.abs(np.diff(rec("deleted bases, rc %d" % rc)["ref_pos"]))
        assert (jumps > 1).any()                                            # a k-mer is skipped: K on the path
        k = names.index("deletion of 130, rc %d" % rc)
        assert 0 < g["n_rec"][k] < nev[k] // 2                              # the read ends at the deletion
    k = names.index("ends one event short, rc 0")
    assert g["n_rec"][k] == nev[k] - 2                                      # the first event is never emitted, the last one is left
    k = names.index("region trim, rc 0")
    assert rec("region trim, rc 0")["ref_pos"].min() >= g["region"][k][0] and rec("region trim, rc 0")["ref_pos"].max() <= g["region"][k][1]
    ref = g["cg_ref_arena"]
    assert ((ref >= ord("a")) & (ref <= ord("z"))).any() and np.isin(ref, np.frombuffer(b"NRYKSBMnry", np.uint8)).any()


def test_restatement_equals_golden_summary_and_tsv():
    g, calib, cg = golden()
    goff = np.concatenate([[0], np.cumsum(g["n_rec"])])
    o = dict(rec=np.zeros(int(g["event_off"][-1]), R.REC_DTYPE), n_rec=g["n_rec"])
    for r in range(len(g["n_rec"])):
        o["rec"][g["event_off"][r]:g["event_off"][r] + g["n_rec"][r]] = g["rec"][goff[r]:goff[r + 1]]
    got = R.summary(g["event_off"], g["events"], g["model"], calib["scale"], calib["shift"], calib["var"], cg, o)
    for f in got.dtype.names:
        a, b = got[f], g["summary"][f]
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), f
    tsv = g["tsv"].tobytes()
    for r in range(len(g["n_rec"])):
        ev = g["events"][g["event_off"][r]:g["event_off"][r + 1]]
        ref = cg["ref_arena"][cg["ref_off"][r]:cg["ref_off"][r] + cg["ref_len"][r]]
        for v in range(4):
            want = tsv[g["tsv_off"][4 * r + v]:g["tsv_off"][4 * r + v + 1]]
            got_t = R.tsv(ev, g["model"], calib["scale"][r], calib["shift"][r], calib["var"][r], cg["rc"][r], cg["pos"][r], ref, g["rec"][goff[r]:goff[r + 1]],
                          header=r == 0, print_read_names=bool(v & 1), scale_events=bool(v & 2), read_index=7 + r, read_name=b"read", ref_name=b"chr1")
            assert got_t == want, (str(g["names"][r]), v)
    assert b"inf" in tsv or b"nan" in tsv                                   # a B record divides by a zero stdv


def test_kmers_of_the_golden_records():
    """ref_kmer and model_kmer as the reference stored them, from the 12 bytes of a record (the TSV test reads them as text)"""
    g, _, cg = golden()
    goff = np.concatenate([[0], np.cumsum(g["n_rec"])])
    km = g["kmers"].reshape(-1, 14)
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    for r in range(len(g["n_rec"])):
        ref = MR.disambiguate(bytes(cg["ref_arena"][cg["ref_off"][r]:cg["ref_off"][r] + cg["ref_len"][r]]))
        for q, k in zip(g["rec"][goff[r]:goff[r + 1]], km[goff[r]:goff[r + 1]]):
            s = q["ref_pos"] - cg["pos"][r]
            rk = ref[s:s + 6]
            mk = b"NNNNNN" if q["state"] == ord("B") else rk if not cg["rc"][r] else bytes(comp[c] for c in rk[::-1])
            assert bytes(k[:6]) == rk and bytes(k[7:13]) == mk


def test_from_rule():
    ninf = -np.inf
    assert R.pick([ninf] * 6)[0] == 5                                      # six -inf: HMT_FROM_SOFT
    assert R.pick([1.0, 1.0, 0.5, 1.0, 0.0, ninf]) == (3, np.float32(1.0))  # ties go to the higher index
    assert R.pick([2.0, 1.0, 2.0, ninf, ninf, ninf])[0] == 2
    assert R.pick([ninf, -3.0, ninf, -3.0, -4.0, ninf])[0] == 3
    assert R.pick([0.25, ninf, ninf, ninf, ninf, ninf])[0] == 0
    assert R.pick([ninf, ninf, ninf, ninf, ninf, -0.5])[0] == 5
    assert R.pick([0.0, -0.0, ninf, ninf, ninf, ninf])[0] == 1            # 0.0 == -0.0


@pytest.mark.parametrize("epb", [1.05, 1.2, 2.0, 2.7182818, 4.9, 7.5])
def test_transitions_equal_the_methylation_stage(epb):
    assert np.array_equal(R.transitions(epb).view(np.uint32), MR.transitions(epb).view(np.uint32))


def test_status_rules_of_the_restatement():
    """rows_cap and the reads that get nothing, on the edge batch of the GPU tests"""
    b = R.edge_batch()
    o = R.run(b["seq_off"], b["seq_len"], b["event_off"], b["events"]["mean"], b["model"], b["calib"], b["cg"], rows_cap=R.EDGE_ROWS_CAP)
    at = {nm: i for i, nm in enumerate(b["names"])}
    over = [at["rows %d, rc %d" % (R.EDGE_ROWS_CAP + 1, rc)] for rc in (0, 1)]
    assert (o["status"][over] == 1).all() and (o["n_rec"][over] == 0).all() and (np.delete(o["status"], over) == 0).all()
    for rc in (0, 1):
        assert o["n_rec"][at["rows %d, rc %d" % (R.EDGE_ROWS_CAP, rc)]] == R.EDGE_ROWS_CAP - 1
        assert o["counts"][at["12 bases, 12 rows, rc %d" % rc]].tolist()[:2] == [1, 3 * 12 * 7]
        assert o["counts"][at["101 bases then 40, rc %d" % rc]][0] == 2 and o["counts"][at["several segments, rc %d" % rc]][0] >= 8
    assert o["n_rec"][at["flagged"]] == 0 and o["n_rec"][at["no events"]] == 0
    with pytest.raises(ValueError):
        cg = dict(b["cg"]); cg["cigar"] = cg["cigar"].copy(); cg["cigar"][3] = (5 << 4) | 3
        R.run(b["seq_off"], b["seq_len"], b["event_off"], b["events"]["mean"], b["model"], b["calib"], cg)
