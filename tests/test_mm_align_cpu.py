"""CPU-side checks for the base-level alignment stage: the device's rules compiled for the host (mm_align_rules.h in
libgbx_mm_cpu.so) against the restatement (tests/mm_align_ref.py, its C twin for the larger jobs) on every case of
tests/mm_align_cases.py, the C twin against the Python restatement on the small ones, properties that rest on no one's memory of
minimap2 (the CIGAR consumes the reported spans, re-scores to the job score, a wide-band global score equals a general-gap DP), the
parameter and host-entry refusals (all before a device is touched), the PAF-with-CIGAR text, the frozen example, the mmpaf driver's
command line, and the host build of the rules under ASan + UBSan in a program of its own (tests/sanitize_mm_align)."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mm_align as MA
from genomicsbench_amd import mm_map as MM
import mm_align_cases as AK
import mm_align_ref as AR
import mm_cases as K
from mm_align_cases import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MMPAF = os.path.join(ROOT, "genomicsbench_amd", "bin", "mmpaf")
SAN = os.path.join(ROOT, "tests", "sanitize_mm_align")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mm_align_example.json")


def twin(b, **kw):
    return MA.align_cpu(MA.make_params(**b.P), *b.arrays(), **kw)


def test_exports_and_sizes():
    L = MA.lib()
    for name in ("align_default_params", "align_check_params", "align_workspace_bytes", "align_device", "align_host", "paf_cigar_workspace_bytes",
                 "paf_cigar_device", "paf_cigar_host"):
        assert hasattr(L, "gbx_mm_" + name), name
    T = MA._twin()
    assert hasattr(T, "gbx_mm_align_cpu") and hasattr(T, "gbx_mm_paf_cigar_cpu") and hasattr(T, "gbx_mm_map_cpu")
    assert C.sizeof(MA.MmAlignParams) == 48 and MA.ALN_DTYPE.itemsize == 56
    p = MA.make_params()
    assert {k: getattr(p, k) for k in AR.DEFAULTS} == AR.DEFAULTS
    MA.check_params(p)


@pytest.mark.parametrize("kw,word", [(dict(a=0), "a ="), (dict(b=-1), "b ="), (dict(sc_ambi=-1), "sc_ambi"), (dict(q=-1), "q ="), (dict(q2=-2), "q2"),
                                     (dict(e=0), "e ="), (dict(e2=0), "e2"), (dict(bw=0), "bw"), (dict(min_ksw_len=0), "min_ksw_len"),
                                     (dict(max_ext=-1), "max_ext"), (dict(end_bonus=-1), "end_bonus"), (dict(b=256), "b = 256")])
def test_check_params_refuses(kw, word):
    with pytest.raises(N.GbxError) as e:
        MA.check_params(MA.make_params(**kw))
    assert e.value.code == N.GBX_ERR_ARG and word in str(e.value)


# ------------------------------------------------------------------------------------------------ single jobs
def _job_cases():
    rng = random.Random(4321)
    out = []
    for _ in range(400):
        n = rng.randrange(1, 40)
        t = K.rand_seq(rng, n, "ACGTN" if rng.random() < 0.1 else "ACGT")
        q = bytearray(K.mutate(rng, t, 0.1))
        if rng.random() < 0.5 and len(q) > 4:                         # a planted indel of up to 25 bases
            o, ln = rng.randrange(len(q)), rng.randrange(1, 26)
            if rng.random() < 0.5:
                q[o:o] = K.rand_seq(rng, ln)
            else:
                del q[o:o + ln]
        if not q:
            q = bytearray(b"A")
        out.append((t, bytes(q), rng.choice([1, 2, 3, 5, 8, 20, 100]), rng.randrange(2), rng.randrange(2), rng.choice([0, 5, 20])))
    return out


def test_single_jobs_python_c_and_host_build_agree_and_hold_their_properties():
    """400 random pairs with planted indels, both tie modes, global and extension, bands 1..100: the Python restatement, its C twin
    and the host build of the device's rules give the same score, end cell, flags and runs; the runs consume the reported spans
    and re-score, with gap(l) a run, to the job's score."""
    n_ext_end = n_zdrop = n_empty = 0
    for t, q, w, mode, ext, bonus in _job_cases():
        P = AR.params(zdrop=30, end_bonus=bonus)                       # with no bonus the query end never beats the maximum
        p = MA.make_params(**P)
        T, Q = AR.codes(t), AR.codes(q)
        if not ext:
            w = max(w, abs(len(T) - len(Q)) + 1)
        py = AR.dp_job(P, T, Q, w, mode, ext)
        assert AR.dp_job_c(P, T, Q, w, mode, ext) == py, (t, q, w, mode, ext)
        hb = MA.job_cpu(p, t, q, w, mode, ext)
        assert (hb["score"], hb["ct"], hb["cq"], hb["flags"]) == (py["score"], py["ct"], py["cq"], py["zdropped"] | 2 * py["reach_end"]), (t, q, w, mode, ext)
        assert [(int(x) & 15, int(x) >> 4) for x in hb["cigar"]] == py["ops"], (t, q, w, mode, ext)
        s, ct, cq = AR.rescore(P, T, Q, py["ops"])
        assert (ct, cq) == (py["ct"], py["cq"]) and s == py["score"], (t, q, w, mode, ext)
        if not ext:
            assert (ct, cq) == (len(T), len(Q))
        n_ext_end += py["reach_end"]
        n_zdrop += py["zdropped"]
        n_empty += ext and py["end"] is None
    assert n_ext_end > 10 and n_zdrop > 3 and n_empty > 0


def test_wide_band_global_score_equals_a_general_gap_cost_dp():
    P = AR.params()
    rng = random.Random(99)
    for _ in range(60):
        t = K.rand_seq(rng, rng.randrange(1, 45))
        q = bytearray(K.mutate(rng, t, 0.08))
        if len(q) > 30 and rng.random() < 0.6:
            o = rng.randrange(len(q) - 26)
            del q[o:o + rng.randrange(18, 26)]                        # long enough for the second piece
        q = bytes(q) or b"C"
        T, Q = AR.codes(t), AR.codes(q)
        for mode in (AR.LEFT, AR.RIGHT):
            assert AR.dp_job(P, T, Q, len(T) + len(Q), mode, False)["score"] == AR.general_gap_global(P, T, Q)


@pytest.mark.parametrize("kind", ["fill", "right", "left"])
@pytest.mark.parametrize("bw", AK.BANDS)
def test_single_job_regions(bw, kind):
    """The size pairs at every band through the region entry: the small ones against the Python restatement, all against its C twin"""
    small = AK.single_job_batch(bw, kind, True)
    if small.regs:
        want = small.expected()
        assert small.expected(dp=AR.dp_job_c) == want
        same(twin(small), want)
    big = AK.single_job_batch(bw, kind, False)
    assert len(small.regs) + len(big.regs) == len(AK.size_pairs())
    same(twin(big), big.expected(dp=AR.dp_job_c))


# ------------------------------------------------------------------------------------------------ rules
def test_tie_rules_leftmost_gap():
    b, want = AK.tie_batch()
    same(twin(b), want)


def test_gap_pieces():
    b, want = AK.gap_batch()
    same(twin(b), want)


def test_ambiguous_bases():
    b, want = AK.ambi_batch()
    same(twin(b), want)


def test_zdrop_and_extension_ends():
    for name, b, want in AK.zdrop_batches():
        same(twin(b), want)


@pytest.mark.parametrize("min_ksw_len,max_ext", [(8, 5000), (200, 5000), (8, 0), (200, 10), (8, 10)])
def test_composed_regions(min_ksw_len, max_ext):
    b, want = AK.region_batch(min_ksw_len, max_ext)
    same(twin(b), want)


def test_wide_jobs():
    for b, want in AK.wide_batches():
        assert all(a["flags"] & 1 for a in want["alns"])
        same(twin(b), want)


@pytest.mark.parametrize("min_ksw_len,max_ext,bw", [(8, 5000, 500), (200, 5000, 500), (200, 0, 500), (8, 10, 20)])
def test_seeded_regions(min_ksw_len, max_ext, bw):
    b = AK.seeded_batch(min_ksw_len, max_ext, bw)
    want = b.expected(dp=AR.dp_job_c)
    assert sum(a["flags"] & 1 for a in want["alns"]) >= 10
    same(twin(b), want)


def test_seeded_regions_python_restatement():
    """the Python restatement itself on the seeded reads, at a band it can do in a few seconds"""
    b = AK.seeded_batch(8, 10, 20)
    b2 = AK.Batch(**b.P)
    keep = 3
    b2.refs, b2.reads, b2.off, b2.reg_off, b2.n_chained = b.refs, b.reads[:keep], b.off[:keep + 1], b.reg_off[:keep + 1], b.n_chained[:keep]
    b2.regs, b2.cax, b2.cay = b.regs[:b.reg_off[keep]], b.cax[:b.off[keep]], b.cay[:b.off[keep]]
    want = b2.expected()
    assert want == b2.expected(dp=AR.dp_job_c) and len(want["alns"]) >= 2
    same(twin(b2), want)


def test_z_room_flags_regions_in_order():
    """z_bytes between the needs of two regions: the ones whose jobs end past it get flag 32 and copy their region, the counts
    report the whole need"""
    b, full = AK.region_batch(8, 5000)
    need = full["counts"][2]
    for z in (0, need // 3, need - 16, need):
        want = b.expected(z_bytes=z)
        n32 = sum(a["flags"] == 32 for a in want["alns"])
        assert (n32 == 0) == (z == need) and want["counts"][2] == need
        same(twin(b, z_bytes=z), want)
    assert sum(a["flags"] == 32 for a in b.expected(z_bytes=need // 3)["alns"]) not in (0, 6)


def test_cigar_cap_short_reports_the_need():
    b, want = AK.gap_batch()
    got = twin(b, cigar_cap=5)
    assert got["counts"] == tuple(want["counts"]) and got["cigar"].tolist() == want["cigar"][:5]


# ------------------------------------------------------------------------------------------------ text
def test_paf_with_cigar_text():
    g, ro, alns, cig, qn, so, rep, tn, to, text = AK.paf_case()
    got, line_off = MA.paf_cigar_cpu(g, ro, alns, cig, qn, so, rep, tn, to)
    assert got.decode() == text
    lines = text.splitlines()
    assert sum("cg:Z:" in ln for ln in lines) == 6 and sum("cg:Z:" not in ln for ln in lines) == 7
    assert line_off[-1] == len(text) and all(text[:o].count("\n") == int(ro[r]) for r, o in enumerate(line_off))
    one = [ln for ln in lines if "cg:Z:" in ln][0].split("\t")
    assert one[12].startswith("NM:i:") and one[13].startswith("ms:i:") and one[14].startswith("AS:i:") and one[15].startswith("nn:i:") and one[16] == "tp:A:P"


def test_paf_cigar_text_without_alignments_is_the_plain_text():
    """one line rule behind both entries of the host build: gbx_mm_paf_cigar_cpu on records with their flags cleared gives what
    gbx_mm_paf_cpu gives, which is the restatement's plain text"""
    from genomicsbench_amd import mm_stage as ST
    g, ro, alns, cig, qn, so, rep, tn, to, _ = AK.paf_case()
    cleared = alns.copy()
    cleared["flags"] = 0
    got, line_off = MA.paf_cigar_cpu(g, ro, cleared, cig, qn, so, rep, tn, to)
    plain, plain_off = ST.paf_text(ST.twin().gbx_mm_paf_cpu, g, ro, qn, so, rep, tn, to, host=False)
    want = AR.paf_cigar([{k: int(r[k]) for k in AK.REG_KEYS} for r in g], ro, cleared, cig, qn, np.diff(so), tn, np.diff(to), rep)      # rule 9: not aligned
    assert got == plain and plain.decode() == want and np.array_equal(line_off, plain_off) and want.count("\n") == len(g)


def test_golden_example():
    """The frozen worked example: a forward and a reverse region, each with a left extension, two fills and a right extension; one
    fill holds a 25-base deletion, which the second gap piece pays for (24 + 25 = 49 against 4 + 50)."""
    ex = json.load(open(GOLDEN))
    b = AK.Batch(**ex["params"])
    for r in ex["reads"]:
        rid = b.ref(r["ref"].encode())
        b.read(r["read"].encode())
        b.region(rid, r["rev"], [tuple(a) for a in r["anchors"]])
    b.close()
    want = b.expected()
    for a, e in zip(want["alns"], ex["expect"]):
        words = want["cigar"][a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]
        assert AR.cigar_text(words) == e["cigar"]
        assert {k: a[k] for k in e if k != "cigar"} == {k: e[k] for k in e if k != "cigar"}
        assert "25D" in e["cigar"] and a["flags"] & 1
    same(twin(b), want)


# ------------------------------------------------------------------------------------------------ refusals
def test_host_entries_refuse_before_a_device():
    L, p = MA.lib(), MA.make_params()
    err = lambda: L.gbx_last_error().decode()
    i64 = lambda *v: np.array(v, np.int64)
    regs, alns = np.zeros(4, MM.REG_DTYPE), np.zeros(4, MA.ALN_DTYPE)
    regs["read"][:3] = [0, 1, 1]
    ax, nc, seq, cig, cnt = np.zeros(8, np.uint64), np.array([3, 5], np.int32), np.zeros(300, np.uint8), np.zeros(16, np.uint32), np.zeros(3, np.int64)

    def go(n, reg_off, off=i64(0, 3, 8), seq_off=i64(0, 100, 200), tseq_off=i64(0, 50, 90), nc_=nc, cax=ax, cig_=cig, cigar_cap=16, z_bytes=0, p_=p, n_t=2):
        return L.gbx_mm_align_host(C.byref(p_), n, N.ptr(regs), N.ptr(reg_off), N.ptr(off), N.ptr(cax), N.ptr(ax), N.ptr(nc_), N.ptr(seq), N.ptr(seq_off), n_t,
                                   N.ptr(seq), N.ptr(tseq_off), N.ptr(alns), N.ptr(cig_), cigar_cap, z_bytes, N.ptr(cnt))
    ro = i64(0, 1, 3)
    assert go(2, None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, off=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, cax=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, cig_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, nc_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, i64(1, 1, 3)) == N.GBX_ERR_ARG and "reg_off[0]" in err()
    assert go(2, i64(0, 2, 1)) == N.GBX_ERR_ARG and "reg_off is not monotone at read 1" in err()
    assert go(2, ro, off=i64(0, 5, 3)) == N.GBX_ERR_ARG and "off is not monotone at read 1" in err()
    assert go(2, ro, seq_off=i64(0, 100, 50)) == N.GBX_ERR_ARG and "seq_off is not monotone at read 1" in err()
    assert go(2, ro, tseq_off=i64(0, 50, 40)) == N.GBX_ERR_ARG and "tseq_off is not monotone at target 1" in err()
    assert go(2, ro, seq_off=i64(0, 100, 100 + 2 ** 28)) == N.GBX_ERR_UNSUPPORTED and "read 1" in err()
    assert go(2, ro, tseq_off=i64(0, 2 ** 28, 2 ** 28 + 5)) == N.GBX_ERR_UNSUPPORTED and "target 0" in err()
    assert go(2, ro, cigar_cap=-1) == N.GBX_ERR_ARG and go(2, ro, z_bytes=-1) == N.GBX_ERR_ARG and go(2, ro, n_t=-1) == N.GBX_ERR_ARG
    assert go(2 ** 21 + 1, ro) == N.GBX_ERR_UNSUPPORTED and "reads" in err()
    assert go(2, ro, p_=MA.make_params(e2=0)) == N.GBX_ERR_ARG and "e2" in err()
    assert go(2, i64(0, 2, 3)) == N.GBX_ERR_ARG and "region 1 names read 1" in err()
    assert go(2, ro, nc_=np.array([3, 6], np.int32)) == N.GBX_ERR_ARG and "n_chained = 6 at read 1" in err()
    assert go(0, i64(0), off=i64(0), seq_off=i64(0)) == N.GBX_OK and cnt.tolist() == [0, 0, 0]
    assert go(2, i64(0, 0, 0)) == N.GBX_OK and cnt.tolist() == [0, 0, 0]              # no regions: nothing for a device to do
    # PAF with CIGAR
    lo, nt = np.zeros(4, np.int64), C.c_int64(0)
    names, noff = np.frombuffer(b"abcd", np.uint8).copy(), i64(0, 2, 4)
    rep = np.zeros(4, np.int32)

    def paf(n, reg_off, qoff=noff, toff=noff, tso=i64(0, 50, 90), lines=seq, text_cap=64, lo_=lo, cig_=cig, n_cigar=16):
        return L.gbx_mm_paf_cigar_host(n, N.ptr(regs), N.ptr(reg_off), N.ptr(alns), N.ptr(cig_), n_cigar, N.ptr(names), N.ptr(qoff), N.ptr(i64(0, 100, 200)),
                                       N.ptr(rep), 2, N.ptr(names), N.ptr(toff), N.ptr(tso), N.ptr(lines), text_cap, N.ptr(lo_), C.byref(nt))
    assert paf(2, None) == N.GBX_ERR_ARG and "null" in err()
    assert paf(2, ro, lines=None) == N.GBX_ERR_ARG and "null" in err()
    assert paf(2, ro, cig_=None) == N.GBX_ERR_ARG and "null" in err()
    assert paf(2, ro, n_cigar=-1) == N.GBX_ERR_ARG
    assert paf(2, i64(0, 2, 1)) == N.GBX_ERR_ARG and "reg_off is not monotone at read 1" in err()
    assert paf(2, ro, toff=i64(1, 2, 4)) == N.GBX_ERR_ARG and "tname_off[0]" in err()
    assert paf(2, i64(0, 2, 3)) == N.GBX_ERR_ARG and "region 1 names read 1" in err()
    assert paf(0, i64(0)) == N.GBX_OK and nt.value == 0


def test_device_entries_refuse_bad_arguments():
    L, p = MA.lib(), MA.make_params()
    none = [None] * 3
    assert L.gbx_mm_align_device(C.byref(p), 1, *none, 4, *([None] * 4), 10, None, None, 1, *([None] * 4), 10, None, None, 0, None, 0, None) == N.GBX_ERR_ARG
    assert L.gbx_mm_align_device(C.byref(p), 2 ** 21 + 1, *none, 0, *([None] * 4), 0, None, None, 0, *([None] * 4), 0, None, None, 0, None, 0, None) == N.GBX_ERR_UNSUPPORTED
    assert L.gbx_mm_align_device(C.byref(MA.make_params(bw=0)), 1, *none, 0, *([None] * 4), 0, None, None, 0, *([None] * 4), 0, None, None, 0, None, 0, None) == N.GBX_ERR_ARG
    assert "bw" in L.gbx_last_error().decode()
    assert L.gbx_mm_paf_cigar_device(1, *none, 4, None, None, 0, *([None] * 4), 1, *([None] * 4), 10, None, None, None, 0, None) == N.GBX_ERR_ARG
    assert L.gbx_mm_align_workspace_bytes(4, 100, 1000) >= 1200 * 88 and L.gbx_mm_align_workspace_bytes(4, -1, 0) == 0
    assert L.gbx_mm_paf_cigar_workspace_bytes(4, 100) >= 808


# ------------------------------------------------------------------------------------------------ sanitizers, driver
def test_rules_under_asan_ubsan(tmp_path):
    """The host build of the rules and of the PAF-with-CIGAR writer in a stand-alone program under ASan + UBSan
    (tests/sanitize_mm_align), every buffer exactly as large as the entry names, on the composed regions: clean, and the
    restatement's records, words and text."""
    r = subprocess.run(["make", "-C", SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    b, want = AK.region_batch(8, 5000)
    g, ro, off, cax, cay, nc, reads, refs = b.arrays()
    _, _, _, _, qn, so, rep, tn, to, text = AK.paf_case()
    from genomicsbench_amd import mm_seed as MS
    seq, seq_off = MS.pack_seqs(reads)
    tseq, tseq_off = MS.pack_seqs(refs)
    qnames, qoff = MM.pack_names(qn)
    tnames, toff = MM.pack_names(tn)
    src, out = tmp_path / "batch.bin", tmp_path / "out.bin"
    P = MA.make_params(**b.P)
    with open(src, "wb") as f:
        f.write(np.array([len(reads), len(g), len(cax), len(refs), len(seq), len(tseq), len(qnames), len(tnames), want["counts"][1], want["counts"][2]],
                         np.int64).tobytes())
        f.write(bytes(P))
        for a in (g, ro, off, cax, cay, nc, seq, seq_off, tseq, tseq_off, qnames, qoff, tnames, toff, np.ascontiguousarray(rep, np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([os.path.join(SAN, "_build", "align_main"), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    raw = open(out, "rb").read()
    cnt = np.frombuffer(raw, np.int64, 3)
    alns = np.frombuffer(raw, MA.ALN_DTYPE, len(g), 24)
    cig = np.frombuffer(raw, np.uint32, int(cnt[1]), 24 + 56 * len(g))
    same(dict(alns=alns, cigar=cig, counts=tuple(int(v) for v in cnt)), want)
    at = 24 + 56 * len(g) + 4 * int(cnt[1])
    assert int(np.frombuffer(raw, np.int64, 1, at)[0]) == len(text) and raw[at + 8:].decode() == text


def test_mmpaf_command_line(tmp_path):
    run = lambda *a: subprocess.run([MMPAF] + list(a), capture_output=True, text=True, timeout=60)
    r = run("--help")
    assert r.returncode == 0 and "[-c " in r.stdout and "--end-bonus" in r.stdout and "--min-ksw-len" in r.stdout and "--max-ext" in r.stdout
    for args, word in ((("-A", "2", "a", "b"), "-A needs -c"), (("-B", "4", "a", "b"), "-B needs -c"), (("-O", "4,24", "a", "b"), "-O needs -c"),
                       (("-E", "2,1", "a", "b"), "-E needs -c"), (("-z", "400", "a", "b"), "-z needs -c"), (("--end-bonus", "5", "a", "b"), "--end-bonus needs -c"),
                       (("--min-ksw-len", "100", "a", "b"), "--min-ksw-len needs -c"), (("--max-ext", "100", "a", "b"), "--max-ext needs -c"),
                       (("-c", "-A", "0", "a", "b"), "a = 0"), (("-c", "-O", "4", "a", "b"), "-O takes two integers"), (("-c", "-E", "2,0", "a", "b"), "e2 = 0"),
                       (("-c", "-O", "x,1", "a", "b"), "-O takes two integers"), (("-c", "-z"), "-z takes an integer"), (("-c", "-r", "0", "a", "b"), "bw"),
                       (("-c", "--min-ksw-len", "0", "a", "b"), "min_ksw_len"), (("-c", "--max-ext", "-1", "a", "b"), "max_ext")):
        r = run(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr)
    fa = tmp_path / "ref.fa"
    fa.write_text(">r\nACGT\n")
    r = run("-c", str(fa), str(tmp_path / "absent.fq"))
    assert r.returncode == 1 and "fail to open" in r.stderr
