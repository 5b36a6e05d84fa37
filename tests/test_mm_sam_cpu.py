"""CPU-side checks for the mm sam stage: the device's rules compiled for the host (mm_sam_rules.h in libgbx_mm_cpu.so) against the
restatement (tests/mm_sam_ref.py) on every case of tests/mm_sam_cases.py and every option set, with a team of one lane and with
teams of host threads that meet as a wavefront's lanes do; the validator on every SAM text, and refusing texts with one byte
altered; the frozen example; capacities behind guard bytes; seeded regions through align_cpu; the refusals; the mmpaf driver's
command line; and the host build under ASan + UBSan in a program of its own (tests/sanitize_mm_sam)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mm_align as MA
from genomicsbench_amd import mm_sam as MS
from genomicsbench_amd import mm_stage as ST
import mm_align_cases as AK
import mm_sam_cases as SK
import mm_sam_ref as SR
from mm_sam_cases import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MMPAF = os.path.join(ROOT, "genomicsbench_amd", "bin", "mmpaf")
SAN = os.path.join(ROOT, "tests", "sanitize_mm_sam")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mm_sam_example.json")
BATCHES = sorted(SK.all_batches())


def test_exports_and_sizes():
    L, T = MS.lib(), ST.twin()
    for name in ("gbx_mm_sam_default_params", "gbx_mm_sam_check_params", "gbx_mm_sam_workspace_bytes", "gbx_mm_sam_device", "gbx_mm_sam_host"):
        assert hasattr(L, name), name
    assert hasattr(T, "gbx_mm_sam_cpu") and hasattr(T, "gbx_mm_sam_cpu_lanes")
    assert C.sizeof(MS.MmSamParams) == 20
    p = MS.make_params()
    assert [getattr(p, k) for k, _ in MS.MmSamParams._fields_] == [0] * 5
    assert L.gbx_mm_sam_workspace_bytes(4, 100) >= 105 * 8 and L.gbx_mm_sam_workspace_bytes(-1, 0) == 0 and L.gbx_mm_sam_workspace_bytes(0, -1) == 0


@pytest.mark.parametrize("kw,word", [(dict(format=2), "format"), (dict(format=-1), "format"), (dict(cs=3), "cs"), (dict(cs=-1), "cs"), (dict(md=2), "md"),
                                     (dict(eqx=2), "eqx"), (dict(eqx=-1), "eqx"), (dict(softclip=2), "softclip")])
def test_check_params_refuses(kw, word):
    with pytest.raises(N.GbxError) as e:
        MS.check_params(MS.make_params(**kw))
    assert e.value.code == N.GBX_ERR_ARG and word in str(e.value)
    assert MS.lib().gbx_mm_sam_check_params(None) == N.GBX_ERR_ARG


@pytest.mark.parametrize("opts", sorted(SK.OPTION_SETS))
@pytest.mark.parametrize("batch", BATCHES)
def test_host_build_equals_the_restatement(batch, opts):
    b, o = SK.all_batches()[batch], SK.OPTION_SETS[opts]
    want = b.expected(**o)
    got = MS.sam_cpu(MS.make_params(**o), *b.arrays())
    same(got, want)
    if o.get("format") and batch != "malformed":
        reads, refs = b.named()
        n = SR.validate(got["text"].decode("latin-1"), reads, refs, got["line_off"])
        assert n == sum(SR.prints(a, len(b.cigar)) for a in b.alns)


@pytest.mark.parametrize("batch,opts,lanes", [("edges", "sam_all", 64), ("edges", "paf_all", 8), ("edges_noqual", "sam_all_long", 16), ("kinds", "sam_all", 64),
                                              ("kinds", "sam_Y", 7), ("letters", "sam_all_long", 64), ("malformed", "sam_all", 64), ("malformed", "paf_all", 5),
                                              ("edges", "sam_all_long", 3), ("kinds_noqual", "sam", 2)])
def test_a_team_of_lanes_writes_the_same_bytes(batch, opts, lanes):
    """the paths one lane never takes - steps of many columns, batches of many words, a ballot over a read's regions - on a team of
    host threads that meet at every ballot, scan and shuffle"""
    b, o = SK.all_batches()[batch], SK.OPTION_SETS[opts]
    same(MS.sam_cpu(MS.make_params(**o), *b.arrays(), lanes=lanes), b.expected(**o))


def test_cases_cover_what_they_claim():
    b = SK.edge_batch()
    sam = b.expected(format=1, cs=1, md=1, eqx=1)["text"].decode()
    for n in (9, 10, 99, 100, 1000):
        assert ":%d*" % n in sam and "%d=" % n in sam
    assert "130X" in sam and "200=" in sam and "cs:Z::200\t" in sam and "MD:Z:200\n" in sam and re.search(r"\+[acgt]{70}", sam) and re.search(r"\^[ACGT]{70}", sam)
    k = SK.kinds_batch().expected(format=1)["text"].decode().split("\n")
    flags = [int(ln.split("\t")[1]) for ln in k if ln]
    assert {0, 16 | 2048, 256, 4, 2048, 16} <= set(flags), flags
    assert sum("SA:Z:" in ln for ln in k) == 6 and any("\t*\t*\tNM" in ln for ln in k) and any(re.search(r"\t\d+H\d+M", ln) for ln in k)
    y = SK.kinds_batch().expected(format=1, softclip=1)["text"].decode()
    assert "H" not in "".join(ln.split("\t")[5] for ln in y.split("\n") if ln)
    lt = SK.letters_batch().expected(format=1, cs=1, md=1)["text"].decode()
    assert "*na" in lt and "*an" in lt or "*nc" in lt
    assert max(len(n) for n in SK.letters_batch().qnames) == 300 and min(len(n) for n in SK.letters_batch().qnames) == 1


def test_paf_with_every_option_off_is_the_paf_cigar_text():
    for b in (SK.edge_batch(), SK.kinds_batch(), SK.letters_batch()):
        g, ro, alns, cig, qn, reads, quals, rep, tn, refs = b.arrays()
        so, to = np.cumsum([0] + [len(r) for r in reads]), np.cumsum([0] + [len(r) for r in refs])
        want, want_off = MA.paf_cigar_cpu(g, ro, alns, cig, qn, so, rep, tn, to)
        got = MS.sam_cpu(MS.make_params(), *b.arrays())
        assert got["text"] == want and np.array_equal(got["line_off"], want_off) and got["counts"] == (len(g), 0)
    g, ro, alns, cig, qn, so, rep, tn, to, text = AK.paf_case()                # the composed regions of the align stage, aligned or not
    b, _ = AK.region_batch(8, 5000)
    got = MS.sam_cpu(MS.make_params(), g, ro, alns, cig, qn, b.reads, None, rep, tn, b.refs)
    assert got["text"].decode() == text


def _alter(text, tag, how):
    """one byte of the first `tag` field that `how` finds altered"""
    lines = text.split("\n")
    for i, ln in enumerate(lines):
        f = ln.split("\t")
        for j, x in enumerate(f):
            if (x.startswith(tag) if tag else j == 5) and how(x) is not None:
                f[j] = how(x)
                lines[i] = "\t".join(f)
                return "\n".join(lines)
    raise AssertionError("nothing to alter")


def test_validator_refuses_altered_texts():
    b = SK.edge_batch()
    reads, refs = b.named()
    text = b.expected(format=1, cs=1, md=1, eqx=1)["text"].decode()
    assert SR.validate(text, reads, refs) == len(b.alns)

    def digit(x):
        m = re.search(r"[1-8]", x[5:])
        return None if not m else x[:5 + m.start()] + str(int(m.group()) + 1) + x[5 + m.start() + 1:]

    def base(x):
        m = re.search(r"[ACGT]", x[5:])
        return None if not m else x[:5 + m.start()] + "ACGT"[("ACGT".index(m.group()) + 1) % 4] + x[5 + m.start() + 1:]

    def sub(x):
        m = re.search(r"\*[acgt]", x)
        return None if not m else x[:m.start() + 1] + "acgt"[("acgt".index(x[m.start() + 1]) + 1) % 4] + x[m.start() + 2:]

    def eqx(x):
        m = re.search(r"\d=\d+X", x)
        return None if not m else x[:m.start() + 1] + "X" + x[m.start() + 2:]
    for tag, how in (("MD:Z:", digit), ("MD:Z:", base), ("cs:Z:", digit), ("cs:Z:", sub), (None, eqx), ("NM:i:", digit)):
        with pytest.raises(SR.Invalid):
            SR.validate(_alter(text, tag, how), reads, refs)
    with pytest.raises(SR.Invalid):
        off = list(b.expected(format=1)["line_off"])
        off[3] += 1
        SR.validate(b.expected(format=1)["text"].decode(), reads, refs, off)


def test_golden_example():
    """The frozen worked example, its lines written out for every option set and checked by hand"""
    ex = json.load(open(GOLDEN))
    b = SK.Batch()
    b.refs, b.tnames = [r["seq"].encode() for r in ex["refs"]], [r["name"] for r in ex["refs"]]
    b.reads, b.qnames = [r["seq"].encode() for r in ex["reads"]], [r["name"] for r in ex["reads"]]
    b.quals, b.rep_len = [r["qual"].encode() for r in ex["reads"]], [r["rep_len"] for r in ex["reads"]]
    b.regs, b.alns, b.cigar, b.reg_off = ex["regs"], ex["alns"], ex["cigar"], ex["reg_off"]
    assert set(ex["expect"]) == set(SK.OPTION_SETS)
    for name, e in ex["expect"].items():
        text = "".join(ln + "\n" for ln in e["lines"]).encode()
        assert b.expected(**e["options"])["text"] == text, name
        assert MS.sam_cpu(MS.make_params(**e["options"]), *b.arrays())["text"] == text, name
        assert MS.sam_cpu(MS.make_params(**e["options"]), *b.arrays(), lanes=64)["text"] == text, name
    all_ = ex["expect"]["sam_all"]["lines"]
    assert all_[0].split("\t")[5] == "2S2=1X2=2I4=3D2=1X" and all_[0].endswith("cs:Z::2*ct:2+aa:4-tac:2*an\tMD:Z:2C6^TAC2A")
    assert all_[1].split("\t")[9:11] == ["ACCCGGG", "MF?81*#"] and all_[2].split("\t")[1] == "4"


@pytest.mark.parametrize("lanes", [1, 64])
def test_short_text_cap_reports_the_need_and_writes_nothing_past_it(lanes):
    b = SK.kinds_batch()
    o = SK.OPTION_SETS["sam_all"]
    want = b.expected(**o)
    full = len(want["text"])
    for cap in (0, 1, 100, full // 2, full - 1, full):
        T = ST.twin()
        p = MS.make_params(**o)
        g, ro, alns, cig, qn, reads, quals, rep, tn, refs = b.arrays()
        qa, qo = ST.pack_seqs(qn)
        ta, to = ST.pack_seqs(tn)
        seq, so = ST.pack_seqs(reads)
        ql, _ = ST.pack_seqs(quals)
        tseq, tso = ST.pack_seqs(refs)
        buf = np.full(cap + 64, 0xA5, np.uint8)
        line_off, cnt = np.zeros(len(ro), np.int64), np.zeros(2, np.int64)
        need = T.gbx_mm_sam_cpu_lanes(C.byref(p), lanes, len(ro) - 1, N.ptr(g), N.ptr(ro), N.ptr(alns), N.ptr(cig), len(cig), N.ptr(qa), N.ptr(qo), N.ptr(seq),
                                      N.ptr(ql), N.ptr(so), N.ptr(rep), len(to) - 1, N.ptr(ta), N.ptr(to), N.ptr(tseq), N.ptr(tso), N.ptr(buf), cap, N.ptr(line_off),
                                      N.ptr(cnt))
        assert need == full and buf[:cap].tobytes() == want["text"][:cap] and (buf[cap:] == 0xA5).all()
        assert list(line_off) == want["line_off"] and tuple(cnt) == want["counts"]


@pytest.mark.parametrize("min_ksw_len,max_ext,bw", [(8, 5000, 500), (200, 0, 500)])
def test_seeded_regions_through_the_align_stage(min_ksw_len, max_ext, bw):
    b = AK.seeded_batch(min_ksw_len, max_ext, bw)
    al = MA.align_cpu(MA.make_params(**b.P), *b.arrays())
    assert sum(int(a["flags"]) & 1 for a in al["alns"]) >= 10
    qn, tn = ["q%d" % i for i in range(len(b.reads))], ["contig_%d" % i for i in range(len(b.refs))]
    rep = np.arange(len(b.reads), dtype=np.int32) % 5
    quals = [bytes(33 + (i * 11) % 50 for i in range(len(r))) for r in b.reads]
    alns = [{k: int(a[k]) for k in SK.ALN_KEYS} for a in al["alns"]]
    for opts in ("sam_all", "sam_all_long", "paf_all", "sam_Y"):
        o = SK.OPTION_SETS[opts]
        want = SR.sam_text(SR.params(**o), b.regs, b.reg_off, alns, [int(w) for w in al["cigar"]], qn, b.reads, quals, rep, tn, b.refs)
        got = MS.sam_cpu(MS.make_params(**o), b.arrays()[0], b.reg_off, al["alns"], al["cigar"], qn, b.reads, quals, rep, tn, b.refs)
        same(got, want)
        if o.get("format"):
            n = SR.validate(got["text"].decode(), list(zip(qn, [r.decode() for r in b.reads])), list(zip(tn, [r.decode() for r in b.refs])), got["line_off"])
            assert n >= 10
    if max_ext == 0:
        same(MS.sam_cpu(MS.make_params(**o), b.arrays()[0], b.reg_off, al["alns"], al["cigar"], qn, b.reads, quals, rep, tn, b.refs, lanes=64), want)


# ------------------------------------------------------------------------------------------------ refusals
def test_host_entry_refuses_before_a_device():
    L, p = MS.lib(), MS.make_params(format=1)
    err = lambda: L.gbx_last_error().decode()
    i64 = lambda *v: np.array(v, np.int64)
    from genomicsbench_amd import mm_map as MM
    regs, alns = np.zeros(4, MM.REG_DTYPE), np.zeros(4, MA.ALN_DTYPE)
    regs["read"][:3] = [0, 1, 1]
    seq, cig, cnt, lo, nt = np.zeros(300, np.uint8), np.zeros(16, np.uint32), np.zeros(2, np.int64), np.zeros(4, np.int64), C.c_int64(0)
    names, noff, rep = np.frombuffer(b"abcd", np.uint8).copy(), i64(0, 2, 4), np.zeros(4, np.int32)

    def go(n, reg_off, qoff=noff, toff=noff, so=i64(0, 100, 200), tso=i64(0, 50, 90), lines=seq, text_cap=64, cig_=cig, n_cigar=16, p_=p, seq_=seq, tseq=seq, cnt_=cnt):
        return L.gbx_mm_sam_host(C.byref(p_), n, N.ptr(regs), N.ptr(reg_off), N.ptr(alns), N.ptr(cig_), n_cigar, N.ptr(names), N.ptr(qoff), N.ptr(seq_), None,
                                 N.ptr(so), N.ptr(rep), 2, N.ptr(names), N.ptr(toff), N.ptr(tseq), N.ptr(tso), N.ptr(lines), text_cap, N.ptr(lo), C.byref(nt),
                                 N.ptr(cnt_))
    ro = i64(0, 1, 3)
    assert go(2, None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, lines=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, cig_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, seq_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, tseq=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, cnt_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, ro, n_cigar=-1) == N.GBX_ERR_ARG and go(2, ro, text_cap=-1) == N.GBX_ERR_ARG
    assert go(2, i64(0, 2, 1)) == N.GBX_ERR_ARG and "reg_off is not monotone at read 1" in err()
    assert go(2, ro, toff=i64(1, 2, 4)) == N.GBX_ERR_ARG and "tname_off[0]" in err()
    assert go(2, ro, so=i64(0, 100, 50)) == N.GBX_ERR_ARG and "seq_off is not monotone at read 1" in err()
    assert go(2, ro, so=i64(0, 100, 100 + 2 ** 28)) == N.GBX_ERR_UNSUPPORTED and "read 1" in err()
    assert go(2, i64(0, 2, 3)) == N.GBX_ERR_ARG and "region 1 names read 1" in err()
    assert go(2, ro, p_=MS.make_params(cs=3)) == N.GBX_ERR_ARG and "cs" in err()
    assert go(2 ** 21 + 1, ro) == N.GBX_ERR_UNSUPPORTED and "reads" in err()
    assert go(0, i64(0), qoff=i64(0), so=i64(0)) == N.GBX_OK and nt.value == 0 and cnt.tolist() == [0, 0]


def test_device_entry_refuses_bad_arguments():
    L, p = MS.lib(), MS.make_params()
    n3, n4, n5, n6 = [None] * 3, [None] * 4, [None] * 5, [None] * 6
    assert L.gbx_mm_sam_device(C.byref(p), 1, *n3, 4, None, None, 0, *n6, 1, *n5, 10, *n4, 0, None) == N.GBX_ERR_ARG and "null" in L.gbx_last_error().decode()
    assert L.gbx_mm_sam_device(C.byref(p), 2 ** 21 + 1, *n3, 0, None, None, 0, *n6, 0, *n5, 0, *n4, 0, None) == N.GBX_ERR_UNSUPPORTED
    assert L.gbx_mm_sam_device(C.byref(MS.make_params(md=5)), 1, *n3, 0, None, None, 0, *n6, 0, *n5, 0, *n4, 0, None) == N.GBX_ERR_ARG
    assert "md" in L.gbx_last_error().decode()
    assert L.gbx_mm_sam_device(None, 1, *n3, 0, None, None, 0, *n6, 0, *n5, 0, *n4, 0, None) == N.GBX_ERR_ARG


def test_header():
    assert MS.header(["a", b"b"], [5, 7], ["-a", "x.fa", "y.fq"]) == "@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:a\tLN:5\n@SQ\tSN:b\tLN:7\n" \
                                                                    "@PG\tID:mmpaf\tPN:mmpaf\tCL:mmpaf -a x.fa y.fq\n"


# ------------------------------------------------------------------------------------------------ sanitizers, driver
def test_rules_under_asan_ubsan(tmp_path):
    """The host build of the rules in a stand-alone program under ASan + UBSan (tests/sanitize_mm_sam), every buffer exactly as large
    as the entry names, on every batch of the cases: clean, and the restatement's text.  One lane, and a team of threads."""
    r = subprocess.run(["make", "-C", SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from genomicsbench_amd import mm_map as MM
    for name in ("edges", "kinds", "letters", "malformed", "kinds_noqual"):
        b = SK.all_batches()[name]
        g, ro, alns, cig, qn, reads, quals, rep, tn, refs = b.arrays()
        qa, qo = MM.pack_names(qn)
        ta, to = MM.pack_names(tn)
        seq, so = ST.pack_seqs(reads)
        tseq, tso = ST.pack_seqs(refs)
        sets = [(k, 1) for k in sorted(SK.OPTION_SETS)] + [("sam_all", 16), ("paf_all", 4)]
        src, out = tmp_path / (name + ".bin"), tmp_path / (name + ".out")
        with open(src, "wb") as f:
            f.write(np.array([len(reads), len(g), len(refs), len(seq), len(tseq), len(qa), len(ta), len(cig), quals is not None, len(sets)], np.int64).tobytes())
            arrays = [g, ro, alns, cig, qa, qo, seq] + ([ST.pack_seqs(quals)[0]] if quals is not None else []) + [so, rep, ta, to, tseq, tso]
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
            for k, lanes in sets:
                f.write(bytes(MS.make_params(**SK.OPTION_SETS[k])) + np.int32(lanes).tobytes())
        r = subprocess.run([os.path.join(SAN, "_build", "sam_main"), str(src), str(out)], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
        raw, at, n = open(out, "rb").read(), 0, len(reads)
        for k, lanes in sets:
            want = b.expected(**SK.OPTION_SETS[k])
            need = int(np.frombuffer(raw, np.int64, 1, at)[0])
            cnt = tuple(int(v) for v in np.frombuffer(raw, np.int64, 2, at + 8))
            lo = np.frombuffer(raw, np.int64, n + 1, at + 24).tolist()
            text = raw[at + 24 + 8 * (n + 1):at + 24 + 8 * (n + 1) + need]
            at += 24 + 8 * (n + 1) + need
            assert (need, cnt, lo) == (len(want["text"]), tuple(want["counts"]), want["line_off"]) and text == want["text"], (name, k, lanes)
        assert at == len(raw)


def test_mmpaf_command_line(tmp_path):
    run = lambda *a: subprocess.run([MMPAF] + list(a), capture_output=True, text=True, timeout=60)
    r = run("--help")
    assert r.returncode == 0 and "[-a [-Y]]" in r.stdout and "--cs[=short|long]" in r.stdout and "--MD" in r.stdout and "--eqx" in r.stdout
    for args, word in ((("--cs", "a", "b"), "--cs needs -c or -a"), (("--cs=long", "a", "b"), "--cs=long needs -c or -a"), (("--MD", "a", "b"), "--MD needs -c or -a"),
                       (("--eqx", "a", "b"), "--eqx needs -c or -a"), (("-c", "--cs=both", "a", "b"), "--cs takes short or long"), (("-c", "-Y", "a", "b"), "-Y needs -a"),
                       (("-a", "-A", "0", "a", "b"), "a = 0")):                # -a implies -c: the align options are taken and checked
        r = run(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr)
    fa = tmp_path / "ref.fa"
    fa.write_text(">r\nACGT\n")
    for args in (("-a",), ("-a", "--cs", "--MD", "--eqx", "-Y"), ("-c", "--cs=short", "--MD", "--eqx")):
        r = run(*args, str(fa), str(tmp_path / "absent.fq"))
        assert r.returncode == 1 and "fail to open" in r.stderr, (args, r.stderr)
