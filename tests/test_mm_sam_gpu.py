"""The mm sam stage on the GPU (gbx_mm_sam_host, gbx_mm_sam_device), compared byte for byte with the restatement tests/mm_sam_ref.py
on every case of tests/mm_sam_cases.py and every option set; capacities behind guard bytes; two runs; then reads -> SAM on one
stream (DeviceMmMapper(align=True) -> DeviceMmSam) through the validator, and the mmpaf driver with -a.  There is no tolerance
anywhere in this stage."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mm_map as MM
from genomicsbench_amd import mm_sam as MSAM
from genomicsbench_amd import mm_seed as MS
from genomicsbench_amd import mm_stage as ST
import mm_map_cases as MK
import mm_sam_cases as SK
import mm_sam_ref as SR
from mm_sam_cases import same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomicsbench_amd", "bin")
GUARD = 0x5a
BATCHES = sorted(SK.all_batches())


def dev():
    import torch
    return torch.device("cuda:0")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def device_sam(b, opts, text_cap, reg_cap=None):
    """gbx_mm_sam_device on a batch with the text in front of guard bytes -> the dict sam_host gives (the text cut to the capacity)
    plus `intact`: nothing at or past the capacity was touched"""
    import torch
    d = dev()
    g, ro, alns, cig, qn, reads, quals, rep, tn, refs = b.arrays()
    qa, qo = ST.pack_seqs(qn)
    ta, to = ST.pack_seqs(tn)
    seq, so = ST.pack_seqs(reads)
    tseq, tso = ST.pack_seqs(refs)
    t = lambda a: torch.from_numpy(ST.pad(np.ascontiguousarray(a)).view(np.uint8)).to(d)
    n, nr, room = len(reads), len(g), 64
    reg_cap = nr if reg_cap is None else reg_cap
    tg, tro, tal, tcg, tqa, tqo, tseq_, tso_, trep, tta, tto, ttseq, ttso = [t(a) for a in (g, ro, alns, cig, qa, qo, seq, so, rep, ta, to, tseq, tso)]
    tql = None if quals is None else t(ST.pack_seqs(quals)[0])
    n_regs = torch.tensor([nr], dtype=torch.int64, device=d)
    lines = torch.full((text_cap + room,), GUARD, dtype=torch.uint8, device=d)
    line_off = torch.full((n + 1 + 8,), -7, dtype=torch.int64, device=d)
    cnt = torch.full((3,), -7, dtype=torch.int64, device=d)
    L, p = MSAM.lib(), MSAM.make_params(**opts)
    wb = L.gbx_mm_sam_workspace_bytes(n, reg_cap)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=d)
    N.check(L.gbx_mm_sam_device(C.byref(p), n, tg.data_ptr(), tro.data_ptr(), n_regs.data_ptr(), reg_cap, tal.data_ptr(), tcg.data_ptr(), len(cig), tqa.data_ptr(),
                                tqo.data_ptr(), tseq_.data_ptr(), None if tql is None else tql.data_ptr(), tso_.data_ptr(), trep.data_ptr(), len(refs),
                                tta.data_ptr(), tto.data_ptr(), ttseq.data_ptr(), ttso.data_ptr(), lines.data_ptr(), text_cap, line_off.data_ptr(),
                                cnt.data_ptr() + 16, cnt.data_ptr(), work.data_ptr(), wb, stream()))
    torch.cuda.synchronize()
    c, raw, lo = cnt.cpu().numpy(), lines.cpu().numpy(), line_off.cpu().numpy()
    intact = (raw[text_cap:] == GUARD).all() and (lo[n + 1:] == -7).all()
    return dict(text=raw[:min(int(c[2]), text_cap)].tobytes(), line_off=lo[:n + 1], n_text=int(c[2]), counts=(int(c[0]), int(c[1])), intact=bool(intact))


@pytest.mark.parametrize("batch", BATCHES)
def test_host_entry_equals_the_restatement(batch):
    b = SK.all_batches()[batch]
    for name, o in sorted(SK.OPTION_SETS.items()):
        try:
            same(MSAM.sam_host(MSAM.make_params(**o), *b.arrays()), b.expected(**o))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


@pytest.mark.parametrize("batch", BATCHES)
def test_device_entry_equals_the_restatement_behind_guard_bytes(batch):
    b = SK.all_batches()[batch]
    for name, o in sorted(SK.OPTION_SETS.items()):
        want = b.expected(**o)
        got = device_sam(b, o, len(want["text"]))
        assert got.pop("intact"), name
        try:
            same(got, want)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


def test_short_capacities_report_the_need():
    b = SK.kinds_batch()
    for name in ("sam_all", "paf_all"):
        o = SK.OPTION_SETS[name]
        want = b.expected(**o)
        full = len(want["text"])
        for cap in (0, 1, 100, full // 2, full - 1):
            got = device_sam(b, o, cap)
            assert got["intact"] and got["n_text"] == full and got["text"] == want["text"][:cap], (name, cap)
            assert list(got["line_off"]) == want["line_off"] and got["counts"] == tuple(want["counts"])
        with pytest.raises(N.GbxError) as e:
            MSAM.sam_host(MSAM.make_params(**o), *b.arrays(), text_cap=full - 1)
        assert e.value.code == N.GBX_ERR_ARG and str(full) in str(e.value)
    # regions at and past reg_cap do not exist: the text of the regions below it, the reads behind them unmapped
    o = SK.OPTION_SETS["sam_all"]
    cut = SK.Batch()
    for k in ("refs", "tnames", "reads", "qnames", "quals", "rep_len", "cigar"):
        setattr(cut, k, getattr(b, k))
    cut.regs, cut.alns, cut.reg_off = b.regs[:4], b.alns[:4], [min(v, 4) for v in b.reg_off]
    want = cut.expected(**o)
    got = device_sam(b, o, len(want["text"]) + 100, reg_cap=4)
    assert got.pop("intact")
    same(got, want)


def test_two_runs_give_identical_bytes():
    b, o = SK.edge_batch(), SK.OPTION_SETS["sam_all"]
    n = len(b.expected(**o)["text"])
    first, again = device_sam(b, o, n), device_sam(b, o, n)
    assert first["text"] == again["text"] and np.array_equal(first["line_off"], again["line_off"]) and first["counts"] == again["counts"]


def test_no_reads_and_no_regions():
    e = SK.Batch()
    got = device_sam(e, SK.OPTION_SETS["sam_all"], 0)
    assert got["intact"] and got["n_text"] == 0 and got["line_off"].tolist() == [0] and got["counts"] == (0, 0)
    e.ref(b"ACGT")
    e.read(b"ACGTT", "lonely")
    for name, n_lines in (("sam", 1), ("paf_all", 0)):
        want = e.expected(**SK.OPTION_SETS[name])
        got = device_sam(e, SK.OPTION_SETS[name], 64, reg_cap=0)
        assert got.pop("intact") and got["counts"] == (n_lines, 0)
        same(got, want)


@pytest.fixture(scope="module")
def mapper():
    c = MK.map_case()
    ix = MS.DeviceMmIndex(MS.make_params(**MK.MAP_PARAMS), c["refs"], dev(), stream())
    m = MM.DeviceMmMapper(MS.DeviceMmSeeder(ix, c["reads"]), read_names=c["qnames"], ref_names=c["tnames"], align=True)
    m.run(stream())
    return m


def _quals(c):
    return [bytes(33 + (i * 7 + len(r)) % 60 for i in range(len(r))) for r in c["reads"]]


def test_mapper_to_sam_end_to_end(mapper):
    """reads -> seeds -> chains -> regions -> alignments -> SAM on one stream: the restatement's text on the stage's own records, and
    every record through the validator"""
    c = MK.map_case()
    quals = _quals(c)
    o = SK.OPTION_SETS["sam_all"]
    sam = MSAM.DeviceMmSam(mapper.aligner, MSAM.make_params(**o), quals=quals)
    sam.run(stream())
    assert mapper.fits() and mapper.aligner.fits() and sam.fits()
    text = sam.text()
    res = mapper.results()
    regs = [{k: int(res["regs"][k][i]) for k in SK.REG_KEYS} for i in range(len(res["regs"]))]
    alns = [{k: int(a[k]) for k in SK.ALN_KEYS} for a in res["alns"]]
    want = SR.sam_text(SR.params(**o), regs, [int(v) for v in res["reg_off"]], alns, [int(w) for w in res["cigar"]], c["qnames"], c["reads"], quals,
                       [int(v) for v in c["seeds"]["rep_len"]], c["tnames"], c["refs"])
    assert text.encode("latin-1") == want["text"] and sam.counts()[:2] == tuple(want["counts"])
    lo = sam.results()["line_off"]
    assert lo.tolist() == want["line_off"]
    n = SR.validate(text, list(zip(c["qnames"], [r.decode() for r in c["reads"]])), list(zip(c["tnames"], [r.decode() for r in c["refs"]])), lo)
    assert n >= 10 and n == sum(SR.prints(a, len(res["cigar"])) for a in alns)
    sam.run(stream())
    assert sam.text() == text
    short = MSAM.DeviceMmSam(mapper.aligner, MSAM.make_params(**o), quals=quals, text_cap=len(text) // 2)
    short.run(stream())
    assert not short.fits() and short.counts()[2] == len(text)
    with pytest.raises(N.GbxError):
        short.text()


def test_mmpaf_driver_with_a(mapper, tmp_path):
    """mmpaf -a --cs --MD --eqx on the same reads written to files equals the Python path's text below the @PG line; the header; and
    without a new option the driver prints what it printed"""
    c = MK.map_case()
    quals = _quals(c)
    fa, fq, out = tmp_path / "ref.fa", tmp_path / "reads.fq", tmp_path / "out.sam"
    with open(fa, "w") as f:
        for nm, r in zip(c["tnames"], c["refs"]):
            f.write(">%s some text\n" % nm)
            f.write("\n".join(r[o:o + 70].decode() for o in range(0, len(r), 70)) + "\n")
    with open(fq, "wb") as f:
        for nm, r, q in zip(c["qnames"], c["reads"], quals):
            f.write(b"@%s\tmore\n%s\n+\n%s\n" % (nm.encode(), r, q))
    sam = MSAM.DeviceMmSam(mapper.aligner, MSAM.make_params(format=1, cs=1, md=1, eqx=1), quals=quals)
    sam.run(stream())
    args = ["-a", "--cs", "--MD", "--eqx", "--mid-occ", str(MK.MAP_PARAMS["mid_occ"]), "-o", str(out), str(fa), str(fq)]
    r = subprocess.run([os.path.join(BIN, "mmpaf")] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = open(out, "rb").read().decode("latin-1")
    head = MSAM.header(c["tnames"], [len(t) for t in c["refs"]], args)
    assert got.startswith(head) and got[len(head):] == sam.text()
    paf = []
    for extra in (["-c"], ["-c", "--cs=long", "--MD", "--eqx"]):
        r = subprocess.run([os.path.join(BIN, "mmpaf")] + extra + ["--mid-occ", str(MK.MAP_PARAMS["mid_occ"]), "-o", str(out), str(fa), str(fq)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        paf.append(open(out).read())
    assert paf[0] == mapper.paf()
    tagged = MSAM.DeviceMmSam(mapper.aligner, MSAM.make_params(cs=2, md=1, eqx=1))
    tagged.run(stream())
    assert paf[1] == tagged.text() and paf[1].count("cs:Z:=") == paf[0].count("cg:Z:")
