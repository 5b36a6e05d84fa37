"""The base-level alignment stage on the GPU (gbx_mm_align_*, gbx_mm_paf_cigar_*), compared exactly - every record field, every
CIGAR word, the counts - with the restatement tests/mm_align_ref.py (its C twin runs the DP jobs Python is too slow for; the CPU
tests hold the two against each other); the capacities; then reads -> PAF with CIGAR on one stream (DeviceMmMapper(align=True))
and the mmpaf driver with -c.  There is no tolerance anywhere in this stage."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mm_align as MA
from genomicsbench_amd import mm_map as MM
from genomicsbench_amd import mm_seed as MS
import mm_align_cases as AK
import mm_align_ref as AR
import mm_map_cases as MK
from mm_align_cases import same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomicsbench_amd", "bin")
GUARD = 0x5a


def dev():
    import torch
    return torch.device("cuda:0")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def host(b, **kw):
    return MA.align_host(MA.make_params(**b.P), *b.arrays(), **kw)


def device_align(b, cigar_cap, z_bytes):
    """gbx_mm_align_device on a batch with the outputs in front of guard bytes -> the dict align_host gives (the words cut to the
    capacity) plus `intact`: nothing behind a capacity was touched"""
    import torch
    d = dev()
    g, ro, off, cax, cay, nc, reads, refs = b.arrays()
    seq, so = MS.pack_seqs(reads)
    tseq, to = MS.pack_seqs(refs)
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    t = lambda a, view=None: torch.from_numpy(pad(np.ascontiguousarray(a)).view(view or a.dtype)).to(d)
    nr, na, room = len(g), len(cax), 64
    tg, tro, toff, tcx, tcy, tnc = t(g.view(np.uint8)), t(ro), t(off), t(cax, np.int64), t(cay, np.int64), t(nc)
    tseq_, tso, ttseq, tto = t(seq), t(so), t(tseq), t(to)
    n_regs = torch.tensor([nr], dtype=torch.int64, device=d)
    alns = torch.full((nr * 56 + room,), GUARD, dtype=torch.uint8, device=d)
    cig = torch.full((cigar_cap * 4 + room,), GUARD, dtype=torch.uint8, device=d)
    z = torch.full((z_bytes + room,), GUARD, dtype=torch.uint8, device=d)
    cnt = torch.zeros(3, dtype=torch.int64, device=d)
    L, p = MA.lib(), MA.make_params(**b.P)
    wb = L.gbx_mm_align_workspace_bytes(len(reads), nr, na)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=d)
    N.check(L.gbx_mm_align_device(C.byref(p), len(reads), tg.data_ptr(), tro.data_ptr(), n_regs.data_ptr(), nr, toff.data_ptr(), tcx.data_ptr(), tcy.data_ptr(),
                                  tnc.data_ptr(), na, tseq_.data_ptr(), tso.data_ptr(), len(refs), ttseq.data_ptr(), tto.data_ptr(), alns.data_ptr(),
                                  cig.data_ptr(), cigar_cap, cnt.data_ptr(), z.data_ptr(), z_bytes, work.data_ptr(), wb, stream()))
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    a, w, zz = alns.cpu().numpy(), cig.cpu().numpy(), z.cpu().numpy()
    intact = (a[nr * 56:] == GUARD).all() and (w[cigar_cap * 4:] == GUARD).all() and (zz[z_bytes:] == GUARD).all()
    n = max(min(int(c[1]), cigar_cap), 0)
    return dict(alns=a[:nr * 56].view(MA.ALN_DTYPE), cigar=w[:n * 4].view(np.uint32), counts=tuple(int(v) for v in c), intact=bool(intact))


@pytest.mark.parametrize("kind", ["fill", "right", "left"])
@pytest.mark.parametrize("bw", AK.BANDS)
def test_single_job_regions(bw, kind):
    """One region a job: about forty (tl, ql) pairs of {1, 2, 63, 64, 65, 127, 128, 129, 200, 700} at every band, global fills
    (LEFT), right extensions (LEFT) and left extensions (reversed, RIGHT)"""
    for small in (True, False):
        b = AK.single_job_batch(bw, kind, small)
        if b.regs:
            same(host(b), b.expected(dp=AR.dp_job_c))


def test_tie_rules_leftmost_gap():
    """the generator asserts on the restatement's answer that every gap sits leftmost on the forward strand, in a fill, a right
    and a left extension, and - by re-scoring the gap shifted a unit at a time - that every case has more than one co-optimal
    placement"""
    b, want = AK.tie_batch()
    same(host(b), want)


def test_gap_pieces():
    b, want = AK.gap_batch()
    same(host(b), want)


def test_ambiguous_bases():
    b, want = AK.ambi_batch()
    same(host(b), want)


def test_zdrop_and_extension_ends():
    names = []
    for name, b, want in AK.zdrop_batches():
        same(host(b), want)
        names.append(name)
    assert names == ["dropped", "zdrop_off", "saved_by_l", "same_without_room", "empty", "end_bonus_0", "end_bonus_20"]


@pytest.mark.parametrize("min_ksw_len,max_ext", [(8, 5000), (200, 5000), (8, 0), (200, 10), (8, 10)])
def test_composed_regions(min_ksw_len, max_ext):
    """clipped target windows at both contig ends, a reverse-strand region, a read with two regions, spans that differ with
    anchors closer than half a span, invalid regions next to valid ones"""
    b, want = AK.region_batch(min_ksw_len, max_ext)
    same(host(b), want)


def test_measuring_switch_keeps_every_row_in_the_room(monkeypatch):
    """GBX_MM_ALIGN_LDS=0 (read per call; scripts/time_mm_align.py alternates it) changes where the rows live, not a byte of output"""
    monkeypatch.setenv("GBX_MM_ALIGN_LDS", "0")
    b, want = AK.region_batch(8, 5000)
    same(host(b), want)
    b, want = AK.tie_batch()
    same(host(b), want)


def test_wide_jobs_keep_their_rows_in_the_room():
    """rows wider than the LDS a wavefront has (a band of 600 around 700 bases and more, fills with a 600-base indel): the DP
    rows go to the job's room in z, other lanes' rows are read through memory, diagonals of hundreds of cells"""
    for b, want in AK.wide_batches():
        same(host(b), want)


@pytest.mark.parametrize("min_ksw_len,max_ext,bw", [(8, 5000, 500), (200, 5000, 500), (200, 0, 500), (8, 10, 20)])
def test_seeded_regions(min_ksw_len, max_ext, bw):
    b = AK.seeded_batch(min_ksw_len, max_ext, bw)
    same(host(b), b.expected(dp=AR.dp_job_c))


def test_device_entry_capacities():
    """z_bytes and cigar_cap too small through the device entry: the regions whose jobs end past z_bytes get flag 32 in region
    order whatever the scheduling, the counts report the needs, nothing is written at or past a capacity"""
    b, full = AK.region_batch(8, 5000)
    jobs, words, need = full["counts"]
    got = device_align(b, words, need)
    assert got.pop("intact")
    same(got, full)
    for z in (0, (need // 3) & ~15, need - 16):
        want = b.expected(z_bytes=z, dp=AR.dp_job_c)
        got = device_align(b, words, z)
        assert got.pop("intact")
        same(got, want)
        assert got["counts"][2] == need and any(a["flags"] == 32 for a in want["alns"])
    got = device_align(b, 7, need)
    assert got.pop("intact") and got["counts"] == (jobs, words, need) and got["cigar"].tolist() == full["cigar"][:7]
    fit = [i for i, a in enumerate(full["alns"]) if a["cigar_off"] + a["n_cigar"] <= 7]
    for k in AR.ALN_FIELDS:
        assert [int(got["alns"][k][i]) for i in fit] == [full["alns"][i][k] for i in fit], k


def test_host_entry_reports_the_needs():
    b, full = AK.gap_batch()
    with pytest.raises(N.GbxError) as e:
        host(b, cigar_cap=3, z_bytes=full["counts"][2])
    assert e.value.code == N.GBX_ERR_ARG and "%d CIGAR words" % full["counts"][1] in str(e.value)
    with pytest.raises(N.GbxError) as e:
        host(b, cigar_cap=full["counts"][1], z_bytes=full["counts"][2] - 16)
    assert e.value.code == N.GBX_ERR_ARG and "%d bytes of z" % full["counts"][2] in str(e.value)


def test_paf_with_cigar_host():
    g, ro, alns, cig, qn, so, rep, tn, to, text = AK.paf_case()
    got, line_off = MA.paf_cigar_host(g, ro, alns, cig, qn, so, rep, tn, to)
    assert got.decode() == text and line_off[-1] == len(text)
    with pytest.raises(N.GbxError) as e:
        MA.paf_cigar_host(g, ro, alns, cig, qn, so, rep, tn, to, text_cap=100)
    assert e.value.code == N.GBX_ERR_ARG and str(len(text)) in str(e.value)


def _paf_device(alns=None, cigar=None, n_reads=None, **kw):
    """both device entries on the composed regions of paf_case(): alns None is gbx_mm_paf_device"""
    g, ro, _, _, qn, so, rep, tn, to, text = AK.paf_case()
    return MK.device_paf(g, ro, qn, so, rep, tn, to, kw.get("reg_cap", len(g)), kw.get("text_cap", len(text) + 64), alns, cigar)


def test_paf_one_stage_two_modes():
    """The cigar entry on records with their flags cleared prints the plain entry's text; with every second record marked NO_ROOM those
    regions print plain lines and the rest cg:Z: lines, as the host build of the rule and the restatement do"""
    g, ro, alns, cig, qn, so, rep, tn, to, text = AK.paf_case()
    qlen, tlen = np.diff(so), np.diff(to)
    cleared = alns.copy()
    cleared["flags"] = 0
    plain = AR.paf_cigar([{k: int(r[k]) for k in AK.REG_KEYS} for r in g], ro, cleared, cig, qn, qlen, tn, tlen, rep)
    assert "cg:Z:" not in plain and plain.count("\n") == len(g)
    a, b = _paf_device(), _paf_device(cleared, cig)
    assert a["intact"] and b["intact"] and a["n_text"] == b["n_text"] == len(plain)
    assert a["text"][:len(plain)].decode() == plain and b["text"] == a["text"] and np.array_equal(a["line_off"], b["line_off"])
    mixed = alns.copy()
    mixed["flags"][1::2] |= MA.NO_ROOM
    want = AR.paf_cigar([{k: int(r[k]) for k in AK.REG_KEYS} for r in g], ro, mixed, cig, qn, qlen, tn, tlen, rep)
    n_cg = sum(1 for i, r in enumerate(alns) if i % 2 == 0 and r["flags"] & MA.ALIGNED and not r["flags"] & (MA.NO_ROOM | MA.INVALID))
    assert 0 < n_cg == want.count("cg:Z:") < text.count("cg:Z:")
    got = _paf_device(mixed, cig)
    cpu, cpu_off = MA.paf_cigar_cpu(g, ro, mixed, cig, qn, so, rep, tn, to)
    assert got["intact"] and got["n_text"] == len(want) and got["text"][:len(want)].decode() == want == cpu.decode()
    assert np.array_equal(got["line_off"], cpu_off)


@pytest.mark.parametrize("with_alns", [False, True], ids=["plain", "cigar"])
def test_paf_device_without_reads_or_room(with_alns):
    """no reads, and reads with room for no region: GBX_OK, no text, line_off all 0 - through both device entries"""
    g, ro, alns, cig, qn, so, rep, tn, to, _ = AK.paf_case()
    al = dict(alns=alns[:0], cigar=cig[:0]) if with_alns else {}
    got = MK.device_paf(g[:0], [0], [], [0], rep[:0], tn, to, 0, 0, **al)
    assert got["n_text"] == 0 and got["line_off"].tolist() == [0] and got["intact"]
    got = MK.device_paf(g[:0], np.zeros(len(ro), np.int64), qn, so, rep, tn, to, 0, 0, **al)
    assert got["n_text"] == 0 and not got["line_off"].any() and got["intact"]


@pytest.fixture(scope="module")
def mapper():
    c = MK.map_case()
    ix = MS.DeviceMmIndex(MS.make_params(**MK.MAP_PARAMS), c["refs"], dev(), stream())
    m = MM.DeviceMmMapper(MS.DeviceMmSeeder(ix, c["reads"]), read_names=c["qnames"], ref_names=c["tnames"], align=True)
    m.run(stream())
    return m


def test_mapper_with_align_end_to_end(mapper):
    """reads -> seeds -> chain scores -> regions -> alignments -> PAF with CIGAR on one stream: the regions are the restatement's
    (as without align), the records and words the alignment restatement's on them, the text rule 9's"""
    c = MK.map_case()
    e = c["exp"]
    assert mapper.fits() and mapper.aligner.fits()
    got = mapper.results()
    MK.same(got, e, c["batch"])
    b = AK.seeded_batch(200, 5000)
    want = b.expected(dp=AR.dp_job_c)
    assert mapper.aligner.counts()[:3] == tuple(want["counts"])
    same(dict(alns=got["alns"], cigar=got["cigar"], counts=mapper.aligner.counts()[:3]), want)
    qlen, tlen = [len(r) for r in c["reads"]], [len(r) for r in c["refs"]]
    text = AR.paf_cigar(e["regs"], e["reg_off"], want["alns"], want["cigar"], c["qnames"], qlen, c["tnames"], tlen, c["seeds"]["rep_len"])
    assert mapper.paf() == text and text.count("cg:Z:") == len(want["alns"])
    lo = got["line_off"]
    assert lo[0] == 0 and lo[-1] == len(text) and (np.diff(lo) >= 0).all()


def test_two_runs_are_identical(mapper):
    first, text = mapper.results(), mapper.paf()
    mapper.run(stream())
    again = mapper.results()
    assert first["alns"].tobytes() == again["alns"].tobytes() and np.array_equal(first["cigar"], again["cigar"]) and mapper.paf() == text


def test_mapper_reports_a_short_z_room(mapper):
    c = MK.map_case()
    need = mapper.aligner.counts()[2]
    m = MM.DeviceMmMapper(mapper.seeder, read_names=c["qnames"], ref_names=c["tnames"], align=True)
    m.aligner.caps = (None, (need // 2) & ~15, None)
    m.run(stream())
    assert not m.aligner.fits() and m.aligner.counts()[2] == need
    with pytest.raises(N.GbxError):
        m.paf()


def test_mmpaf_driver_with_c(tmp_path):
    """mmpaf -c on the mapped reads written to files gives the text of the restatement; without -c the text as before"""
    c = MK.map_case()
    fa, fq, out = tmp_path / "ref.fa", tmp_path / "reads.fq", tmp_path / "out.paf"
    with open(fa, "w") as f:
        for nm, r in zip(c["tnames"], c["refs"]):
            f.write(">%s some text\n" % nm)
            f.write("\n".join(r[o:o + 70].decode() for o in range(0, len(r), 70)) + "\n")
    with open(fq, "w") as f:
        for nm, r in zip(c["qnames"], c["reads"]):
            f.write("@%s\tmore\n%s\n+\n%s\n" % (nm, r.decode(), "I" * len(r)))
    qlen, tlen = [len(r) for r in c["reads"]], [len(r) for r in c["refs"]]
    e = c["exp"]
    for extra in ((), ("-A", "1", "-B", "3", "-O", "5,20", "-E", "2,1", "-z", "200", "--end-bonus", "7", "--min-ksw-len", "50", "--max-ext", "40", "-r", "100")):
        r = subprocess.run([os.path.join(BIN, "mmpaf"), "-c", "--mid-occ", str(MK.MAP_PARAMS["mid_occ"]), "-o", str(out)] + list(extra) + [str(fa), str(fq)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        if "-r" in extra:                                             # -r feeds chain's band too: other chain scores, other regions
            assert "Alignment:" in r.stderr and open(out).read().count("cg:Z:") > 10
            continue
        b = AK.seeded_batch(200, 5000)
        want = b.expected(dp=AR.dp_job_c)
        text = AR.paf_cigar(e["regs"], e["reg_off"], want["alns"], want["cigar"], c["qnames"], qlen, c["tnames"], tlen, c["seeds"]["rep_len"])
        assert open(out).read() == text
        assert "Alignment: %d jobs, %d CIGAR words" % tuple(want["counts"][:2]) in r.stderr
