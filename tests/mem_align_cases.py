"""Inputs and expected outputs for the aligner's tests (tests/test_mem_align_cpu.py, tests/test_mem_align_gpu.py): generated
reads, and the EXISTING composition of the stage classes (mem_sam.pipeline and its parts) with generous capacities, which is what
the aligner has to equal byte for byte.  The composition asserts that none of its capacities overflowed."""
import ctypes as C

import numpy as np

from genomicsbench_amd import _native as N
from genomicsbench_amd import bsw_seeds as BS
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd import mem_cigar as MG
from genomicsbench_amd import mem_pair as MP
from genomicsbench_amd import mem_regs as MR
from genomicsbench_amd import mem_rescue as MS
from genomicsbench_amd import mem_sam as SM
import mem_rescue_cases as KR

CONTIG_OFF = np.array([0, 14_000, 30_000], dtype=np.int64)
CONTIG_NAMES = ["first", "second_contig"]
LETTERS = "ACGTN"


def genome(seed=8301):
    return KR.genome(30_000, seed)


def revcomp(s):
    s = np.asarray(s, dtype=np.uint8)
    return np.where(s < 4, 3 - s, 4).astype(np.uint8)[::-1].copy()


def pairs(g, n, seed, mean=300., sd=25.):
    """n FR pairs of 101 bases cut from g, interleaved -> (FmiReadSet, names, qual).  Every fifth pair's mate has a substitution
    every 15 bases (no exact 19-mer: only the rescue finds it); every seventh pair's first read is chimeric: 50 bases of the
    fragment, then 51 from another place on the other strand."""
    rng = np.random.default_rng(seed)
    reads = []
    for k in range(n):
        frag = max(150, int(round(rng.normal(mean, sd))))
        at = int(rng.integers(0, len(g) - frag))
        ends = [g[at:at + 101].copy(), revcomp(g[at + frag - 101:at + frag])]
        if k % 5 == 4:
            ends[1][7::15] = (ends[1][7::15] + 1) % 4
        if k % 7 == 3:
            other = int(rng.integers(0, len(g) - 101))
            ends[0][50:] = revcomp(g[other:other + 51])
        reads += ends
    rs = FM.FmiReadSet.fixed(np.array(reads, dtype=np.uint8))
    names = ["pair%d" % (k // 2) for k in range(2 * n)]
    qual = np.random.default_rng(seed + 2).integers(33, 74, len(rs.enc)).astype(np.uint8)
    return rs, names, qual


def mixed(g, n, seed):
    """n single reads of 30..151 bases -> (FmiReadSet, names, qual, letters): read 3 is all N, read 5 has 12 bases (below
    min_seed_len), and read 7's letters are lower case in its FASTQ form (`letters`: one str per read; the codes are the same).
    One read in four is reverse-complemented, one in three carries two substitutions."""
    rng = np.random.default_rng(seed)
    seqs, letters = [], []
    for k in range(n):
        ln = 12 if k == 5 else int(rng.integers(30, 152))
        at = int(rng.integers(0, len(g) - ln))
        s = g[at:at + ln].copy()
        if k % 4 == 1:
            s = revcomp(s)
        if k % 3 == 2 and ln > 40:
            for at2 in rng.integers(0, ln, 2):
                s[at2] = (s[at2] + 1) % 4
        if k == 3:
            s[:] = 4
        seqs.append(s)
        t = "".join(LETTERS[c] for c in s)
        letters.append(t.lower() if k == 7 else t)
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.zeros(n, dtype=np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    rs = FM.FmiReadSet(np.concatenate(seqs), off, lens)
    names = ["read%d" % k for k in range(n)]
    qual = np.random.default_rng(seed + 2).integers(33, 74, len(rs.enc)).astype(np.uint8)
    return rs, names, qual, letters


def fastq(names, letters, qual, read_off, suffix=""):
    """FASTQ text of reads given as letters; qual: the uint8 arena at read_off."""
    out = []
    for k, (n, s) in enumerate(zip(names, letters)):
        q = bytes(qual[int(read_off[k]):int(read_off[k]) + len(s)]).decode("latin-1")
        out.append("@%s%s\n%s\n+\n%s\n" % (n, suffix, s, q))
    return "".join(out)


def letters_of(rs):
    return ["".join(LETTERS[c] for c in rs.enc[int(o):int(o) + int(l)]) for o, l in zip(rs.read_off, rs.read_len)]


class Composed:
    """The stages up to the seed extension, queued as tests/test_mem_sam_gpu.py::test_whole_pipeline_on_one_stream queues them."""

    def __init__(self, g, rs, cap=8000):
        import torch
        self.g, self.rs, self.cap = g, rs, cap
        self.idx, self.smp = FM.build_index(g, sa_compx=3)
        self.text = MC.text_of(g)
        self.stream = torch.cuda.Stream()
        s = self.stream.cuda_stream
        with torch.cuda.stream(self.stream):
            d = self.fmi = FM.DeviceFmi(self.idx, rs, torch.device("cuda:0"))
            d.set_sa(self.smp)
            d.run(s)
            d.sal(500, pos_cap=cap, stream=s)
            self.chain = MC.DeviceMemChain(d, len(g), CONTIG_OFF)
            self.chain.run(s)
            self.ext = self.chain.extension(self.text)
            self.ext.run(BS.make_seed_params(), s)

    def check_front(self):
        d = self.fmi
        assert int(d.n_out.item()) <= d.out_cap and int(d.n_pos.item()) <= self.cap and not d.overflow()
        self.chain.results()


def _finish(c, sm, cg, stages, pe=None):
    c.stream.synchronize()
    c.check_front()
    for st in stages:
        st.results()                                     # each raises when one of its capacities overflowed
    alns, _ = cg.results()
    assert not (alns["rid"] == -2).any()
    got = sm.results()
    pes = pe.results()["pes"] if pe is not None else None
    return dict(sam=got["lines"].tobytes(), recs=got["recs"], rec_off=got["rec_off"], pes=pes, stages=stages)


def _cigar_room(n_reads):
    p = MG.make_params()
    return p, 8 * n_reads * MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), 151, 302)


def compose_paired(g, rs, names, qual, id0):
    """mem_sam.pipeline (regs -> pestat -> rescue -> pair -> cigar -> sam), no header."""
    import torch
    c = Composed(g, rs)
    p, z = _cigar_room(rs.n_reads)
    with torch.cuda.stream(c.stream):
        sam, (rg, rsc, pe, cg, sm) = SM.pipeline(c.ext, names, qual, CONTIG_NAMES, c.stream.cuda_stream, id0, with_header=False, cigar_params=p,
                                                 cigar_cap=8 * c.cap, z_bytes=z)
    out = _finish(c, sm, cg, [rg, rsc, pe, cg, sm], pe)
    assert out["sam"] == sam
    out["rescue_stats"] = rsc.results()["stats"]
    return out


def compose_variant(g, rs, names, qual, id0, pes=None, no_rescue=False, no_pairing=False):
    """The same classes queued by hand for what mem_sam.pipeline has no argument for: a given estimate, no rescue (bwa -S),
    no pairing (bwa -P)."""
    import torch
    c = Composed(g, rs)
    p, z = _cigar_room(rs.n_reads)
    s = c.stream.cuda_stream
    pp = MP.make_params(no_pairing=1 if no_pairing else 0)
    with torch.cuda.stream(c.stream):
        rg = MR.DeviceMemRegs(c.ext, None, read_id0=2 * int(id0))
        rg.run(s)
        stages = [rg]
        before = rg
        if not no_rescue:
            before = MS.DeviceMemRescue(rg, None, pp, pes=pes)
            before.run(s)
            stages.append(before)
            pe = MP.DeviceMemPair(before, pp, pes_in=before.pes_host(s))
        else:
            pe = MP.DeviceMemPair(rg, pp, pes_in=pes)
        pe.run(s)
        cg = MG.DeviceMemCigar(pe.cigar_input, p, cigar_cap=8 * c.cap, z_bytes=z)
        cg.run(s)
        sm = SM.DeviceMemSam(pe, cg, names, qual, CONTIG_NAMES)
        sm.run(s)
    return _finish(c, sm, cg, stages + [pe, cg, sm], pe)


def compose_single(g, rs, names, qual, id0):
    """regs -> cigar on the regs stage's list -> DeviceMemSam mode 0."""
    import torch
    c = Composed(g, rs)
    p, z = _cigar_room(rs.n_reads)
    s = c.stream.cuda_stream
    with torch.cuda.stream(c.stream):
        rg = MR.DeviceMemRegs(c.ext, None, read_id0=int(id0))
        rg.run(s)
        cg = MG.DeviceMemCigar(rg.cigar_input, p, cigar_cap=8 * c.cap, z_bytes=z)
        cg.run(s)
        sm = SM.DeviceMemSam(rg, cg, names, qual, CONTIG_NAMES)
        sm.run(s)
    return _finish(c, sm, cg, [rg, cg, sm])


def same_output(got, want, pes=True):
    assert got["sam"] == want["sam"]
    assert got["recs"].tobytes() == want["recs"].tobytes()
    assert np.array_equal(got["rec_off"], want["rec_off"])
    if pes:
        assert got["pes"].tobytes() == want["pes"].tobytes()
