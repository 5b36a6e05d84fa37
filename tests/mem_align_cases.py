"""Inputs and expected outputs for the aligner's tests (tests/test_mem_align_cpu.py, tests/test_mem_align_gpu.py): generated
reads, and the EXISTING composition of the stage classes (mem_pipeline.Stages, which mem_sam.pipeline queues through) with generous
capacities, which is what the aligner has to equal byte for byte.  The composition asserts that none of its capacities overflowed."""
import ctypes as C

import numpy as np

from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd import mem_cigar as MG
from genomicsbench_amd import mem_pair as MP
from genomicsbench_amd import mem_sam as SM
from genomicsbench_amd.mem_pipeline import Stages
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


def compose(g, rs, names, qual, id0, cap=8000, **options):
    """The composition on its own stream, from the index to the SAM stage -> (Stages, the torch stream); `options` go to
    mem_pipeline.Stages (skip, pes, params)."""
    import torch
    idx, smp = FM.build_index(g, sa_compx=3)
    p = MG.make_params()
    z = 8 * rs.n_reads * MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), 151, 302)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = FM.DeviceFmi(idx, rs, torch.device("cuda:0"))
        d.set_sa(smp)
        params = dict(options.pop("params", {}), cigar=p)
        st = Stages(d, MC.text_of(g), len(g), CONTIG_OFF, id0=id0, params=params, caps=dict(pos_cap=cap, cigar_cap=8 * cap, z_bytes=z),
                    sam_input=(names, qual, CONTIG_NAMES), **options)
        st.queue(stream.cuda_stream)
    return st, stream


def finish(st, stream):
    stream.synchronize()
    res = st.check()                                     # each stage raises when one of its capacities overflowed
    assert not (res["cigar"][0]["rid"] == -2).any()
    got = res["sam"]
    pes = res["pair"]["pes"] if "pair" in res else None
    stages = [st.st[n] for n in st.names[3:]]             # from the regs stage on
    return dict(sam=got["lines"].tobytes(), recs=got["recs"], rec_off=got["rec_off"], pes=pes, stages=stages)


def compose_paired(g, rs, names, qual, id0):
    """regs -> pestat -> rescue -> pair -> cigar -> sam, which is mem_sam.pipeline (no header) behind the same extension."""
    import torch
    st, stream = compose(g, rs, names, qual, id0)
    out = finish(st, stream)
    with torch.cuda.stream(stream):
        sam, _ = SM.pipeline(st.extend, names, qual, CONTIG_NAMES, stream.cuda_stream, id0, with_header=False, cigar_params=st.params["cigar"],
                             cigar_cap=st.caps["cigar_cap"], z_bytes=st.caps["z_bytes"])
    assert out["sam"] == sam
    out["rescue_stats"] = st.rescue.results()["stats"]
    return out


def compose_variant(g, rs, names, qual, id0, pes=None, no_rescue=False, no_pairing=False):
    """What mem_sam.pipeline has no argument for: a given estimate, no rescue (bwa -S), no pairing (bwa -P)."""
    pp = MP.make_params(no_pairing=1 if no_pairing else 0)
    return finish(*compose(g, rs, names, qual, id0, pes=pes, skip=("rescue",) if no_rescue else (), params=dict(pair=pp)))


def compose_single(g, rs, names, qual, id0):
    """regs -> cigar on the regs stage's list -> DeviceMemSam mode 0."""
    return finish(*compose(g, rs, names, qual, id0, skip=("rescue", "pair")))


def same_output(got, want, pes=True):
    assert got["sam"] == want["sam"]
    assert got["recs"].tobytes() == want["recs"].tobytes()
    assert np.array_equal(got["rec_off"], want["rec_off"])
    if pes:
        assert got["pes"].tobytes() == want["pes"].tobytes()
