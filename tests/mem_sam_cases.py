"""Inputs of the SAM-record tests (gbx_mem_sam_*), shared by the CPU and the GPU tests: hand-built calls of the stage, one per rule
and branch of DESIGN 3.15, with the lines they must give written out in EXPECT (tests/golden/mem_sam_example.json holds the long
ones), and what the generated-pairs test needs.

A read is given as its alignments in SAM terms - contig, position, strand, CIGAR, the M positions that mismatch - and the read's
bases are made from the text to fit them; the builder turns that into what the stages before hand over.  A job is dict(mode,
softclip, regs, reg_off, pairs, alns, cigar, qer, read_off, read_len, qual, names, contig_names, text, L, contig_off)."""
import functools
import json
import os
import re

import numpy as np

import mem_sam_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REG_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("seed", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("read", "<i4"), ("rid", "<i4"),
                      ("score", "<i4"), ("truesc", "<i4"), ("sub", "<i4"), ("sub_n", "<i4"), ("w", "<i4"), ("seedcov", "<i4"),
                      ("seedlen0", "<i4"), ("secondary", "<i4"), ("mapq", "<i4"), ("flag", "<i4"), ("sel", "<i4"), ("csub", "<i4")])
ALN_DTYPE = np.dtype([("pos", "<i8"), ("cigar_off", "<i8"), ("rid", "<i4"), ("is_rev", "<i4"), ("n_cigar", "<i4"), ("nm", "<i4"),
                      ("score", "<i4"), ("w", "<i4"), ("tries", "<i4"), ("pad_", "<i4")])
PAIR_DTYPE = np.dtype([("dist", "<i8"), ("score", "<i4"), ("sub", "<i4"), ("n_sub", "<i4"), ("n_cand", "<i4"), ("z0", "<i4"), ("z1", "<i4"),
                       ("q_pe", "<i4"), ("q_se0", "<i4"), ("q_se1", "<i4"), ("paired", "<i4"), ("proper", "<i4"), ("dir", "<i4")])
assert REG_DTYPE.itemsize == 88 and ALN_DTYPE.itemsize == 48 and PAIR_DTYPE.itemsize == 56
OPN = {"M": 0, "I": 1, "D": 2, "S": 4}


def words_of(cigar):
    return [int(n) << 4 | OPN[op] for n, op in re.findall(r"(\d+)([MIDS])", cigar)]


def genome(n, seed, n_at=()):
    g = np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)
    g[list(n_at)] = 4
    return g


def text_of(g):
    return np.concatenate([g, np.where(g[::-1] < 4, 3 - g[::-1], 4).astype(np.uint8)])


def aln(rid, pos, rev, cigar, mm=(), nread=(), mapq=60, score=None, sub=0, csub=0):
    """One alignment of a read: mm / nread: the M positions (counted along the M runs in SAM order) where the read gets another
    base / an N."""
    return dict(rid=rid, pos=pos, rev=rev, cigar=cigar, mm=tuple(mm), nread=tuple(nread), mapq=mapq, score=score, sub=sub, csub=csub)


def build(reads, g, contig_off, contig_names, mode, softclip=0, seed=7, proper=None, with_qual=True, text=None, extra_regions=True):
    """reads: [(name, length, [aln, ...])].  -> a job.  The alignments of a read go into alns in reverse order, so that sel is
    no identity, and every read gets an unreported region in front when extra_regions."""
    rng = np.random.default_rng(seed)
    contig_off = np.asarray(contig_off, dtype=np.int64)
    L = int(contig_off[-1])
    text = text_of(g) if text is None else text
    qer, read_off, read_len, regs, reg_off, alns, cigar, names = [], [], [], [], [0], [], [], []
    at = 0
    for r, (name, lq, als) in enumerate(reads):
        stored = rng.integers(0, 4, lq).astype(np.uint8)
        for a in als:
            start = int(contig_off[a["rid"]]) + a["pos"]
            i, t, k = 0, start, 0
            for w in words_of(a["cigar"]):
                op, l = w & 15, w >> 4
                if op == 0:
                    for j in range(l):
                        c = int(text[t + j])
                        b = ((c + 1) % 4 if c < 4 else 0) if k in a["mm"] else 4 if k in a["nread"] else c
                        si = lq - 1 - (i + j) if a["rev"] else i + j
                        stored[si] = (3 - b if b < 4 else 4) if a["rev"] else b
                        k += 1
                    i += l
                    t += l
                elif op == 2:
                    t += l
                else:
                    i += l
            assert i == lq, (name, a["cigar"], i, lq)
        # the edit distance, counted on the finished read
        first = len(alns)
        for which, a in enumerate(als):
            seq = R.printed_codes(stored, a["rev"])
            ws = words_of(a["cigar"])
            nonclip = [k for k, w in enumerate(ws) if w & 15 != 4]
            i, t, nm = 0, int(contig_off[a["rid"]]) + a["pos"], 0
            for k, w in enumerate(ws):
                op, l = w & 15, w >> 4
                if op == 0:
                    nm += sum(seq[i + j] != min(int(text[t + j]), 4) for j in range(l))
                    i, t = i + l, t + l
                elif op == 2:
                    nm += l if k not in (nonclip[0], nonclip[-1]) else 0
                    t += l
                else:
                    nm += l if op == 1 else 0
                    i += l
            a["nm"] = nm
        if extra_regions:
            regs.append(dict(read=r, flag=0, sel=-1, score=20, mapq=0))
        order = list(range(len(als)))[::-1]
        slot = {}
        for k in order:
            a = als[k]
            ws = words_of(a["cigar"])
            slot[k] = len(alns)
            alns.append((a["pos"], len(cigar), a["rid"], a["rev"], len(ws), a["nm"], 0, 0, 1, 0))
            cigar += ws
        for which, a in enumerate(als):
            m = sum(w >> 4 for w in words_of(a["cigar"]) if w & 15 == 0)
            regs.append(dict(read=r, flag=1 | (0x800 if which else 0), sel=slot[which], score=m - 5 * a["nm"] if a["score"] is None else a["score"],
                             mapq=a["mapq"], sub=a["sub"], csub=a["csub"], rid=a["rid"]))
        del first
        reg_off.append(len(regs))
        read_off.append(at)
        read_len.append(lq)
        qer.append(stored)
        qer.append(np.full(3, 9, np.uint8))              # a gap between the reads: the offsets are no running sum
        at += lq + 3
        names.append(name)
    R_ = np.zeros(len(regs), dtype=REG_DTYPE)
    R_["secondary"] = -1
    for k, x in enumerate(regs):
        for f, v in x.items():
            R_[f][k] = v
    qer = np.concatenate(qer) if qer else np.zeros(0, np.uint8)
    qual = rng.integers(33, 74, len(qer)).astype(np.uint8) if with_qual else None
    pairs = None
    if mode == 1:
        pairs = np.zeros(len(reads) // 2, dtype=PAIR_DTYPE)
        pairs["proper"] = 1 if proper is None else proper
    return dict(mode=mode, softclip=softclip, regs=R_, reg_off=np.array(reg_off, np.int64), pairs=pairs,
                alns=np.array(alns, dtype=ALN_DTYPE) if alns else np.zeros(0, ALN_DTYPE), cigar=np.array(cigar, dtype=np.uint32),
                qer=qer, read_off=np.array(read_off, np.int64), read_len=np.array(read_len, np.int32), qual=qual, names=names,
                contig_names=list(contig_names), text=text, L=L, contig_off=contig_off)


def reference(j, **caps):
    return R.sam_all(j["mode"], j["regs"], j["reg_off"], j["pairs"], j["alns"], j["cigar"], j["qer"], j["read_off"], j["read_len"], j["qual"],
                     j["names"], j["contig_names"], j["text"], j["L"], j["contig_off"], j["softclip"], **caps)


def same(got, want):
    """The arrays of a call against the restatement's, byte for byte."""
    assert (got["n_recs"], got["n_md"], got["n_text"]) == (want["n_recs"], want["n_md"], want["n_text"])
    assert np.array_equal(got["rec_off"], want["rec_off"])
    assert got["lines"].tobytes() == want["lines"].tobytes()
    assert got["md"].tobytes() == want["md"].tobytes()
    for f in R.SAM_DTYPE.names:
        assert np.array_equal(got["recs"][f], want["recs"][f]), f
    assert got["recs"].tobytes() == want["recs"].tobytes()


CO = np.array([0, 1500, 4000], dtype=np.int64)
CN = ["chr1", "contig_two"]


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> job."""
    H = {}
    g = genome(4000, 4201, n_at=(700, 701, 2300))
    # M runs of 1, 63, 64, 65 and 129 positions with mismatches at 0, 63, 64 and the last position, adjacent ones, none and all
    reads = []
    for n in (1, 63, 64, 65, 129):
        sets = {"none": (), "first": (0,), "last": (n - 1,), "all": tuple(range(n))}
        if n > 64:
            sets.update({"at63": (63,), "at64": (64,), "adjacent": (63, 64), "three": (0, 1, 2)})
        for k, (what, mm) in enumerate(sorted(sets.items())):
            reads.append(("m%d_%s" % (n, what), n, [aln(0, 20 + 7 * k, k & 1, "%dM" % n, mm=mm, mapq=60 if k & 1 else 0)]))
    H["m_runs"] = build(reads, g, CO, CN, 0)
    # MD counts and POS across 9 / 10 and 99 / 100
    reads = [("count_%d" % pos, 250, [aln(1, pos, 0, "250M", mm=(9, 20, 120, 221))]) for pos in (8, 9, 98, 99)]
    H["counts_pos"] = build(reads, g, CO, CN, 0, extra_regions=False)
    # TLEN negative, zero and positive, mapq 0 and 60
    reads = [("fr", 50, [aln(0, 100, 0, "50M", mapq=60)]), ("fr", 50, [aln(0, 300, 1, "50M", mm=(3,), mapq=0)]),
             ("rf", 40, [aln(0, 500, 1, "40M")]), ("rf", 40, [aln(0, 420, 0, "40M")]),
             ("same", 30, [aln(1, 77, 0, "30M")]), ("same", 30, [aln(1, 77, 0, "30M")]),
             ("meet", 30, [aln(1, 200, 0, "30M")]), ("meet", 1, [aln(1, 200, 1, "1M")])]
    H["tlen"] = build(reads, g, CO, CN, 1, proper=[1, 0, 1, 1])
    # interior D and I, a D next to a mismatch on either side, a D as the first and as the last op that is no clip
    reads = [("d_i", 60, [aln(0, 900, 0, "20M2D10M3I27M", mm=(5,))]), ("d_mm", 40, [aln(0, 1000, 0, "20M3D20M", mm=(19, 20))]),
             ("d_last", 30, [aln(0, 1100, 0, "25M2D5S")]), ("d_first", 30, [aln(0, 1150, 1, "4S2D26M", mm=(0,))]),
             ("i_rev", 45, [aln(1, 600, 1, "3S10M1I10M1D21M", mm=(10,))]), ("d_d", 30, [aln(1, 700, 0, "10M1D10M1D10M")])]
    H["indels"] = build(reads, g, CO, CN, 0)
    # N in the read, in the text (700, 701 and contig_two's 800) and in both
    reads = [("n_read", 30, [aln(0, 400, 0, "30M", nread=(4, 29))]), ("n_text", 30, [aln(0, 690, 0, "30M")]),
             ("n_both", 30, [aln(0, 695, 1, "30M", nread=(5, 8))]), ("n_text_del", 30, [aln(1, 790, 0, "9M2D21M")])]
    H["n_bases"] = build(reads, g, CO, CN, 0)
    # reverse-strand records with clips on either side, as supplementary records too, hard- and soft-clipped
    reads = [("chim", 100, [aln(0, 150, 1, "10S55M35S", mm=(7,)), aln(1, 1000, 1, "70S27M3S", mapq=25, sub=19),
                            aln(1, 300, 0, "90S10M", mapq=70, csub=11)]),
             ("chim", 80, [aln(0, 350, 0, "5S70M5S", mm=(69,)), aln(1, 1200, 0, "75S5M", mapq=3)])]
    H["three_records"] = build(reads, g, CO, CN, 1)
    H["three_records_Y"] = build(reads, g, CO, CN, 1, softclip=1)
    H["three_records_se"] = build(reads, g, CO, CN, 0)
    # unmapped ends: with a mapped reverse mate, with a mapped forward mate, both; mates on different contigs
    reads = [("u_rev", 35, []), ("u_rev", 35, [aln(1, 50, 1, "5S30M")]), ("u_fwd", 20, [aln(0, 10, 0, "20M")]), ("u_fwd", 25, []),
             ("none", 12, []), ("none", 13, []), ("apart", 30, [aln(0, 1400, 0, "30M")]), ("apart", 30, [aln(1, 0, 1, "30M", mapq=17)])]
    H["unmapped"] = build(reads, g, CO, CN, 1, proper=[0, 0, 0, 0])
    H["unmapped_se"] = build(reads, g, CO, CN, 0, with_qual=False)
    # read names of 1 and 300 bytes, a read of 1024 bases, no qualities
    reads = [("x", 1024, [aln(1, 100, 0, "1000M1D20M4S", mm=(0, 511, 512, 1019))]), ("y" * 300, 70, [aln(0, 33, 1, "70M")])]
    H["long"] = build(reads, g, CO, CN, 1)
    H["long_no_qual"] = build(reads, g, CO, CN, 1, with_qual=False)
    return H


@functools.lru_cache(maxsize=None)
def big_pos():
    """POS across 999 999 999 / 1 000 000 000: one contig of 10^9 + 200 bases, all A but for its last 400."""
    L = 1_000_000_200
    text = np.zeros(2 * L, dtype=np.uint8)
    tail = genome(400, 4207)
    text[L - 400:L] = tail
    text[L:L + 400] = 3 - tail[::-1]
    reads = [("big", 60, [aln(0, 999_999_998, 0, "60M", mm=(30,))]), ("big", 60, [aln(0, 999_999_999, 1, "2S58M")])]
    j = build(reads, None, np.array([0, L], np.int64), ["huge"], 1, text=text)
    j["text_window"] = (L - 400, 800)
    return j


def expected():
    """name -> the lines the hand-built job must give, written out."""
    with open(os.path.join(HERE, "golden", "mem_sam_example.json")) as f:
        long = json.load(f)["lines"]
    return dict(EXPECT, **long)


# the lines of the short cases, read from the rules by hand (SEQ and QUAL come from the builder's generator, everything else from
# the case's definition above)
EXPECT = {
    'tlen': (
        "fr\t99\tchr1\t101\t60\t50M\t=\t301\t250\tTGTCGGCTCGCGGCGCCCAGACTGACCCTGGCGTGAAAGCGGTCAATATG\t3)I'6G6EE@?88C2GE01>F$#+2'67G?+AB<<->&:FH-.:1>)'#4\tNM:i:0\tMD:Z:50\tMC:Z:50M\tAS:i:50\tXS:i:0\n"
        'fr\t147\tchr1\t301\t0\t50M\t=\t101\t-250\tAACGGCTCCTCAAAATACATGTCAATCTCGTAGGTTTTTATATTGAGTAG\t"\'"-FB6ED?A=FF%C>EB=@!1<#?($;1:*4?H&-0<39(4F9?%9CB\tNM:i:1\tMD:Z:3C46\tMC:Z:50M\tAS:i:45\tXS:i:0\n'
        'rf\t81\tchr1\t501\t60\t40M\t=\t421\t-120\tCCGAATTCCAGAGGTGTAGAGGGCCAGAATCCGGTGGTTC\tEH4A*"08@(*:);2B;7DG8-3!$<%\'%9-"+8H(G+=+\tNM:i:0\tMD:Z:40\tMC:Z:40M\tAS:i:40\tXS:i:0\n'
        "rf\t161\tchr1\t421\t60\t40M\t=\t501\t120\tCGGAGGGCTCACAACTACCCAGACCGAGGAGAGCGTACTC\t8.C.'%-:&A--<D2A-&B@?E5)880;+9A$3<#:FB=A\tNM:i:0\tMD:Z:40\tMC:Z:40M\tAS:i:40\tXS:i:0\n"
        'same\t67\tcontig_two\t78\t60\t30M\t=\t78\t0\tTCCGAAGAGTGGGGCCGCTATCCACCTATA\t>-D4E&\'/"5;<)\'8:GE0\'+E3I;9%90C\tNM:i:0\tMD:Z:30\tMC:Z:30M\tAS:i:30\tXS:i:0\n'
        "same\t131\tcontig_two\t78\t60\t30M\t=\t78\t0\tTCCGAAGAGTGGGGCCGCTATCCACCTATA\t<C60-0<7-)>+).C39$/?@8D-'$)@F&\tNM:i:0\tMD:Z:30\tMC:Z:30M\tAS:i:30\tXS:i:0\n"
        'meet\t99\tcontig_two\t201\t60\t30M\t=\t201\t0\tGCTTCTTTTGGGCCGGTCACCGTTCCATGA\t&;$?F>,C-?C4:D(!2(ED0->3$<>#@6\tNM:i:0\tMD:Z:30\tMC:Z:1M\tAS:i:30\tXS:i:0\n'
        'meet\t147\tcontig_two\t201\t60\t1M\t=\t201\t0\tG\t.\tNM:i:0\tMD:Z:1\tMC:Z:30M\tAS:i:1\tXS:i:0\n'
    ),
    'indels': (
        "d_i\t0\tchr1\t901\t60\t20M2D10M3I27M\t*\t0\t0\tGCGTGCGTATTCAAGTCTAGTGTGGGGTCAGGGGAGCCAAGTAGTATCTGACGGAACATA\t&C2CBH!D:4AH6$>**()F/%(1/-GD8I.&,$H)3)I'6G6EE@?88C2GE01>F$#+\tNM:i:6\tMD:Z:5A14^GC37\tAS:i:27\tXS:i:0\n"
        "d_mm\t0\tchr1\t1001\t60\t20M3D20M\t*\t0\t0\tCGAACAATTATTAGTTGCCATACACGAGGCGGGCCGGGGG\t7G?+AB<<->&:FH-.:1>)'#4)-FBC9%?9F4(93<0-\tNM:i:5\tMD:Z:19T0^GGT0G19\tAS:i:15\tXS:i:0\n"
        'd_last\t0\tchr1\t1101\t60\t25M2D5S\t*\t0\t0\tTGTTAATATGCACTGTACGCGCTATGTAGC\t4*:1;$(?#<1!@=BE>C%FF=A?DE6BF-\tNM:i:0\tMD:Z:25\tAS:i:25\tXS:i:0\n'
        'd_first\t16\tchr1\t1151\t60\t4S2D26M\t*\t0\t0\tTGCACTTGGTTATGGAATCTTCACAGTTAT\t;2B;7DG8-3!$<%\'%9-"+8H(G+=++!2\tNM:i:1\tMD:Z:0A25\tAS:i:21\tXS:i:0\n'
        'i_rev\t16\tcontig_two\t601\t60\t3S10M1I10M1D21M\t*\t0\t0\tCCTGAGTAGGATAAGCGAAGCAGATCAGACAACTTCAAGGCCACC\t$A9+;088)5E?@B&-A2D<--A&:-%\'.C.8#!DEH4A*"08@(\tNM:i:3\tMD:Z:10C9^C21\tAS:i:26\tXS:i:0\n'
        'd_d\t0\tcontig_two\t701\t60\t10M1D10M1D10M\t*\t0\t0\tTATCCTGATTTTGTCCCATCCGTTTACCGA\t:FB=A/.$>-D4E&\'/"5;<)\'8:GE0\'+E\tNM:i:2\tMD:Z:10^T10^G10\tAS:i:20\tXS:i:0\n'
    ),
    'n_bases': (
        "n_read\t0\tchr1\t401\t60\t30M\t*\t0\t0\tACCGNGAAGATATAAGCGCCCGGAGGGCTN\t393;7<H'83/*#1B$1HH)!<!-5D$<6&\tNM:i:2\tMD:Z:4A24C0\tAS:i:20\tXS:i:0\n"
        'n_text\t0\tchr1\t691\t60\t30M\t*\t0\t0\tGTGATCAACTNNACCGCAGCGGAACTGAAT\tG9FH8,&8(?G+7#(0EH;88#0I1)*>"H\tNM:i:0\tMD:Z:30\tAS:i:30\tXS:i:0\n'
        'n_both\t16\tchr1\t696\t60\t30M\t*\t0\t0\tCAACTNNANCGCAGCGGAACTGAATTTAAC\t=,9#/<D26$2>;%H2&F"A0>"#?3.47@\tNM:i:1\tMD:Z:8C21\tAS:i:25\tXS:i:0\n'
        "n_text_del\t0\tcontig_two\t791\t60\t9M2D21M\t*\t0\t0\tAGCCCGTACCATGTCTCTCTATGCGTGCAT\t66@AFI'1G-!8??B;&C2CBH!D:4AH6$\tNM:i:2\tMD:Z:9^TN21\tAS:i:20\tXS:i:0\n"
    ),
    'unmapped': (
        "u_rev\t117\tcontig_two\t51\t0\t*\t=\t51\t0\tAACCCCGGAGCGGGAGTATAGTAAGGTTAACACCA\t;B??8!-G1'IFA@66F/D=,9#/<D26$2>;%H2\tMC:Z:5S30M\tAS:i:0\tXS:i:0\n"
        'u_rev\t185\tcontig_two\t51\t60\t5S30M\t=\t51\t0\tCATTTTATCCGCGTATTCTGAACTCGGCCTCCTCC\t)3)H$,&.I8DG-/1(%/F)(**>$6HA4:D!HBC\tNM:i:0\tMD:Z:30\tAS:i:30\tXS:i:0\n'
        'u_fwd\t73\tchr1\t11\t60\t20M\t=\t11\t0\tCCGATGCAATCATCGAGGTT\tG6EE@?88C2GE01>F$#+2\tNM:i:0\tMD:Z:20\tAS:i:20\tXS:i:0\n'
        "u_fwd\t133\tchr1\t11\t0\t*\t=\t11\t0\tAGCAAGGGGTGCGGAAGCGCAACTC\tG?+AB<<->&:FH-.:1>)'#4)-F\tMC:Z:20M\tAS:i:0\tXS:i:0\n"
        'none\t77\t*\t0\t0\t*\t*\t0\t0\tCGTCGCGCGGGT\t%?9F4(93<0-&\tAS:i:0\tXS:i:0\n'
        'none\t141\t*\t0\t0\t*\t*\t0\t0\tAGCCAACTACTTA\t*:1;$(?#<1!@=\tAS:i:0\tXS:i:0\n'
        'apart\t97\tchr1\t1401\t60\t30M\tcontig_two\t1\t0\tCGTCCACTCCTATACCCATCATGTATAGAC\tC%FF=A?DE6BF-"\'"2!++=+G(H8+"-9\tNM:i:0\tMD:Z:30\tMC:Z:30M\tAS:i:30\tXS:i:0\n'
        'apart\t145\tcontig_two\t1\t17\t30M\tchr1\t1401\t0\tCTGGACAACGTTGAAAAACCGCCTCTCGGA\t8#!DEH4A*"08@(*:);2B;7DG8-3!$<\tNM:i:0\tMD:Z:30\tMC:Z:30M\tAS:i:30\tXS:i:0\n'
    ),
    'unmapped_se': (
        'u_rev\t4\t*\t0\t0\t*\t*\t0\t0\tTGGTGTTAACCTTACTATACTCCCGCTCCGGGGTT\t*\tAS:i:0\tXS:i:0\n'
        'u_rev\t16\tcontig_two\t51\t60\t5S30M\t*\t0\t0\tCATTTTATCCGCGTATTCTGAACTCGGCCTCCTCC\t*\tNM:i:0\tMD:Z:30\tAS:i:30\tXS:i:0\n'
        'u_fwd\t0\tchr1\t11\t60\t20M\t*\t0\t0\tCCGATGCAATCATCGAGGTT\t*\tNM:i:0\tMD:Z:20\tAS:i:20\tXS:i:0\n'
        'u_fwd\t4\t*\t0\t0\t*\t*\t0\t0\tAGCAAGGGGTGCGGAAGCGCAACTC\t*\tAS:i:0\tXS:i:0\n'
        'none\t4\t*\t0\t0\t*\t*\t0\t0\tCGTCGCGCGGGT\t*\tAS:i:0\tXS:i:0\n'
        'none\t4\t*\t0\t0\t*\t*\t0\t0\tAGCCAACTACTTA\t*\tAS:i:0\tXS:i:0\n'
        'apart\t0\tchr1\t1401\t60\t30M\t*\t0\t0\tCGTCCACTCCTATACCCATCATGTATAGAC\t*\tNM:i:0\tMD:Z:30\tAS:i:30\tXS:i:0\n'
        'apart\t16\tcontig_two\t1\t17\t30M\t*\t0\t0\tCTGGACAACGTTGAAAAACCGCCTCTCGGA\t*\tNM:i:0\tMD:Z:30\tAS:i:30\tXS:i:0\n'
    ),
}
