"""SAM records, cs / MD tags and = / X CIGAR operations of minimap2's aligned regions (include/gbx.h): the text stage
behind mm_align, beside its PAF text.

``DeviceMmSam`` takes a ``DeviceMmAligner`` and queues behind it on the same stream.  All arithmetic in libgbx.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import mm_align as MA
from . import mm_map as MM
from . import mm_stage as ST
from .mm_stage import c as _c, pad as _pad

PAF, SAM = 0, 1
CS_NONE, CS_SHORT, CS_LONG = 0, 1, 2


class MmSamParams(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("format", "cs", "md", "eqx", "softclip")]


@N.declare_once
def lib(L):
    """libgbx.so with the gbx_mm_sam_* entries declared"""
    vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
    P = C.POINTER(MmSamParams)
    L.gbx_mm_sam_default_params.argtypes = [P]
    L.gbx_mm_sam_default_params.restype = None
    L.gbx_mm_sam_check_params.argtypes = [P]
    L.gbx_mm_sam_workspace_bytes.argtypes = [i64, i64]
    L.gbx_mm_sam_workspace_bytes.restype = sz
    L.gbx_mm_sam_device.argtypes = [P, i64, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, sz, vp]
    L.gbx_mm_sam_host.argtypes = [P, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp, C.POINTER(C.c_int64), vp]


def make_params(**kw):
    """gbx_mm_sam_default_params (every field 0) with the given fields replaced"""
    return N.fill_params(MmSamParams, lib().gbx_mm_sam_default_params, kw, "gbx_mm_sam_params")


def check_params(p):
    N.check(lib().gbx_mm_sam_check_params(C.byref(p)))


def header(tnames, tlens, args=()):
    """the SAM header the driver writes: @HD, one @SQ a contig, @PG with the command line"""
    names = [s.decode() if isinstance(s, bytes) else s for s in tnames]
    out = ["@HD\tVN:1.6\tSO:unsorted\tGO:query"] + ["@SQ\tSN:%s\tLN:%d" % (s, int(n)) for s, n in zip(names, tlens)]
    out.append("@PG\tID:mmpaf\tPN:mmpaf\tCL:" + " ".join(["mmpaf"] + list(args)))
    return "\n".join(out) + "\n"


def text_room(p, n_reads, n_regs, names, cigar_words, bases):
    """room for the text of n_regs regions of n_reads reads of `bases` bases in all: a bound for well-formed alignments whose reads
    have few regions each, not a promise - counts() reports the need"""
    line = ST.LINE_ROOM + ST.TAG_ROOM + names
    return (n_regs * (line + 4 * (names + 64)) + n_reads * (names + 32) + 11 * cigar_words * (2 if p.eqx else 1) +
            bases * (6 * p.format + 4 * (p.cs != 0) + 3 * p.md + 3 * p.eqx))


def _text(entry, host, p, regs, reg_off, alns, cigar, qnames, reads, quals, rep_len, tnames, refs, text_cap):
    reg_off = _c(reg_off, np.int64)
    n = len(reg_off) - 1
    regs, alns, cigar = _c(regs, MM.REG_DTYPE), _c(alns, MA.ALN_DTYPE), _c(cigar, np.uint32)
    qn, qo = ST.pack_seqs(qnames)
    tn, to = ST.pack_seqs(tnames)
    seq, so = ST.pack_seqs(reads)
    tseq, tso = ST.pack_seqs(refs)
    qual = None
    if quals is not None:
        qual, qlo = ST.pack_seqs(quals)
        if not np.array_equal(qlo, so):
            raise N.GbxError(N.GBX_ERR_ARG, "mm_sam: the qualities do not have the reads' lengths")
        qual = _pad(qual)
    line_off, cnt, nt = np.zeros(n + 1, np.int64), np.zeros(2, np.int64), C.c_int64(0)
    ins = [C.byref(p), n, N.ptr(_pad(regs)), N.ptr(reg_off), N.ptr(_pad(alns)), N.ptr(_pad(cigar)), len(cigar), N.ptr(_pad(qn)), N.ptr(qo), N.ptr(_pad(seq)),
           None if qual is None else N.ptr(qual), N.ptr(so), N.ptr(_pad(_c(rep_len, np.int32))), len(to) - 1, N.ptr(_pad(tn)), N.ptr(to), N.ptr(_pad(tseq)),
           N.ptr(tso)]

    def call(lines, cap):
        """-> (status, the bytes needed)"""
        if host:
            rc = entry(*ins, N.ptr(lines), cap, N.ptr(line_off), C.byref(nt), N.ptr(cnt))
            return rc, nt.value
        return 0, entry(*ins, N.ptr(lines), cap, N.ptr(line_off), N.ptr(cnt))
    if text_cap is None:                                     # sized by a call without room, which reports the need
        rc, text_cap = call(None, 0)
        if rc not in (0, N.GBX_ERR_ARG):
            N.check(rc)
    lines = np.zeros(max(text_cap, 1), np.uint8)
    rc, need = call(lines, text_cap)
    if rc == N.GBX_ERR_ARG and need > text_cap:
        raise N.GbxError(rc, "mm_sam: %d bytes of text do not fit text_cap = %d" % (need, text_cap))
    N.check(rc)
    return dict(text=lines[:min(need, text_cap)].tobytes(), line_off=line_off, n_text=int(need), counts=(int(cnt[0]), int(cnt[1])))


def sam_host(p, regs, reg_off, alns, cigar, qnames, reads, quals, rep_len, tnames, refs, text_cap=None):
    """gbx_mm_sam_host -> dict(text, line_off, n_text, counts = (lines, regions that print nothing)).  quals None: QUAL is `*`.
    A text_cap too small raises GBX_ERR_ARG naming the need."""
    return _text(lib().gbx_mm_sam_host, True, p, regs, reg_off, alns, cigar, qnames, reads, quals, rep_len, tnames, refs, text_cap)


def sam_cpu(p, regs, reg_off, alns, cigar, qnames, reads, quals, rep_len, tnames, refs, text_cap=None, lanes=1):
    """the host build of the same rules (mm_sam_rules.h in libgbx_mm_cpu.so) -> the dict sam_host gives; a text_cap too small is not
    an error here: n_text reports the need and nothing is written past the capacity.  lanes: 1, or a team of 2 .. 64 host threads
    that meet at every ballot, scan and shuffle as a wavefront's lanes do"""
    entry = ST.twin().gbx_mm_sam_cpu if lanes == 1 else (lambda P, *a: ST.twin().gbx_mm_sam_cpu_lanes(P, lanes, *a))
    return _text(entry, False, p, regs, reg_off, alns, cigar, qnames, reads, quals, rep_len, tnames, refs, text_cap)


class DeviceMmSam(ST.Fits):
    """The alignments of a DeviceMmAligner -> SAM records, or PAF lines with cs / MD / eqx, queued behind the aligner on its stream.
    quals: the reads' quality strings (None: QUAL prints `*`).  text_cap None: sized from what the aligner knows (text_room);
    counts() reports the need when a capacity was too small."""

    FIT = (("bytes of text", 2, "text_cap"),)

    def __init__(self, aligner, p=None, quals=None, text_cap=None):
        import torch
        self.aligner, self.mapper, self.device = aligner, aligner.mapper, aligner.device
        self.p = make_params() if p is None else p
        check_params(self.p)
        sd = self.mapper.seeder
        self.qual = None
        if quals is not None:
            q, qo = ST.pack_seqs(quals)
            if not np.array_equal(qo, sd.seq_off.cpu().numpy()):
                raise N.GbxError(N.GBX_ERR_ARG, "mm_sam: the qualities do not have the reads' lengths")
            self.qual = torch.from_numpy(_pad(q)).to(self.device)
        self.cap = text_cap
        self.cnt = torch.zeros(3, dtype=torch.int64, device=self.device)          # lines, regions that print nothing, bytes of text
        self.line_off = torch.zeros(sd.n_reads + 1, dtype=torch.int64, device=self.device)
        self.sized_for = None

    def _size(self):
        import torch
        al, mp, sd = self.aligner, self.mapper, self.mapper.seeder
        al._size()
        key = (mp.reg_cap, al.cigar_cap)
        if self.sized_for == key:
            return
        e = ST.allocator(self.device)
        bases = int(sd.text.numel())
        self.text_cap = text_room(self.p, sd.n_reads, mp.reg_cap, mp.name_room, al.cigar_cap, bases) if self.cap is None else int(self.cap)
        self.lines = e(self.text_cap, torch.uint8)
        self.work_bytes = lib().gbx_mm_sam_workspace_bytes(sd.n_reads, mp.reg_cap)
        self.work = e(self.work_bytes, torch.uint8)
        self.sized_for = key

    def run(self, stream=None):
        """the text, queued on `stream` behind the aligner's run_align()"""
        self._size()
        al, mp, sd, ix = self.aligner, self.mapper, self.mapper.seeder, self.mapper.seeder.index
        N.check(lib().gbx_mm_sam_device(C.byref(self.p), sd.n_reads, mp.regs.data_ptr(), mp.reg_off.data_ptr(), mp.cnt.data_ptr() + 8, mp.reg_cap,
                                        al.alns.data_ptr(), al.cigar.data_ptr(), al.cigar_cap, mp.qnames.data_ptr(), mp.qname_off.data_ptr(),
                                        sd.text.data_ptr(), None if self.qual is None else self.qual.data_ptr(), sd.seq_off.data_ptr(),
                                        sd.rep_len.data_ptr(), ix.n_seqs, mp.tnames.data_ptr(), mp.tname_off.data_ptr(), ix.text.data_ptr(),
                                        ix.off.data_ptr(), self.lines.data_ptr(), self.text_cap, self.line_off.data_ptr(), self.cnt.data_ptr() + 16,
                                        self.cnt.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))

    def counts(self):
        """(lines, regions that print nothing, bytes of text) of the last run().  Synchronises."""
        return tuple(int(v) for v in self.cnt.cpu().numpy())

    def results(self):
        self._need_fit()
        return dict(line_off=self.line_off.cpu().numpy())

    def text(self):
        """the text of the last run(), without a header"""
        self.mapper._need_fit()
        self.aligner._need_fit()
        _, _, t = self._need_fit()
        return self.lines[:t].cpu().numpy().tobytes().decode()
