"""Base-level alignment of minimap2's regions (include/gbx.h): CIGAR, NM and the DP scores of every region, and the PAF
text with ``cg:Z:``.

``DeviceMmAligner`` takes a ``DeviceMmMapper`` and queues behind it on the same stream; ``DeviceMmMapper(align=...)`` does that
itself.  All arithmetic in libgbx.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import mm_map as MM
from . import mm_stage as ST
from .mm_stage import TAG_ROOM, c as _c, pad as _pad, twin as _twin      # noqa: F401  (TAG_ROOM: part of this module's interface)

ALN_DTYPE = np.dtype([(k, "<i4") for k in ("rs", "re", "qs", "qe", "mlen", "blen", "n_ambi", "nm", "dp_score", "dp_max", "n_cigar", "flags")] +
                     [("cigar_off", "<i8")])
assert ALN_DTYPE.itemsize == 56                              # sizeof(gbx_mm_aln)
ALIGNED, ZDROP_L, ZDROP_R, END_L, END_R, NO_ROOM, INVALID = 1, 2, 4, 8, 16, 32, 64


class MmAlignParams(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("a", "b", "sc_ambi", "q", "e", "q2", "e2", "bw", "zdrop", "end_bonus", "min_ksw_len", "max_ext")]


@N.declare_once
def lib(L):
    """libgbx.so with the gbx_mm_align_* and gbx_mm_paf_cigar_* entries declared"""
    vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
    P = C.POINTER(MmAlignParams)
    L.gbx_mm_align_default_params.argtypes = [P]
    L.gbx_mm_align_default_params.restype = None
    L.gbx_mm_align_check_params.argtypes = [P]
    L.gbx_mm_align_workspace_bytes.argtypes = [i64, i64, i64]
    L.gbx_mm_align_workspace_bytes.restype = sz
    L.gbx_mm_align_device.argtypes = [P, i64, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, sz, vp]
    L.gbx_mm_align_host.argtypes = [P, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, i64, vp]
    L.gbx_mm_paf_cigar_workspace_bytes.argtypes = [i64, i64]
    L.gbx_mm_paf_cigar_workspace_bytes.restype = sz
    L.gbx_mm_paf_cigar_device.argtypes = [i64, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, sz, vp]
    L.gbx_mm_paf_cigar_host.argtypes = [i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, C.POINTER(C.c_int64)]


def make_params(**kw):
    """gbx_mm_align_default_params with the given fields replaced"""
    return N.fill_params(MmAlignParams, lib().gbx_mm_align_default_params, kw, "gbx_mm_align_params")


def check_params(p):
    N.check(lib().gbx_mm_align_check_params(C.byref(p)))


def _inputs(regs, reg_off, off, cax, cay, n_chained, reads, refs):
    seq, seq_off = ST.pack_seqs(reads)
    tseq, tseq_off = ST.pack_seqs(refs)
    return (_c(regs, MM.REG_DTYPE), _c(reg_off, np.int64), _c(off, np.int64), _pad(_c(cax, np.uint64)), _pad(_c(cay, np.uint64)),
            _pad(_c(n_chained, np.int32)), _pad(seq), seq_off, _pad(tseq), tseq_off)


def _cut(alns, cigar, cnt):
    return dict(alns=alns, cigar=cigar[:max(min(int(cnt[1]), len(cigar)), 0)], counts=tuple(int(v) for v in cnt))


def align_host(p, regs, reg_off, off, cax, cay, n_chained, reads, refs, cigar_cap=None, z_bytes=None):
    """gbx_mm_align_host -> dict(alns, cigar, counts = (jobs, words, bytes of z)).  z_bytes None: sized by a first call with 0, which
    plans and reports the need without running a job; cigar_cap None: the bound of 2 qlen + 1 words a region."""
    g, ro, off, cx, cy, nc, seq, so, tseq, to = _inputs(regs, reg_off, off, cax, cay, n_chained, reads, refs)
    n, nr = len(ro) - 1, len(g)
    alns, cnt = np.zeros(max(nr, 1), ALN_DTYPE), np.zeros(3, np.int64)

    def call(cc, zb, cig):
        return lib().gbx_mm_align_host(C.byref(p), n, N.ptr(g), N.ptr(ro), N.ptr(off), N.ptr(cx), N.ptr(cy), N.ptr(nc), N.ptr(seq), N.ptr(so), len(to) - 1,
                                       N.ptr(tseq), N.ptr(to), N.ptr(alns), N.ptr(cig), cc, zb, N.ptr(cnt))

    def size(rc):                                            # a short capacity is GBX_ERR_ARG with the need in cnt
        if rc not in (0, N.GBX_ERR_ARG):
            N.check(rc)
    if z_bytes is None:
        size(call(0, 0, None))
        z_bytes = int(cnt[2])
    if cigar_cap is None:                                    # a region's CIGAR has at most 2 qlen + 1 words: no counting run of the DP
        cigar_cap = int((np.diff(ro) * (2 * np.diff(so) + 1)).sum())
    cig = np.zeros(max(cigar_cap, 1), np.uint32)
    N.check(call(cigar_cap, z_bytes, cig))
    return _cut(alns[:nr], cig, cnt)


def align_cpu(p, regs, reg_off, off, cax, cay, n_chained, reads, refs, cigar_cap=None, z_bytes=None):
    """The same rules compiled for the host (mm_align_rules.h in libgbx_mm_cpu.so), one thread -> the dict align_host gives.
    z_bytes None: room for everything."""
    g, ro, off, cx, cy, nc, seq, so, tseq, to = _inputs(regs, reg_off, off, cax, cay, n_chained, reads, refs)
    T = _twin()
    n, nr = len(ro) - 1, len(g)
    alns, cnt = np.zeros(max(nr, 1), ALN_DTYPE), np.zeros(3, np.int64)
    zb = (1 << 62) if z_bytes is None else z_bytes

    def call(cc, cig):
        T.gbx_mm_align_cpu(C.byref(p), n, nr, N.ptr(g), N.ptr(off), N.ptr(cx), N.ptr(cy), N.ptr(nc), N.ptr(seq), N.ptr(so), len(to) - 1, N.ptr(tseq), N.ptr(to),
                           N.ptr(alns), N.ptr(cig), cc, zb, N.ptr(cnt))
    if cigar_cap is None:
        call(0, None)
        cigar_cap = int(cnt[1])
    cig = np.zeros(max(cigar_cap, 1), np.uint32)
    call(cigar_cap, cig)
    return _cut(alns[:nr], cig, cnt)


def job_cpu(p, target, query, w, mode, ext):
    """One DP job of the host build on plain sequences -> dict(score, end_t, end_q, flags, ct, cq, cigar); mode 0 LEFT / 1 RIGHT"""
    t, q = np.frombuffer(bytes(target), np.uint8), np.frombuffer(bytes(query), np.uint8)
    out, cig = np.zeros(6, np.int32), np.zeros(len(t) + len(q) + 1, np.uint32)
    n = _twin().gbx_mm_align_cpu_job(C.byref(p), N.ptr(t), len(t), N.ptr(q), len(q), w, mode, int(ext), N.ptr(out), N.ptr(cig), len(cig))
    return dict(score=int(out[0]), end_t=int(out[1]), end_q=int(out[2]), flags=int(out[3]), ct=int(out[4]), cq=int(out[5]), cigar=cig[:n])


def paf_cigar_host(regs, reg_off, alns, cigar, qnames, seq_off, rep_len, tnames, tseq_off, text_cap=None):
    """gbx_mm_paf_cigar_host -> (text bytes, line_off)"""
    return ST.paf_text(lib().gbx_mm_paf_cigar_host, _c(regs, MM.REG_DTYPE), reg_off, qnames, seq_off, rep_len, tnames, tseq_off, text_cap,
                       _c(alns, ALN_DTYPE), cigar)


def paf_cigar_cpu(regs, reg_off, alns, cigar, qnames, seq_off, rep_len, tnames, tseq_off):
    """the host build of the same line rules -> (text bytes, line_off)"""
    return ST.paf_text(_twin().gbx_mm_paf_cigar_cpu, _c(regs, MM.REG_DTYPE), reg_off, qnames, seq_off, rep_len, tnames, tseq_off, None,
                       _c(alns, ALN_DTYPE), cigar, host=False)


class DeviceMmAligner(ST.Fits):
    """The regions of a DeviceMmMapper -> records, CIGAR words and PAF text with cg:Z:, queued behind the mapper on its stream.
    cigar_cap / z_bytes / text_cap None: sized from what the mapper knows once its anchors are counted - a region's words from its
    reads' bases (cigar_cap = the bases of all reads / 2 + 8 a region), z from `z_per_base` bytes a read base (None: two diagonals of bw + 1 cells and the rows), the text from both.
    counts() reports the needs when a capacity was too small.  z is one allocation for the whole read set (about 1 000 bytes a read
    base at the default band): a read set that does not fit the device that way is aligned a batch of reads a mapper."""

    FIT = (("CIGAR words", 1, "cigar_cap"), ("bytes of z", 2, "z_bytes"), ("bytes of text", 3, "text_cap"))      # the jobs (0) have no capacity

    def __init__(self, mapper, p=None, cigar_cap=None, z_bytes=None, text_cap=None, z_per_base=None):
        import torch
        self.mapper, self.device = mapper, mapper.device
        self.p = make_params() if p is None else p
        check_params(self.p)
        self.caps = (cigar_cap, z_bytes, text_cap)
        self.z_per_base = 2 * (min(self.p.bw, 4096) + 1) + 200 if z_per_base is None else z_per_base
        self.cnt = torch.zeros(4, dtype=torch.int64, device=self.device)          # jobs, words, bytes of z, bytes of text
        self.line_off = torch.zeros(mapper.seeder.n_reads + 1, dtype=torch.int64, device=self.device)
        self.sized_for = None

    def _size(self):
        import torch
        mp, sd, L = self.mapper, self.mapper.seeder, lib()
        key = (mp.reg_cap, sd.anchor_cap)
        if self.sized_for == key:
            return
        e = ST.allocator(self.device)
        cc, zb, tc = self.caps
        bases = int(sd.text.numel())
        self.cigar_cap = bases // 2 + 8 * mp.reg_cap if cc is None else int(cc)
        self.z_bytes = (bases * self.z_per_base + 15) & ~15 if zb is None else int(zb)
        self.text_cap = ST.text_cap(mp.reg_cap, mp.name_room, True, self.cigar_cap) if tc is None else int(tc)
        self.alns = e(mp.reg_cap * ALN_DTYPE.itemsize, torch.uint8)
        self.cigar = e(self.cigar_cap, torch.int32)
        self.z = e(self.z_bytes, torch.uint8)
        self.lines = e(self.text_cap, torch.uint8)
        self.work_bytes = L.gbx_mm_align_workspace_bytes(sd.n_reads, mp.reg_cap, sd.anchor_cap)
        self.work = e(self.work_bytes, torch.uint8)
        self.paf_work_bytes = L.gbx_mm_paf_cigar_workspace_bytes(sd.n_reads, mp.reg_cap)
        self.paf_work = e(self.paf_work_bytes, torch.uint8)
        self.sized_for = key

    def run_align(self, stream=None):
        self._size()
        mp, sd, ix = self.mapper, self.mapper.seeder, self.mapper.seeder.index
        N.check(lib().gbx_mm_align_device(C.byref(self.p), sd.n_reads, mp.regs.data_ptr(), mp.reg_off.data_ptr(), mp.cnt.data_ptr() + 8, mp.reg_cap,
                                          sd.off.data_ptr(), mp.cax.data_ptr(), mp.cay.data_ptr(), mp.n_chained.data_ptr(), sd.anchor_cap,
                                          sd.text.data_ptr(), sd.seq_off.data_ptr(), ix.n_seqs, ix.text.data_ptr(), ix.off.data_ptr(),
                                          self.alns.data_ptr(), self.cigar.data_ptr(), self.cigar_cap, self.cnt.data_ptr(), self.z.data_ptr(), self.z_bytes,
                                          self.work.data_ptr(), self.work_bytes, stream))

    def run_paf(self, stream=None):
        mp, sd, ix = self.mapper, self.mapper.seeder, self.mapper.seeder.index
        N.check(lib().gbx_mm_paf_cigar_device(sd.n_reads, mp.regs.data_ptr(), mp.reg_off.data_ptr(), mp.cnt.data_ptr() + 8, mp.reg_cap, self.alns.data_ptr(),
                                              self.cigar.data_ptr(), self.cigar_cap, mp.qnames.data_ptr(), mp.qname_off.data_ptr(), sd.seq_off.data_ptr(),
                                              sd.rep_len.data_ptr(), ix.n_seqs, mp.tnames.data_ptr(), mp.tname_off.data_ptr(), ix.off.data_ptr(),
                                              self.lines.data_ptr(), self.text_cap, self.line_off.data_ptr(), self.cnt.data_ptr() + 24,
                                              self.paf_work.data_ptr(), self.paf_work_bytes, stream))

    def run(self, stream=None):
        """align -> PAF with CIGAR, queued on `stream` behind the mapper's run_map()"""
        self.run_align(stream)
        self.run_paf(stream)

    def counts(self):
        """(jobs, CIGAR words, bytes of z, bytes of text) of the last run().  Synchronises."""
        return tuple(int(v) for v in self.cnt.cpu().numpy())

    def results(self):
        """dict(alns, cigar, line_off) as numpy arrays, cut to the counts"""
        _, w, _, _ = self._need_fit()
        r = self.mapper.counts()[1]
        return dict(alns=self.alns[:r * ALN_DTYPE.itemsize].cpu().numpy().view(ALN_DTYPE), cigar=self.cigar[:w].cpu().numpy().view(np.uint32),
                    line_off=self.line_off.cpu().numpy())

    def paf(self):
        _, _, _, t = self._need_fit()
        return self.lines[:t].cpu().numpy().tobytes().decode()
